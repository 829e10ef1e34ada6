// Diversified selection (DESIGN.md "Diversified search"): maximal-marginal-relevance picks out of a per-query candidate list,
// by the rule include/tt.h states at tt_mmr_select_f32.  One workgroup of four waves per query, in three phases:
//  1 gather  the C candidate rows by id like score_ids_kernel: whole 16-byte pieces, the row address from the candidate's id,
//            invalid candidates read nothing (their image rows are zeros).  32 features at a time into a 33-float-stride LDS
//            image; the pieces of the next 32 features are in flight while the current ones are multiplied.
//  2 Gram    G = X X^T on v_mfma_f32_32x32x2_f32: the upper-triangle 32x32 tiles are dealt to the waves, every tile's
//            accumulator stays in registers over the whole feature loop (features ascending, two per instruction: the fp32
//            fmaf chain of the oracle, bit for bit), and is written once -- mirrored, G is bitwise symmetric -- into the LDS
//            Gram that then takes the image's place.
//  3 greedy  wave 0 alone: a lane owns candidates lane and lane + 64 (a_c, pen_c and the taken flag in registers), the
//            argmax over (m desc, position asc) is a wave maximum (DPP inside rows of 16, then four scalars) and a ballot; after a pick row s of G (= column s) is read
//            with consecutive lanes on consecutive words.  No workgroup barrier inside the loop.
#include <limits.h>
#include <math.h>

#include "tt_common.h"

// The rule's m_c is two rounded products and one rounded subtraction.  hipcc contracts by default, and __fmul_rn / __fsub_rn do
// not stop it: in this toolchain's headers they are plain operators compiled under the default mode, so the pair still fuses
// into fma(-mu, pen, a) (seen in the ISA, and in the picks).  Hence plain operators under contract(off), for the whole file.
// (The Gram's chain is the MFMA instruction's own; no source-level multiply-add is meant to fuse here.)
#pragma clang fp contract(off)

namespace {

constexpr int MMR_THREADS = 256;
constexpr int MMR_WAVES = MMR_THREADS / TT_WAVE;
constexpr int MMR_FEAT = 32;                 // features per staged block
constexpr int MMR_STRIDE = MMR_FEAT + 1;     // image stride in floats
constexpr int MMR_CMAX = 128, MMR_KMAX = 128;
constexpr size_t MMR_NO_ROW = ~(size_t)0;    // row offset of a candidate that is never read

enum { MMR_F32 = 0, MMR_BF16 = 1, MMR_ROWS = 2 };

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// One 32-feature block of the workgroup's CMAX rows, in registers: pass i holds rows ROWS * i + tid / LANES, 16 bytes per thread.
template <int CMAX, bool BF16>
struct MmrPieces {
    static constexpr int LANES = BF16 ? 4 : 8;              // threads per row: 64-byte (bf16) / 128-byte (fp32) segments
    static constexpr int ELEMS = MMR_FEAT / LANES;          // features per thread
    static constexpr int ROWS = MMR_THREADS / LANES;        // rows per pass
    static constexpr int PASSES = (CMAX + ROWS - 1) / ROWS;
    u32x4 v[PASSES];

    __device__ __forceinline__ void load(const void *D, const size_t *row_off, int x0, int d, int tid)
    {
        const int x = x0 + ELEMS * (tid % LANES);
#pragma unroll
        for (int i = 0; i < PASSES; ++i) {
            v[i] = u32x4{0u, 0u, 0u, 0u};
            if (x < d && row_off[i] != MMR_NO_ROW) {
                if (BF16)
                    v[i] = *(const u32x4 *)((const uint16_t *)D + row_off[i] + x);
                else
                    v[i] = *(const u32x4 *)((const float *)D + row_off[i] + x);
            }
        }
    }

    __device__ __forceinline__ void store(float *img, int tid) const
    {
#pragma unroll
        for (int i = 0; i < PASSES; ++i) {
            const int r = ROWS * i + tid / LANES;
            if (r < CMAX) {
                float *dst = img + r * MMR_STRIDE + ELEMS * (tid % LANES);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const unsigned w = v[i][j];
                    if (BF16) { // two bf16 per word, the lower feature in the low half: widened exactly (bits << 16)
                        dst[2 * j] = __uint_as_float(w << 16);
                        dst[2 * j + 1] = __uint_as_float(w & 0xffff0000u);
                    } else {
                        dst[j] = __uint_as_float(w);
                    }
                }
            }
        }
    }
};

// One step of the wave's maximum inside a row of 16 lanes: every lane meets the value a DPP pattern brings it (quad_perm /
// row_ror: data-path moves, no LDS crossbar).  All 64 lanes are active.
template <int CTRL>
__device__ __forceinline__ float mmr_max_dpp(float x)
{
    return fmaxf(x, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), CTRL, 0xf, 0xf, false)));
}

// The wave's maximum, the same in every lane: quads (xor 1, xor 2), the row's four quads (rotate by 4, by 8), then the four
// rows' maxima through scalar registers.
__device__ __forceinline__ float mmr_wave_max(float x)
{
    x = mmr_max_dpp<0xB1>(x);  // quad_perm:[1,0,3,2]
    x = mmr_max_dpp<0x4E>(x);  // quad_perm:[2,3,0,1]
    x = mmr_max_dpp<0x124>(x); // row_ror:4
    x = mmr_max_dpp<0x128>(x); // row_ror:8
    float r = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), 0));
#pragma unroll
    for (int i = 1; i < 4; ++i)
        r = fmaxf(r, __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), 16 * i)));
    return r;
}

// grid: one workgroup per query
template <int CMAX, int MODE>
__global__ __launch_bounds__(MMR_THREADS) void mmr_kernel(const float *__restrict__ in_val, const int64_t *__restrict__ in_idx,
                                                          int C, const void *__restrict__ D, int64_t N, int d,
                                                          int64_t idx_offset, float lambda, float mu, int k,
                                                          float *__restrict__ out_val, int64_t *__restrict__ out_idx,
                                                          int32_t *__restrict__ out_pos)
{
    constexpr bool BF16 = MODE == MMR_BF16;
    typedef MmrPieces<CMAX, BF16> Pieces;
    constexpr int GS = CMAX + 1;                          // Gram stride: the mirrored store walks a column without conflicts
    constexpr int TMAX = CMAX / 32;
    constexpr int SLOTS = (TMAX * (TMAX + 1) / 2 + MMR_WAVES - 1) / MMR_WAVES; // upper-triangle tiles per wave: 3 (128) or 1 (64)
    constexpr int PER = CMAX / 64;                        // candidates per lane of the greedy wave
    static_assert(CMAX * GS >= CMAX * MMR_STRIDE, "the Gram takes the image's place");
    __shared__ float smem[CMAX * GS];                     // the image [CMAX][33], then G [CMAX][GS]
    __shared__ float s_rel[CMAX];
    __shared__ int64_t s_id[CMAX];
    __shared__ size_t s_off[CMAX];                        // element offset of the candidate's row, MMR_NO_ROW when invalid

    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const size_t b = blockIdx.x;

    if (tid < CMAX) {
        float rel = -INFINITY;
        int64_t g = -1;
        size_t off = MMR_NO_ROW;
        if (tid < C) {
            rel = in_val[b * C + tid];
            g = in_idx[b * C + tid];
            bool valid = g >= 0 && (__float_as_uint(rel) & 0x7f800000u) != 0x7f800000u;
            if (MODE == MMR_ROWS) {
                off = (b * C + tid) * (size_t)d;
            } else {
                // (unsigned difference: exact for every g >= max(idx_offset, 0), whatever the sign of idx_offset)
                const unsigned long long n = (unsigned long long)g - (unsigned long long)idx_offset;
                valid = valid && g >= idx_offset && n < (unsigned long long)N;
                off = (size_t)n * d;
            }
            if (!valid)
                off = MMR_NO_ROW;
        }
        s_rel[tid] = rel;
        s_id[tid] = g;
        s_off[tid] = off;
    }
    __syncthreads();

    // ---- gather + Gram
    const int nt32 = (C + 31) / 32;                       // tile rows in use
    const int n_tiles = nt32 * (nt32 + 1) / 2;
    int ti[SLOTS], tj[SLOTS];
    f32x16 acc[SLOTS];
#pragma unroll
    for (int s = 0; s < SLOTS; ++s) {
        // upper-triangle tile number p = wv + 4 s -> (ti <= tj), rows of tile-row ti first
        int p = wv + MMR_WAVES * s, i = 0;
        if (p < n_tiles) {
            while (p >= nt32 - i) {
                p -= nt32 - i;
                ++i;
            }
            ti[s] = i;
            tj[s] = i + p;
        } else {
            ti[s] = tj[s] = -1;
        }
#pragma unroll
        for (int r = 0; r < 16; ++r)
            acc[s][r] = 0.0f;
    }

    size_t row_off[Pieces::PASSES];
#pragma unroll
    for (int i = 0; i < Pieces::PASSES; ++i) {
        const int r = Pieces::ROWS * i + tid / Pieces::LANES;
        row_off[i] = r < CMAX ? s_off[r] : MMR_NO_ROW;
    }
    Pieces cur, nxt;
    cur.load(D, row_off, 0, d, tid);
    for (int x0 = 0; x0 < d; x0 += MMR_FEAT) {
        if (x0)
            __syncthreads();                              // the previous block has been multiplied
        cur.store(smem, tid);
        nxt.load(D, row_off, x0 + MMR_FEAT, d, tid);      // (behind the last block: beyond d, zeros, no load)
        __syncthreads();
        const int ne = min(MMR_FEAT, d - x0) / 2;         // d is a multiple of 4: whole pairs of features
#pragma unroll
        for (int s = 0; s < SLOTS; ++s) {
            if (ti[s] >= 0) { // wave-uniform
                // A[i = lane & 31][k = lane >> 5], B[k = lane >> 5][j = lane & 31]: features 2e, 2e + 1 in that order
                const float *ap = smem + (32 * ti[s] + (lane & 31)) * MMR_STRIDE + (lane >> 5);
                const float *bp = smem + (32 * tj[s] + (lane & 31)) * MMR_STRIDE + (lane >> 5);
                for (int e = 0; e < ne; ++e)
                    acc[s] = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[2 * e], bp[2 * e], acc[s], 0, 0, 0);
            }
        }
        cur = nxt;
    }
    __syncthreads();                                      // the image is dead: G takes its place
#pragma unroll
    for (int s = 0; s < SLOTS; ++s) {
        if (ti[s] >= 0) {
            const int col = 32 * tj[s] + (lane & 31);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = 32 * ti[s] + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                smem[row * GS + col] = acc[s][r];
                if (ti[s] != tj[s])
                    smem[col * GS + row] = acc[s][r];
            }
        }
    }
    __syncthreads();
    if (wv != 0)
        return;

    // ---- greedy selection, wave 0
    float a[PER], pen[PER];
    bool avail[PER];
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        const int c = lane + 64 * j;
        avail[j] = s_off[c] != MMR_NO_ROW;
        a[j] = lambda * s_rel[c];
        pen[j] = -INFINITY;
    }
    const size_t o = b * (size_t)k;
    int t = 0;
    for (; t < k; ++t) {
        // the largest m of the candidates left, then the lowest position that has it: positions < 64 first, by lane
        float m[PER], best = -INFINITY;
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            const float scaled = mu * pen[j];                // rounded on its own (no contraction in this file)
            m[j] = t == 0 ? a[j] : a[j] - scaled;
            if (avail[j])
                best = fmaxf(best, m[j]);
        }
        best = mmr_wave_max(best);
        int bp = INT_MAX;
#pragma unroll
        for (int j = PER - 1; j >= 0; --j) {
            const unsigned long long hit = __ballot(avail[j] && m[j] == best);
            if (hit)
                bp = 64 * j + __ffsll(hit) - 1;
        }
        if (bp == INT_MAX) // wave-uniform: no valid candidate is left
            break;
        if (lane == 0) {
            out_val[o + t] = s_rel[bp];
            out_idx[o + t] = s_id[bp];
            if (out_pos)
                out_pos[o + t] = bp;
        }
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            const int c = lane + 64 * j;
            pen[j] = fmaxf(pen[j], smem[bp * GS + c]);
            if (c == bp)
                avail[j] = false;
        }
    }
    for (int i = t + lane; i < k; i += 64) {
        out_val[o + i] = -INFINITY;
        out_idx[o + i] = -1;
        if (out_pos)
            out_pos[o + i] = -1;
    }
}

bool mmr_overlap(const void *a, size_t na, const void *b, size_t nb)
{
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return a && b && na && nb && x < y + nb && y < x + na;
}

template <int MODE>
void mmr_launch(int B, int C, const float *in_val, const int64_t *in_idx, const void *D, int64_t N, int d, int64_t idx_offset,
                float lambda, float mu, int k, float *out_val, int64_t *out_idx, int32_t *out_pos, hipStream_t st)
{
    if (C <= 64)
        hipLaunchKernelGGL((mmr_kernel<64, MODE>), dim3((unsigned)B), dim3(MMR_THREADS), 0, st, in_val, in_idx, C, D, N, d,
                           idx_offset, lambda, mu, k, out_val, out_idx, out_pos);
    else
        hipLaunchKernelGGL((mmr_kernel<128, MODE>), dim3((unsigned)B), dim3(MMR_THREADS), 0, st, in_val, in_idx, C, D, N, d,
                           idx_offset, lambda, mu, k, out_val, out_idx, out_pos);
}

// rows form: D = the gathered rows [B][C][d], N and idx_offset unused
int mmr_select(const char *who, int mode, const float *in_val, const int64_t *in_idx, int B, int C, const void *D, int64_t N, int d,
               int64_t idx_offset, float lambda, int k, float *out_val, int64_t *out_idx, int32_t *out_pos, tt_stream_t stream)
{
    const bool bf16 = mode == MMR_BF16, rows = mode == MMR_ROWS;
    if (B < 0 || C < 0 || N < 0)
        return tt_fail(TT_ERR_BAD_SHAPE, "%s: B=%d C=%d N=%lld", who, B, C, (long long)N);
    if (C > MMR_CMAX)
        return tt_fail(TT_ERR_UNSUPPORTED, "%s: C=%d (need 0 <= C <= %d)", who, C, MMR_CMAX);
    if (k < 1 || k > MMR_KMAX)
        return tt_fail(TT_ERR_UNSUPPORTED, "%s: k=%d (need 1 <= k <= %d)", who, k, MMR_KMAX);
    if (d <= 0 || d > 512 || d % (bf16 ? 8 : 4))
        return tt_fail(TT_ERR_UNSUPPORTED, "%s: d=%d (need a multiple of %d, at most 512)", who, d, bf16 ? 8 : 4);
    if (!(lambda >= 0.0f && lambda <= 1.0f))
        return tt_fail(TT_ERR_BAD_SHAPE, "%s: lambda=%g (need 0 <= lambda <= 1)", who, (double)lambda);
    if (B == 0)
        return TT_OK;
    const bool need_rows = C > 0 && (rows || N > 0);
    if (!out_val || !out_idx || (C > 0 && (!in_val || !in_idx)) || (need_rows && !D))
        return tt_fail(TT_ERR_BAD_SHAPE, "%s: null pointer", who);
    if (((uintptr_t)D & 15) || (((uintptr_t)in_val | (uintptr_t)out_val | (uintptr_t)out_pos) & 3) ||
        (((uintptr_t)in_idx | (uintptr_t)out_idx) & 7))
        return tt_fail(TT_ERR_BAD_SHAPE, "%s: rows must be 16-byte aligned, indices 8-byte, values and positions 4-byte", who);
    const size_t n_in = (size_t)B * C, n_out = (size_t)B * k;
    const struct {
        const void *p;
        size_t bytes;
    } in[3] = {{in_val, n_in * 4}, {in_idx, n_in * 8}, {D, rows ? n_in * d * 4 : (size_t)N * d * (bf16 ? 2 : 4)}},
      out[3] = {{out_val, n_out * 4}, {out_idx, n_out * 8}, {out_pos, n_out * 4}};
    for (int i = 0; i < 3; ++i) {
        for (const auto &r : in)
            if (mmr_overlap(r.p, r.bytes, out[i].p, out[i].bytes))
                return tt_fail(TT_ERR_BAD_SHAPE, "%s: out must not overlap in", who);
        for (int j = i + 1; j < 3; ++j)
            if (mmr_overlap(out[i].p, out[i].bytes, out[j].p, out[j].bytes))
                return tt_fail(TT_ERR_BAD_SHAPE, "%s: the outputs overlap", who);
    }
    const float mu = 1.0f - lambda;
    const hipStream_t st = (hipStream_t)stream;
    if (rows)
        mmr_launch<MMR_ROWS>(B, C, in_val, in_idx, D, N, d, idx_offset, lambda, mu, k, out_val, out_idx, out_pos, st);
    else if (bf16)
        mmr_launch<MMR_BF16>(B, C, in_val, in_idx, D, N, d, idx_offset, lambda, mu, k, out_val, out_idx, out_pos, st);
    else
        mmr_launch<MMR_F32>(B, C, in_val, in_idx, D, N, d, idx_offset, lambda, mu, k, out_val, out_idx, out_pos, st);
    TT_LAUNCH_CHECK();
    return TT_OK;
}

} // namespace

TT_EXPORT int tt_mmr_select_f32(const float *in_val, const int64_t *in_idx, int B, int C, const float *D, int64_t N, int d,
                                int64_t idx_offset, float lambda, int k, float *out_val, int64_t *out_idx, int32_t *out_pos,
                                tt_stream_t stream)
{
    return mmr_select("tt_mmr_select_f32", MMR_F32, in_val, in_idx, B, C, D, N, d, idx_offset, lambda, k, out_val, out_idx, out_pos,
                      stream);
}

TT_EXPORT int tt_mmr_select_bf16(const float *in_val, const int64_t *in_idx, int B, int C, const void *D_bf16, int64_t N, int d,
                                 int64_t idx_offset, float lambda, int k, float *out_val, int64_t *out_idx, int32_t *out_pos,
                                 tt_stream_t stream)
{
    return mmr_select("tt_mmr_select_bf16", MMR_BF16, in_val, in_idx, B, C, D_bf16, N, d, idx_offset, lambda, k, out_val, out_idx,
                      out_pos, stream);
}

TT_EXPORT int tt_mmr_select_rows_f32(const float *in_val, const int64_t *in_idx, int B, int C, const float *rows, int d, float lambda,
                                     int k, float *out_val, int64_t *out_idx, int32_t *out_pos, tt_stream_t stream)
{
    return mmr_select("tt_mmr_select_rows_f32", MMR_ROWS, in_val, in_idx, B, C, rows, 0, d, 0, lambda, k, out_val, out_idx, out_pos,
                      stream);
}
