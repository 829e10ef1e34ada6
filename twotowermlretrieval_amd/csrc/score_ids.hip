// Candidate search (DESIGN.md "Candidate search"): the exact scores of a per-query list of document ids.  Where every other
// search streams all N rows, this one reads B * C of them: the rows are gathered by id.
// The score is the project's: the fp32 fmaf chain over the feature index ascending, acc0 = 0 (score_all_kernel's, and with it
// bit for bit what the top-k kernels return for the document), so one lane owns one candidate -- the chain is sequential by
// definition.  A wave takes 64 candidates and stages their rows 32 features at a time through a 33-float-stride LDS image
// like score_all_kernel; the row address comes from the lane's id instead of n0 + lane.  The 128-byte pieces of the next 32
// features are loaded into registers before the chain over the current ones runs, so a wave always has one block of pieces
// (8 x 1 KiB fp32, 4 x 1 KiB bf16) in flight while it computes.
#include <limits.h>
#include <math.h>

#include "tt_common.h"

namespace {

constexpr int SID_THREADS = 256;                    // one workgroup per (query, 256 candidates)
constexpr int SID_WAVES = SID_THREADS / TT_WAVE;
constexpr int SID_FEAT = 32;                        // features per staged block
constexpr int SID_STRIDE = SID_FEAT + 1;            // image stride in floats: lane l reads bank (l + x) % 32

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// The pieces of one 32-feature block of a wave's 64 rows, in registers.
// fp32: piece i = rows 8 i + lane / 8, 16 bytes (4 features) at chunk lane % 8 -- whole 128-byte segments per row.
// bf16: piece i = rows 16 i + lane / 4, 16 bytes (8 features) at chunk lane % 4 -- whole 64-byte segments per row.
template <bool BF16>
struct SidPieces {
    static constexpr int N_PIECES = BF16 ? 4 : 8;
    static constexpr int ROWS = 64 / N_PIECES;      // rows per piece
    static constexpr int LANES = 64 / ROWS;         // lanes per row
    static constexpr int ELEMS = SID_FEAT / LANES;  // features per lane: 4 (fp32) or 8 (bf16), 16 bytes either way
    u32x4 v[N_PIECES];

    // row_off[i]: element offset of this lane's row of piece i; features at or beyond d read as zero (never loaded)
    __device__ __forceinline__ void load(const void *D, const size_t *row_off, int x0, int d, int lane)
    {
        const int x = x0 + ELEMS * (lane % LANES);
        if (x < d) { // one test for all pieces: the loads go out back to back
#pragma unroll
            for (int i = 0; i < N_PIECES; ++i) {
                if (BF16)
                    v[i] = *(const u32x4 *)((const uint16_t *)D + row_off[i] + x);
                else
                    v[i] = *(const u32x4 *)((const float *)D + row_off[i] + x);
            }
        } else {
#pragma unroll
            for (int i = 0; i < N_PIECES; ++i)
                v[i] = u32x4{0u, 0u, 0u, 0u};
        }
    }

    __device__ __forceinline__ void store(float *img, int lane) const
    {
#pragma unroll
        for (int i = 0; i < N_PIECES; ++i) {
            float *dst = img + (ROWS * i + lane / LANES) * SID_STRIDE + ELEMS * (lane % LANES);
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
};

// grid: B * blocks_per_query workgroups, flattened (no B in grid.y: no 65 535 limit)
template <bool BF16>
__global__ __launch_bounds__(SID_THREADS) void score_ids_kernel(const float *__restrict__ Q, const void *__restrict__ D, int64_t N,
                                                                int d, const unsigned *__restrict__ keep,
                                                                const int64_t *__restrict__ ids, int C, int64_t idx_offset,
                                                                int blocks_per_query, float *__restrict__ out_val,
                                                                int64_t *__restrict__ out_idx)
{
    typedef SidPieces<BF16> Pieces;
    __shared__ float qs[512];
    __shared__ float stage[SID_WAVES][64 * SID_STRIDE];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int b = blockIdx.x / blocks_per_query;
    const int c0 = (blockIdx.x - b * blocks_per_query) * SID_THREADS + wv * 64;
    for (int x = threadIdx.x; x < d; x += SID_THREADS)
        qs[x] = Q[(size_t)b * d + x];
    __syncthreads();
    if (c0 >= C)
        return; // wave-uniform; no block barrier below

    // this lane's candidate: global id g -> row n of D, or nothing (padding, another shard's id, a cleared keep bit)
    const int c = c0 + lane;
    const size_t at = (size_t)b * C + c;
    int64_t g = -1;
    if (c < C)
        g = ids[at];
    // (unsigned difference: exact for every g >= max(idx_offset, 0), whatever the sign of idx_offset)
    const unsigned long long n = (unsigned long long)g - (unsigned long long)idx_offset;
    bool valid = g >= 0 && g >= idx_offset && n < (unsigned long long)N;
    if (valid && keep)
        valid = (keep[n >> 5] >> (n & 31)) & 1u;

    const unsigned long long have = __ballot(valid);
    float acc = 0.0f;
    if (have) { // wave-uniform: a wave of padding (and every wave when N = 0) reads no row
        // lanes with nothing to score follow the wave's first valid row, and are overwritten at the end
        const unsigned long long first = __shfl(n, __ffsll(have) - 1);
        const size_t mine_off = (size_t)(valid ? n : first) * d;
        size_t row_off[Pieces::N_PIECES];
#pragma unroll
        for (int i = 0; i < Pieces::N_PIECES; ++i)
            row_off[i] = __shfl(mine_off, Pieces::ROWS * i + lane / Pieces::LANES);

        float *img = stage[wv];
        const float *mine = img + lane * SID_STRIDE;
        Pieces cur, nxt;
        cur.load(D, row_off, 0, d, lane);
        for (int x0 = 0; x0 < d; x0 += SID_FEAT) {
            cur.store(img, lane);
            nxt.load(D, row_off, x0 + SID_FEAT, d, lane); // (behind the last block: beyond d, zeros, no load)
            __builtin_amdgcn_wave_barrier();
            const int xe = min(SID_FEAT, d - x0);
            for (int x = 0; x < xe; ++x)
                acc = fmaf(qs[x0 + x], mine[x], acc);
            __builtin_amdgcn_wave_barrier();
            cur = nxt;
        }
    }
    if (c < C) {
        out_val[at] = valid ? acc : -INFINITY;
        if (out_idx)
            out_idx[at] = valid ? g : -1;
    }
}

bool sid_overlap(const void *a, size_t na, const void *b, size_t nb)
{
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return a && b && na && nb && x < y + nb && y < x + na;
}

int score_ids(const char *who, bool bf16, const float *Q, int B, int d, const void *D, int64_t N, const uint32_t *keep,
              const int64_t *ids, int C, int64_t idx_offset, float *out_val, int64_t *out_idx, tt_stream_t stream)
{
    if (B < 0 || C < 0 || N < 0)
        return tt_fail(TT_ERR_BAD_SHAPE, "%s: B=%d C=%d N=%lld", who, B, C, (long long)N);
    if (d <= 0 || d > 512 || d % (bf16 ? 8 : 4))
        return tt_fail(TT_ERR_UNSUPPORTED, "%s: d=%d (need a multiple of %d, at most 512)", who, d, bf16 ? 8 : 4);
    if (B == 0 || C == 0)
        return TT_OK;
    if (!Q || !ids || !out_val || (N > 0 && !D))
        return tt_fail(TT_ERR_BAD_SHAPE, "%s: null pointer", who);
    if ((((uintptr_t)Q | (uintptr_t)D) & 15) || (((uintptr_t)out_val | (uintptr_t)keep) & 3) ||
        (((uintptr_t)ids | (uintptr_t)out_idx) & 7))
        return tt_fail(TT_ERR_BAD_SHAPE, "%s: Q and D must be 16-byte aligned, ids and indices 8-byte, values and keep 4-byte", who);
    const size_t n_out = (size_t)B * C;
    const struct {
        const void *p;
        size_t bytes;
    } in[4] = {{Q, (size_t)B * d * 4}, {D, (size_t)N * d * (bf16 ? 2 : 4)}, {keep, (size_t)((N + 31) / 32) * 4}, {ids, n_out * 8}};
    for (const auto &r : in)
        if (sid_overlap(r.p, r.bytes, out_val, n_out * 4) || sid_overlap(r.p, r.bytes, out_idx, n_out * 8))
            return tt_fail(TT_ERR_BAD_SHAPE, "%s: out must not overlap in", who);
    if (sid_overlap(out_val, n_out * 4, out_idx, n_out * 8))
        return tt_fail(TT_ERR_BAD_SHAPE, "%s: out_val and out_idx overlap", who);
    const int bpq = (C + SID_THREADS - 1) / SID_THREADS;
    if ((int64_t)B * bpq > INT_MAX)
        return tt_fail(TT_ERR_UNSUPPORTED, "%s: B=%d x ceil(C/%d)=%d workgroups exceed one launch", who, B, SID_THREADS, bpq);
    const dim3 grid((unsigned)((int64_t)B * bpq));
    if (bf16)
        hipLaunchKernelGGL(score_ids_kernel<true>, grid, dim3(SID_THREADS), 0, (hipStream_t)stream, Q, D, N, d, keep, ids, C,
                           idx_offset, bpq, out_val, out_idx);
    else
        hipLaunchKernelGGL(score_ids_kernel<false>, grid, dim3(SID_THREADS), 0, (hipStream_t)stream, Q, D, N, d, keep, ids, C,
                           idx_offset, bpq, out_val, out_idx);
    TT_LAUNCH_CHECK();
    return TT_OK;
}

} // namespace

TT_EXPORT int tt_score_ids_f32(const float *Q, int B, int d, const float *D, int64_t N, const uint32_t *keep, const int64_t *ids,
                               int C, int64_t idx_offset, float *out_val, int64_t *out_idx, tt_stream_t stream)
{
    return score_ids("tt_score_ids_f32", false, Q, B, d, D, N, keep, ids, C, idx_offset, out_val, out_idx, stream);
}

TT_EXPORT int tt_score_ids_bf16(const float *Q, int B, int d, const void *D_bf16, int64_t N, const uint32_t *keep,
                                const int64_t *ids, int C, int64_t idx_offset, float *out_val, int64_t *out_idx,
                                tt_stream_t stream)
{
    return score_ids("tt_score_ids_bf16", true, Q, B, d, D_bf16, N, keep, ids, C, idx_offset, out_val, out_idx, stream);
}
