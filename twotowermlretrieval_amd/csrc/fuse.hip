// Fused lists (DESIGN.md "Fused lists"): the best k ids of the union of L ranked lists per row, by a sum of per-list terms --
// a table entry per column (reciprocal rank fusion, Borda, any rank weighting) or weight * score -- added in list order, every
// step rounded to fp32.  One 256-thread workgroup per row, the row's ids and terms in LDS; every entry finds its id's first
// occurrence in every list (broadcast 128-bit reads, like collapse_kernel's count; over 32-bit words when the row's ids fit
// them), the first live entry of an id sums its terms, then every such representative counts the representatives ranked
// before it -- one 64-bit key per slot, (score, id order) -- and stores itself there.
#include "tt_common.h"

namespace {

constexpr int FUSE_THREADS = 256;
constexpr int FUSE_LMAX = 8;
constexpr int FUSE_EMAX = TT_TOPK_LARGE_KMAX;   // entries of a row, L * M
constexpr int FUSE_SLOTS = FUSE_EMAX + FUSE_LMAX; // a list of odd M is padded to an even pitch: one slot per list at most
constexpr int FUSE_SLOTS32 = FUSE_EMAX + 3 * FUSE_LMAX; // the 32-bit image: four ids per read, a pitch that is a multiple of four
constexpr int FUSE_ABSENT = 0x7fff;

template <typename T, int W> struct __attribute__((aligned(16))) FuseIds {
    T v[W]; // one 128-bit LDS read
};

// One list of a row for the NI entries of a thread: first = the first column that holds the entry's id (unchanged where none
// does), smaller += the slots with a smaller id.  Downwards, so that the last match written is the first of the list; every
// lane reads the same W ids per step (a broadcast ds_read_b128).
template <int NI, typename T, int W>
__device__ __forceinline__ void fuse_scan(const T *lst, int pitch, const T (&id)[NI], int (&first)[NI], int (&smaller)[NI])
{
#pragma unroll 4
    for (int j = pitch - W; j >= 0; j -= W) {
        const FuseIds<T, W> p = *reinterpret_cast<const FuseIds<T, W> *>(lst + j);
#pragma unroll
        for (int w = W - 1; w >= 0; --w) {
#pragma unroll
            for (int i = 0; i < NI; ++i) {
                first[i] = p.v[w] == id[i] ? j + w : first[i];
                smaller[i] += p.v[w] < id[i];
            }
        }
    }
}

// NI: entries per thread, ceil(L * M / 256).  SCORE: the term of entry (l, m) is fl32(weight[l] * in_val), else table[l][m].
template <int NI, bool SCORE>
__global__ __launch_bounds__(FUSE_THREADS) void fuse_kernel(const float *__restrict__ in_val, const int64_t *__restrict__ in_idx,
                                                            int L, int M, const float *__restrict__ table,
                                                            const float *__restrict__ missing, int k, float *__restrict__ out_val,
                                                            int64_t *__restrict__ out_idx, int *__restrict__ out_pos)
{
    // list l at [l * P, l * P + M), P = M rounded up to even: the ids (-1 = padding) while the entries look for their ids, then
    // the sort keys of the representatives (0 everywhere else)
    __shared__ __attribute__((aligned(16))) int64_t sid[FUSE_SLOTS];
    // the ids' low words, list l at [l * P4, l * P4 + M): the image the entries read when every id of the row is below 2^31
    __shared__ __attribute__((aligned(16))) int sid32[FUSE_SLOTS32];
    __shared__ float sterm[FUSE_SLOTS];
    __shared__ float smiss[FUSE_LMAX];
    const int tid = threadIdx.x;
    const int64_t row = blockIdx.x;
    const int E = L * M, P = (M + 1) & ~1, P4 = (M + 3) & ~3;
    in_idx += row * E;
    if (SCORE)
        in_val += row * E;
    out_val += row * k;
    out_idx += row * k;

    int64_t id[NI];
    int id32[NI], slot[NI], own_l[NI], own_m[NI];
    bool small = true;
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        const int e = tid + FUSE_THREADS * i;
        id[i] = -1;
        own_l[i] = own_m[i] = slot[i] = 0;
        if (e < E) {
            own_l[i] = e / M;
            own_m[i] = e - own_l[i] * M;
            slot[i] = own_l[i] * P + own_m[i];
            const int64_t x = in_idx[e];
            id[i] = x < 0 ? -1 : x;
            sid[slot[i]] = id[i];
            sid32[own_l[i] * P4 + own_m[i]] = (int)id[i];
            sterm[slot[i]] = SCORE ? __fmul_rn(table[own_l[i]], in_val[e]) : table[e];
        }
        id32[i] = (int)id[i];
        small &= id[i] < ((int64_t)1 << 31);
    }
    if (tid < L) {
        smiss[tid] = missing[tid];
        if (P != M) // the pad slots of the list: no id
            sid[tid * P + M] = -1;
        for (int m = M; m < P4; ++m)
            sid32[tid * P4 + m] = -1;
    }
    // every id of the row fits 31 bits (padding is -1 in either image): the entries compare words, four per read
    const bool narrow = __syncthreads_and(small);

    // per entry: the column of its id's first occurrence in every list (16 bits each, 0 = absent), the sum of the terms in list
    // order, whether the entry is that first occurrence in its own list (live), whether an earlier list holds the id, and how
    // many slots hold a smaller id (below: ids in 11 bits, in the same order)
    float acc[NI];
    uint64_t pos_lo[NI], pos_hi[NI];
    bool live[NI], earlier[NI];
    int smaller[NI];
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        acc[i] = 0.0f;
        pos_lo[i] = pos_hi[i] = 0;
        live[i] = earlier[i] = false;
        smaller[i] = 0;
    }
    bool work = false; // (padding finds nothing: a wave of padding skips the scan)
#pragma unroll
    for (int i = 0; i < NI; ++i)
        work |= id[i] >= 0;
    if (work) {
        for (int l = 0; l < L; ++l) {
            int first[NI];
#pragma unroll
            for (int i = 0; i < NI; ++i)
                first[i] = FUSE_ABSENT;
            if (narrow)
                fuse_scan<NI, int, 4>(sid32 + l * P4, P4, id32, first, smaller);
            else
                fuse_scan<NI, int64_t, 2>(sid + l * P, P, id, first, smaller);
            const float miss = smiss[l];
#pragma unroll
            for (int i = 0; i < NI; ++i) {
                const bool present = id[i] >= 0 && first[i] != FUSE_ABSENT;
                const float t = present ? sterm[l * P + first[i]] : miss;
                acc[i] = __fadd_rn(acc[i], t);
                earlier[i] |= present && l < own_l[i];
                live[i] |= present && l == own_l[i] && first[i] == own_m[i];
                const uint64_t w = (uint64_t)(present ? first[i] + 1 : 0) << (16 * (l & 3));
                pos_lo[i] |= l < 4 ? w : 0;
                pos_hi[i] |= l < 4 ? 0 : w;
            }
        }
    }
    // A representative's sort key: the fused score as an unsigned integer in the order of the floats (the sum is never -0: it
    // starts at +0), above the complement of `smaller` -- of two representatives the one with the smaller id has fewer slots
    // below it, its own among the other's.  Distinct, and above the 0 of every other slot, for finite scores.
    bool rep[NI];
    uint64_t key[NI];
    int reps = 0;
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        rep[i] = id[i] >= 0 && live[i] && !earlier[i];
        const uint32_t u = __float_as_uint(acc[i]);
        key[i] = rep[i] ? ((uint64_t)(u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u)) << 32) | (uint32_t)(0xffff - smaller[i]) : 0;
        reps += rep[i];
    }
    // (the first of these barriers is also the one behind the last read of an id)
    int n_rep = 0;
#pragma unroll
    for (int c = 1; c <= NI; ++c)
        n_rep += c * __syncthreads_count(reps == c);
    uint64_t *skey = reinterpret_cast<uint64_t *>(sid);
#pragma unroll
    for (int i = 0; i < NI; ++i)
        if (tid + FUSE_THREADS * i < E)
            skey[slot[i]] = key[i];
    if (tid < L && P != M)
        skey[tid * P + M] = 0;
    __syncthreads();

    // the rank of a representative = the representatives before it under (fused desc, id asc) = the larger keys; the keys are
    // distinct, so the ranks are a permutation of [0, n_rep).  A wave whose representatives all have k before them is done.
    work = false;
#pragma unroll
    for (int i = 0; i < NI; ++i)
        work |= rep[i];
    if (work) {
        int before[NI];
#pragma unroll
        for (int i = 0; i < NI; ++i)
            before[i] = 0;
        const int S = L * P; // even
        for (int j0 = 0; j0 < S; j0 += 64) {
            const int end = min(j0 + 64, S);
#pragma unroll 4
            for (int j = j0; j < end; j += 2) {
                const ulonglong2 p = *reinterpret_cast<const ulonglong2 *>(skey + j);
#pragma unroll
                for (int i = 0; i < NI; ++i)
                    before[i] += (p.x > key[i]) + (p.y > key[i]);
            }
            bool done = true;
#pragma unroll
            for (int i = 0; i < NI; ++i)
                done &= !rep[i] || before[i] >= k;
            if (__all(done))
                break;
        }
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            if (rep[i] && before[i] < k) {
                const int r = before[i];
                out_val[r] = acc[i];
                out_idx[r] = id[i];
                if (out_pos) {
                    int *op = out_pos + (row * k + r) * L;
                    for (int l = 0; l < L; ++l)
                        op[l] = (int)(((l < 4 ? pos_lo[i] : pos_hi[i]) >> (16 * (l & 3))) & 0xffff) - 1;
                }
            }
        }
    }
    for (int r = min(n_rep, k) + tid; r < k; r += FUSE_THREADS) {
        out_val[r] = -INFINITY;
        out_idx[r] = -1;
        if (out_pos)
            for (int l = 0; l < L; ++l)
                out_pos[(row * k + r) * L + l] = -1;
    }
}

bool fuse_overlap(const void *a, size_t na, const void *b, size_t nb)
{
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return a && b && x < y + nb && y < x + na;
}

// The checks the two entries share (in_val: null in the rank form; table: rank_weight [L][M] or weight [L]).
// *launch = false when there is nothing to do (B = 0).
int fuse_check(const char *fn, bool score, const float *in_val, const int64_t *in_idx, int B, int L, int M, const float *table,
               const float *missing, int k, const float *out_val, const int64_t *out_idx, const int32_t *out_pos, bool *launch)
{
    *launch = false;
    if (B < 0 || L < 1 || M < 1)
        return tt_fail(TT_ERR_BAD_SHAPE, "%s: B=%d L=%d M=%d (need B >= 0, L >= 1, M >= 1)", fn, B, L, M);
    if (L > FUSE_LMAX || (int64_t)L * M > FUSE_EMAX)
        return tt_fail(TT_ERR_UNSUPPORTED, "%s: L=%d M=%d (need L <= %d, L*M <= %d)", fn, L, M, FUSE_LMAX, FUSE_EMAX);
    if (k < 1 || k > L * M)
        return tt_fail(TT_ERR_BAD_SHAPE, "%s: k=%d (need 1 <= k <= L*M = %d)", fn, k, L * M);
    if (B == 0)
        return TT_OK;
    if ((score && !in_val) || !in_idx || !table || !missing || !out_val || !out_idx)
        return tt_fail(TT_ERR_BAD_SHAPE, "%s: null pointer", fn);
    if ((((uintptr_t)in_val | (uintptr_t)table | (uintptr_t)missing | (uintptr_t)out_val | (uintptr_t)out_pos) & 3) ||
        (((uintptr_t)in_idx | (uintptr_t)out_idx) & 7))
        return tt_fail(TT_ERR_BAD_SHAPE, "%s: values, tables and positions must be 4-byte aligned, indices 8-byte aligned", fn);
    const size_t n_in = (size_t)B * L * M, n_out = (size_t)B * k;
    const void *ins[4] = {score ? in_val : nullptr, in_idx, table, missing};
    const size_t in_bytes[4] = {n_in * 4, n_in * 8, (score ? (size_t)L : (size_t)L * M) * 4, (size_t)L * 4};
    const void *outs[3] = {out_val, out_idx, out_pos};
    const size_t out_bytes[3] = {n_out * 4, n_out * 8, n_out * L * 4};
    for (int o = 0; o < 3; ++o)
        for (int i = 0; i < 4; ++i)
            if (fuse_overlap(ins[i], in_bytes[i], outs[o], out_bytes[o]))
                return tt_fail(TT_ERR_BAD_SHAPE, "%s: out must not alias in", fn);
    *launch = true;
    return TT_OK;
}

template <bool SCORE>
void fuse_launch(const float *in_val, const int64_t *in_idx, int B, int L, int M, const float *table, const float *missing, int k,
                 float *out_val, int64_t *out_idx, int32_t *out_pos, hipStream_t stream)
{
    const dim3 grid(B), block(FUSE_THREADS);
    switch ((L * M + FUSE_THREADS - 1) / FUSE_THREADS) {
    case 1:
        hipLaunchKernelGGL((fuse_kernel<1, SCORE>), grid, block, 0, stream, in_val, in_idx, L, M, table, missing, k, out_val, out_idx,
                           (int *)out_pos);
        break;
    case 2:
        hipLaunchKernelGGL((fuse_kernel<2, SCORE>), grid, block, 0, stream, in_val, in_idx, L, M, table, missing, k, out_val, out_idx,
                           (int *)out_pos);
        break;
    case 3:
        hipLaunchKernelGGL((fuse_kernel<3, SCORE>), grid, block, 0, stream, in_val, in_idx, L, M, table, missing, k, out_val, out_idx,
                           (int *)out_pos);
        break;
    default:
        hipLaunchKernelGGL((fuse_kernel<4, SCORE>), grid, block, 0, stream, in_val, in_idx, L, M, table, missing, k, out_val, out_idx,
                           (int *)out_pos);
        break;
    }
}

} // namespace

TT_EXPORT int tt_topk_fuse_rank_f32(const int64_t *in_idx, int B, int L, int M, const float *rank_weight, const float *missing, int k,
                                    float *out_val, int64_t *out_idx, int32_t *out_pos, tt_stream_t stream)
{
    bool launch;
    TT_RC_CHECK(fuse_check("tt_topk_fuse_rank_f32", false, nullptr, in_idx, B, L, M, rank_weight, missing, k, out_val, out_idx, out_pos,
                           &launch));
    if (!launch)
        return TT_OK;
    fuse_launch<false>(nullptr, in_idx, B, L, M, rank_weight, missing, k, out_val, out_idx, out_pos, (hipStream_t)stream);
    TT_LAUNCH_CHECK();
    return TT_OK;
}

TT_EXPORT int tt_topk_fuse_score_f32(const float *in_val, const int64_t *in_idx, int B, int L, int M, const float *weight,
                                     const float *missing, int k, float *out_val, int64_t *out_idx, int32_t *out_pos,
                                     tt_stream_t stream)
{
    bool launch;
    TT_RC_CHECK(fuse_check("tt_topk_fuse_score_f32", true, in_val, in_idx, B, L, M, weight, missing, k, out_val, out_idx, out_pos,
                           &launch));
    if (!launch)
        return TT_OK;
    fuse_launch<true>(in_val, in_idx, B, L, M, weight, missing, k, out_val, out_idx, out_pos, (hipStream_t)stream);
    TT_LAUNCH_CHECK();
    return TT_OK;
}
