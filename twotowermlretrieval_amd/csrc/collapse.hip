// Collapsed search (DESIGN.md "Collapsed search"): the first k entries of a sorted row that are ungrouped (group id < 0) or
// among the first max_per_group entries of the row with their group id.  One 256-thread workgroup per row, the row's group
// ids in LDS, every entry counts the earlier entries with its id, then the order-preserving ballot compaction of exclude.hip.
#include "tt_common.h"

namespace {

constexpr int COL_THREADS = 256;
constexpr int COL_WAVES = COL_THREADS / TT_WAVE;
constexpr int COL_MMAX = TT_TOPK_LARGE_KMAX; // entries of a row: 8 KB of group ids in LDS

// TABLE: src = groups [N], the group of entry e is groups[in_idx[e] - idx_offset] (ungrouped outside the table);
// otherwise src = in_gid [B][M], one id per entry.
template <bool TABLE>
__global__ __launch_bounds__(COL_THREADS) void collapse_kernel(const float *__restrict__ in_val, const int64_t *__restrict__ in_idx,
                                                               int M, const int64_t *__restrict__ src, int64_t N,
                                                               int64_t idx_offset, int max_per_group, int k,
                                                               float *__restrict__ out_val, int64_t *__restrict__ out_idx,
                                                               int64_t *__restrict__ out_gid, int *__restrict__ out_info)
{
    __shared__ __attribute__((aligned(16))) int64_t gid[COL_MMAX];
    __shared__ int wave_kept[2][COL_WAVES]; // per chunk parity: one barrier per chunk
    const int tid = threadIdx.x, lane = tid & (TT_WAVE - 1), wave = tid / TT_WAVE;
    const int64_t row = blockIdx.x;
    in_val += row * M;
    in_idx += row * M;
    out_val += row * k;
    out_idx += row * k;
    out_gid += row * k;

    // the row's group ids; padding of the input row (idx < 0) is ungrouped, so it counts against nobody
    for (int e = tid; e < M; e += COL_THREADS) {
        const int64_t id = in_idx[e];
        int64_t g = -1;
        if (id >= 0) {
            if (TABLE) {
                const uint64_t n = (uint64_t)id - (uint64_t)idx_offset; // (wraps to a huge value below the table)
                if (n < (uint64_t)N)
                    g = src[n];
            } else {
                g = src[row * M + e];
            }
        }
        gid[e] = g;
    }
    __syncthreads();

    int base = 0; // entries kept so far (the same in every thread)
    for (int c = 0, it = 0; c < M && base < k; c += COL_THREADS, ++it) {
        const int m = c + tid;
        int64_t id = -1, g = -1;
        if (m < M) {
            id = in_idx[m];
            g = gid[m];
        }
        // earlier entries with this id: every lane reads the same two ids per step (a broadcast ds_read_b128); the pair that
        // straddles the end of the row reads an unwritten word at most, which j < m < M keeps out of the count
        int earlier = 0;
        const int end = min(c + COL_THREADS, M);
        for (int j = 0; j < end; j += 2) {
            const longlong2 p = *reinterpret_cast<const longlong2 *>(&gid[j]);
            earlier += (j < m && p.x == g) + (j + 1 < m && p.y == g);
        }
        const bool keep = id >= 0 && (g < 0 || earlier < max_per_group);
        const unsigned long long b = __ballot(keep);
        if (lane == 0)
            wave_kept[it & 1][wave] = __popcll(b);
        __syncthreads();
        int pos = base + __popcll(b & ((1ull << lane) - 1ull));
        int total = 0;
#pragma unroll
        for (int w = 0; w < COL_WAVES; ++w) {
            const int n = wave_kept[it & 1][w];
            pos += w < wave ? n : 0;
            total += n;
        }
        if (keep && pos < k) {
            out_val[pos] = in_val[m];
            out_idx[pos] = id;
            out_gid[pos] = g;
        }
        base += total;
    }
    const int kept = min(base, k);
    for (int p = kept + tid; p < k; p += COL_THREADS) {
        out_val[p] = -INFINITY;
        out_idx[p] = -1;
        out_gid[p] = -1;
    }
    if (tid == 0) {
        out_info[2 * row] = kept;
        out_info[2 * row + 1] = kept == k || in_idx[M - 1] < 0; // every eligible row was seen: nothing lies beyond padding
    }
}

bool col_overlap(const void *a, size_t na, const void *b, size_t nb)
{
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + nb && y < x + na;
}

// The checks the two entries share (src: the group table [N], which may be null when N = 0, or the rows' group ids [B][M]).
// *launch = false when there is nothing to do (B = 0).
int col_check(const char *fn, const float *in_val, const int64_t *in_idx, const int64_t *src, bool gids_form, int64_t N, int B, int M,
              int max_per_group, int k, const float *out_val, const int64_t *out_idx, const int64_t *out_gid, const int32_t *out_info,
              bool *launch)
{
    *launch = false;
    if (B < 0 || M < 0 || N < 0 || k < 1 || k > M || max_per_group < 1)
        return tt_fail(TT_ERR_BAD_SHAPE, "%s: B=%d M=%d N=%lld k=%d max_per_group=%d (need 1 <= k <= M, max_per_group >= 1)", fn, B, M,
                       (long long)N, k, max_per_group);
    if (M > COL_MMAX)
        return tt_fail(TT_ERR_UNSUPPORTED, "%s: M=%d > %d", fn, M, COL_MMAX);
    if (B == 0)
        return TT_OK;
    if (!in_val || !in_idx || !out_val || !out_idx || !out_gid || !out_info || (!src && (gids_form || N > 0)))
        return tt_fail(TT_ERR_BAD_SHAPE, "%s: null pointer", fn);
    if ((((uintptr_t)in_val | (uintptr_t)out_val | (uintptr_t)out_info) & 3) ||
        (((uintptr_t)in_idx | (uintptr_t)src | (uintptr_t)out_idx | (uintptr_t)out_gid) & 7))
        return tt_fail(TT_ERR_BAD_SHAPE, "%s: values and info must be 4-byte aligned, indices and group ids 8-byte aligned", fn);
    const size_t n_in = (size_t)B * M, n_out = (size_t)B * k, n_src = gids_form ? n_in : (size_t)N;
    if (col_overlap(in_val, n_in * 4, out_val, n_out * 4) || col_overlap(in_idx, n_in * 8, out_idx, n_out * 8) ||
        col_overlap(in_idx, n_in * 8, out_gid, n_out * 8) || col_overlap(src, n_src * 8, out_idx, n_out * 8) ||
        col_overlap(src, n_src * 8, out_gid, n_out * 8))
        return tt_fail(TT_ERR_BAD_SHAPE, "%s: out must not alias in", fn);
    *launch = true;
    return TT_OK;
}

} // namespace

TT_EXPORT int tt_topk_collapse_table(const float *in_val, const int64_t *in_idx, int B, int M, const int64_t *groups, int64_t N,
                                     int64_t idx_offset, int max_per_group, int k, float *out_val, int64_t *out_idx,
                                     int64_t *out_gid, int32_t *out_info, tt_stream_t stream)
{
    bool launch;
    TT_RC_CHECK(col_check("tt_topk_collapse_table", in_val, in_idx, groups, false, N, B, M, max_per_group, k, out_val, out_idx, out_gid,
                          out_info, &launch));
    if (!launch)
        return TT_OK;
    hipLaunchKernelGGL(collapse_kernel<true>, dim3(B), dim3(COL_THREADS), 0, (hipStream_t)stream, in_val, in_idx, M, groups, N,
                       idx_offset, max_per_group, k, out_val, out_idx, out_gid, (int *)out_info);
    TT_LAUNCH_CHECK();
    return TT_OK;
}

TT_EXPORT int tt_topk_collapse_gids(const float *in_val, const int64_t *in_idx, const int64_t *in_gid, int B, int M,
                                    int max_per_group, int k, float *out_val, int64_t *out_idx, int64_t *out_gid,
                                    int32_t *out_info, tt_stream_t stream)
{
    bool launch;
    TT_RC_CHECK(col_check("tt_topk_collapse_gids", in_val, in_idx, in_gid, true, 0, B, M, max_per_group, k, out_val, out_idx, out_gid,
                          out_info, &launch));
    if (!launch)
        return TT_OK;
    hipLaunchKernelGGL(collapse_kernel<false>, dim3(B), dim3(COL_THREADS), 0, (hipStream_t)stream, in_val, in_idx, M, in_gid,
                       (int64_t)0, (int64_t)0, max_per_group, k, out_val, out_idx, out_gid, (int *)out_info);
    TT_LAUNCH_CHECK();
    return TT_OK;
}
