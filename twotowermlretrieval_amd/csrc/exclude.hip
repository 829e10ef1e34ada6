// Per-query exclusion (DESIGN.md "Per-query exclusion"): the first k entries of a sorted top-(k + E) row whose index is not in
// that query's list of E ids.  One 256-thread workgroup per row, the list in LDS, order-preserving compaction with wave ballots.
#include <limits.h>

#include "tt_common.h"

namespace {

constexpr int EXC_THREADS = 256;
constexpr int EXC_WAVES = EXC_THREADS / TT_WAVE;
constexpr int EXC_EMAX = TT_TOPK_LARGE_KMAX;   // LDS entries (8 KB): E <= EXC_EMAX - 1 real ids, the rest INT64_MAX
constexpr int EXC_DIRECT_MAX = 32;             // up to here every candidate is compared with the whole list (broadcast reads)

// Whether id is in the list: lst[0, E) unsorted (E <= EXC_DIRECT_MAX), or lst[0, P) ascending with P a power of two >= E whose
// first E entries are the list (the rest INT64_MAX, which is nobody's id: a hit has to lie below E).
__device__ __forceinline__ bool exc_listed(const int64_t *lst, int E, int P, int64_t id)
{
    if (E <= EXC_DIRECT_MAX) {
        bool hit = false;
        for (int e = 0; e < E; ++e)
            hit |= lst[e] == id;
        return hit;
    }
    int pos = 0; // the first entry >= id: the steps add up to P - 1, so pos stays inside the list
    for (int s = P >> 1; s > 0; s >>= 1)
        if (lst[pos + s - 1] < id)
            pos += s;
    return pos < E && lst[pos] == id;
}

__global__ __launch_bounds__(EXC_THREADS) void exclude_ids_kernel(const float *__restrict__ in_val, const int64_t *__restrict__ in_idx,
                                                                  int M, const int64_t *__restrict__ exclude, int E, int P, int k,
                                                                  float *__restrict__ out_val, int64_t *__restrict__ out_idx)
{
    __shared__ int64_t lst[EXC_EMAX];
    __shared__ int wave_kept[2][EXC_WAVES]; // per chunk parity: one barrier per chunk
    const int tid = threadIdx.x, lane = tid & (TT_WAVE - 1), wave = tid / TT_WAVE;
    const int64_t row = blockIdx.x;
    in_val += row * M;
    in_idx += row * M;
    out_val += row * k;
    out_idx += row * k;

    if (E > 0) {
        const int64_t *ex = exclude + row * E;
        const int n = E <= EXC_DIRECT_MAX ? E : P;
        for (int e = tid; e < n; e += EXC_THREADS)
            lst[e] = e < E ? ex[e] : INT64_MAX;
        __syncthreads();
        if (E > EXC_DIRECT_MAX) { // bitonic sort, ascending (negative padding first, the INT64_MAX fill last)
            for (int len = 2; len <= P; len <<= 1)
                for (int j = len >> 1; j > 0; j >>= 1) {
                    for (int i = tid; i < P; i += EXC_THREADS) {
                        const int l = i ^ j;
                        if (l > i) {
                            const int64_t a = lst[i], b = lst[l];
                            if ((a > b) == ((i & len) == 0)) {
                                lst[i] = b;
                                lst[l] = a;
                            }
                        }
                    }
                    __syncthreads();
                }
        }
    }

    int base = 0; // entries kept so far (the same in every thread)
    for (int c = 0, it = 0; c < M && base < k; c += EXC_THREADS, ++it) {
        const int m = c + tid;
        int64_t id = -1;
        if (m < M)
            id = in_idx[m];
        const bool keep = id >= 0 && !exc_listed(lst, E, P, id); // (padding of the input row, idx < 0, is dropped: the tail is written below)
        const unsigned long long b = __ballot(keep);
        if (lane == 0)
            wave_kept[it & 1][wave] = __popcll(b);
        __syncthreads();
        int pos = base + __popcll(b & ((1ull << lane) - 1ull));
        int total = 0;
#pragma unroll
        for (int w = 0; w < EXC_WAVES; ++w) {
            const int n = wave_kept[it & 1][w];
            pos += w < wave ? n : 0;
            total += n;
        }
        if (keep && pos < k) {
            out_val[pos] = in_val[m];
            out_idx[pos] = id;
        }
        base += total;
    }
    for (int p = base + tid; p < k; p += EXC_THREADS) {
        out_val[p] = -INFINITY;
        out_idx[p] = -1;
    }
}

bool exc_overlap(const void *a, size_t na, const void *b, size_t nb)
{
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + nb && y < x + na;
}

} // namespace

TT_EXPORT int tt_topk_exclude_ids(const float *in_val, const int64_t *in_idx, int B, int M, const int64_t *exclude, int E, int k,
                                  float *out_val, int64_t *out_idx, tt_stream_t stream)
{
    if (B < 0 || M < 0 || E < 0 || k < 1 || k > M)
        return tt_fail(TT_ERR_BAD_SHAPE, "tt_topk_exclude_ids: B=%d M=%d E=%d k=%d (need 1 <= k <= M, E >= 0)", B, M, E, k);
    if (E > TT_TOPK_LARGE_KMAX - 1)
        return tt_fail(TT_ERR_UNSUPPORTED, "tt_topk_exclude_ids: E=%d > %d", E, TT_TOPK_LARGE_KMAX - 1);
    if (B == 0)
        return TT_OK;
    if (!in_val || !in_idx || !out_val || !out_idx || (E > 0 && !exclude))
        return tt_fail(TT_ERR_BAD_SHAPE, "tt_topk_exclude_ids: null pointer");
    if ((((uintptr_t)in_val | (uintptr_t)out_val) & 3) || (((uintptr_t)in_idx | (uintptr_t)out_idx | (uintptr_t)exclude) & 7))
        return tt_fail(TT_ERR_BAD_SHAPE, "tt_topk_exclude_ids: values must be 4-byte aligned, indices and ids 8-byte aligned");
    const size_t n_in = (size_t)B * M, n_out = (size_t)B * k;
    if (exc_overlap(in_val, n_in * 4, out_val, n_out * 4) || exc_overlap(in_idx, n_in * 8, out_idx, n_out * 8))
        return tt_fail(TT_ERR_BAD_SHAPE, "tt_topk_exclude_ids: out must not alias in");
    int P = 1;
    while (P < E)
        P <<= 1;
    hipLaunchKernelGGL(exclude_ids_kernel, dim3(B), dim3(EXC_THREADS), 0, (hipStream_t)stream, in_val, in_idx, M, exclude, E, P, k,
                       out_val, out_idx);
    TT_LAUNCH_CHECK();
    return TT_OK;
}
