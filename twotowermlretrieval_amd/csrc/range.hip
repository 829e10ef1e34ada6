// Threshold search (DESIGN.md "Threshold search"), the parts around the counting pass of score_topk.hip: the sum of a query's
// per-chunk counts, and the cut of sorted top-k rows at a per-query threshold.
#include <math.h>

#include "score_topk.h"

namespace {

// count[b] (+)= the sum of part[b][0, n_chunks): one wave per query.  Integer sums: the order does not matter.
__global__ __launch_bounds__(TT_WAVE) void count_finish_kernel(const int64_t *__restrict__ part, int n_chunks,
                                                               int64_t *__restrict__ count, int accumulate)
{
    const int b = blockIdx.x, lane = threadIdx.x;
    int64_t s = 0;
    for (int c = lane; c < n_chunks; c += TT_WAVE)
        s += part[(size_t)b * n_chunks + c];
#pragma unroll
    for (int off = TT_WAVE / 2; off >= 1; off >>= 1)
        s += __shfl_xor(s, off);
    if (lane == 0)
        count[b] = accumulate ? count[b] + s : s;
}

constexpr int CUT_THREADS = 256;

__global__ __launch_bounds__(CUT_THREADS) void cut_below_kernel(float *__restrict__ val, int64_t *__restrict__ idx, int64_t total,
                                                                int k, const float *__restrict__ min_score)
{
    const int64_t i = (int64_t)blockIdx.x * CUT_THREADS + threadIdx.x;
    if (i >= total)
        return;
    if (!(val[i] >= min_score[i / k]) || idx[i] < 0) { // (a NaN threshold cuts the whole row)
        val[i] = -INFINITY;
        idx[i] = -1;
    }
}

} // namespace

int tt_count_finish(const int64_t *part, int B, int n_chunks, int64_t *count, int accumulate, hipStream_t st)
{
    hipLaunchKernelGGL(count_finish_kernel, dim3(B), dim3(TT_WAVE), 0, st, part, n_chunks, count, accumulate);
    TT_LAUNCH_CHECK();
    return TT_OK;
}

TT_EXPORT int tt_topk_cut_below(float *val, int64_t *idx, int B, int k, const float *min_score, tt_stream_t stream)
{
    if (B < 0 || k <= 0)
        return tt_fail(TT_ERR_BAD_SHAPE, "tt_topk_cut_below: B=%d k=%d", B, k);
    if (B == 0)
        return TT_OK;
    if (!val || !idx || !min_score)
        return tt_fail(TT_ERR_BAD_SHAPE, "tt_topk_cut_below: null pointer");
    if ((((uintptr_t)val | (uintptr_t)min_score) & 3) || ((uintptr_t)idx & 7))
        return tt_fail(TT_ERR_BAD_SHAPE, "tt_topk_cut_below: values and thresholds must be 4-byte aligned, indices 8-byte aligned");
    const int64_t total = (int64_t)B * k;
    hipLaunchKernelGGL(cut_below_kernel, dim3((unsigned)((total + CUT_THREADS - 1) / CUT_THREADS)), dim3(CUT_THREADS), 0,
                       (hipStream_t)stream, val, idx, total, k, min_score);
    TT_LAUNCH_CHECK();
    return TT_OK;
}
