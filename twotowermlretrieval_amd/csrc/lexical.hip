// Lexical search (DESIGN.md "Lexical search"): sparse TF-IDF rows times a sparse query, exact top-k, no [B,N] matrix.
// Score contract (include/tt.h): s(b,n) = ((0 + p_1) + p_2) + ..., p_i = fl32(vals[i] * q_b[cols[i]]) over the row's entries in
// stored order, every product rounded to fp32 (__fmul_rn) and added in fp32 (__fadd_rn): no FMA.  The chain is row-local --
// one lane owns one row and adds its products in order -- so a score depends on the row and the query alone, not on where
// the row lies in the nnz stream, on N, B, or the split over workgroups, slices or ranks.
// One workgroup (16 waves) takes one chunk of LEX_CHUNK documents of one query:
//   1. the query's dense image of F floats in LDS: zeroed, then the query's entries scattered (columns distinct);
//   2. four rounds of 64 rows per wave.  The 64 rows' entries are one contiguous span of the nnz stream: the wave walks it in
//      pieces of LEX_PIECE entries, loads cols / vals coalesced (the next piece's loads are in flight while the current one
//      is walked), gathers the query weight from the image and leaves the PRODUCT in its LDS stage; then each lane adds the
//      products of its own row that lie in the piece, in order, and carries the chain into the next piece (rows longer than
//      a piece, rows that straddle two);
//   3. top-k mode: the chunk's ranked values become 64-bit keys (inverted order key of the value, local index) in LDS; a
//      bitonic selection orders the best k by (value desc, index asc) -- the keys are distinct, so tie groups of any size
//      resolve by index: blocks of P = 2^ceil(log2 k) are sorted, then halved pairwise (elementwise minima + a merge) down
//      to one -- and they go out as the chunk's partial list, in tt_score_topk_partials_f32's form (idx -1 = empty).
// The existing merges finish (tt_topk_merge_large, which is tt_topk_merge up to k = 64): in one step up to LEX_DIRECT lists,
// above that in two (groups of about sqrt(lists) lists, one merge workgroup each, then the groups' results).
// No atomics, no host synchronisation; every word of the workspace is written before it is read.
#include <limits.h>
#include <math.h>

#include "tt_common.h"

namespace {

constexpr int LEX_THREADS = 1024;
constexpr int LEX_WAVES = LEX_THREADS / TT_WAVE;
constexpr int LEX_CHUNK = 4096;                       // documents per workgroup = per partial list
constexpr int LEX_ROUNDS = LEX_CHUNK / LEX_THREADS;   // rounds of one row per lane
constexpr int LEX_PIECE = 512;                        // staged entries per wave and step
constexpr int LEX_PER_LANE = LEX_PIECE / TT_WAVE;
constexpr int LEX_DIRECT = 64;                        // up to this many partial lists: one merge
constexpr unsigned long long LEX_EMPTY = ~0ull;       // key of a document that is no candidate: ranks last
static_assert(TT_LEXICAL_FMAX * 4 + LEX_WAVES * LEX_PIECE * 4 + LEX_CHUNK * 8 <= 160 * 1024 - 1024, "LDS budget of one CU");
static_assert(TT_TOPK_LARGE_KMAX <= LEX_CHUNK, "a chunk's list holds k entries");

struct LexParams {
    const int64_t *indptr;
    const int32_t *cols;
    const float *vals;
    int64_t N;
    int F;
    const int64_t *q_indptr;
    const int32_t *q_cols;
    const float *q_vals;
    const uint32_t *keep;
    const float *min_score;
    const float *base;
    int64_t base_stride;
    float w_base, w_lex;
    int k, n_lists; // top-k mode: entries per partial list, lists per query (the chunks, padded to whole merge groups)
    int64_t idx_offset;
    float *pval;    // [B][n_lists][k]
    int64_t *pidx;
    float *S;       // score-all mode: [B][N]
};

// The next piece of a wave's span in registers: entry p0 + t * 64 + lane; behind the span's end column -1 (dropped by the guard).
struct LexPiece {
    int c[LEX_PER_LANE];
    float v[LEX_PER_LANE];
    __device__ __forceinline__ void load(const int32_t *__restrict__ cols, const float *__restrict__ vals, int64_t p0, int64_t z,
                                         int lane)
    {
#pragma unroll
        for (int t = 0; t < LEX_PER_LANE; ++t) {
            const int64_t i = p0 + t * TT_WAVE + lane;
            const bool ok = i < z;
            c[t] = ok ? cols[i] : -1;
            v[t] = ok ? vals[i] : 0.0f;
        }
    }
};

// grid: x = chunk (top-k mode: padded to n_lists, the chunks behind N write empty lists), y = query
template <bool ALL>
__global__ __launch_bounds__(LEX_THREADS) void lexical_kernel(LexParams p)
{
    __shared__ float qimg[TT_LEXICAL_FMAX];
    __shared__ float stage[LEX_WAVES][LEX_PIECE];
    __shared__ unsigned long long keys[ALL ? 1 : LEX_CHUNK];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int b = blockIdx.y;
    const int64_t n0 = (int64_t)blockIdx.x * LEX_CHUNK;
    const int k = p.k;

    if (n0 < p.N) { // block-uniform
        for (int x = tid; x < p.F; x += LEX_THREADS)
            qimg[x] = 0.0f;
        __syncthreads();
        const int64_t qe = p.q_indptr[b + 1];
        for (int64_t j = p.q_indptr[b] + tid; j < qe; j += LEX_THREADS) {
            const int c = p.q_cols[j];
            if ((unsigned)c < (unsigned)p.F)
                qimg[c] = p.q_vals[j];
        }
        __syncthreads();

        float *st = stage[wv];
        for (int round = 0; round < LEX_ROUNDS; ++round) {
            const int li = round * LEX_THREADS + wv * TT_WAVE + lane; // the lane's document within the chunk
            const int64_t r = n0 + li;
            // rows at or behind N are empty rows at the end of the stream
            const int64_t s = p.indptr[r < p.N ? r : p.N];
            const int64_t e = p.indptr[r + 1 < p.N ? r + 1 : p.N];
            const int64_t a = __shfl(s, 0), z = __shfl(e, 63); // the wave's span of the nnz stream
            float acc = 0.0f;
            LexPiece cur;
            cur.load(p.cols, p.vals, a, z, lane);
            for (int64_t p0 = a; p0 < z; p0 += LEX_PIECE) {
#pragma unroll
                for (int t = 0; t < LEX_PER_LANE; ++t) {
                    const bool in = (unsigned)cur.c[t] < (unsigned)p.F; // one unsigned compare: a column outside [0,F) adds +0
                    const float w = qimg[in ? cur.c[t] : 0];
                    st[t * TT_WAVE + lane] = in ? __fmul_rn(cur.v[t], w) : 0.0f;
                }
                __builtin_amdgcn_wave_barrier();
                cur.load(p.cols, p.vals, p0 + LEX_PIECE, z, lane); // in flight during the walk (behind z: nothing is loaded)
                const int64_t lo = s > p0 ? s : p0, hi = e < p0 + LEX_PIECE ? e : p0 + LEX_PIECE;
                const int i1 = hi > lo ? (int)(hi - p0) : 0;
                // four products per step: the reads are independent, the adds are the chain.  acc is never -0 (it starts at
                // +0, and x + y = -0 only for x = y = -0), so the +0 a step reads behind the row's end changes nothing.
                for (int i = hi > lo ? (int)(lo - p0) : 0; i < i1; i += 4) {
                    const float f0 = st[i];
                    const float f1 = st[min(i + 1, LEX_PIECE - 1)];
                    const float f2 = st[min(i + 2, LEX_PIECE - 1)];
                    const float f3 = st[min(i + 3, LEX_PIECE - 1)];
                    acc = __fadd_rn(acc, f0);
                    acc = __fadd_rn(acc, i + 1 < i1 ? f1 : 0.0f);
                    acc = __fadd_rn(acc, i + 2 < i1 ? f2 : 0.0f);
                    acc = __fadd_rn(acc, i + 3 < i1 ? f3 : 0.0f);
                }
                __builtin_amdgcn_wave_barrier();
            }
            if (ALL) {
                if (r < p.N)
                    p.S[(size_t)b * (size_t)p.N + (size_t)r] = acc;
            } else {
                unsigned long long key = LEX_EMPTY;
                if (r < p.N) {
                    float v = acc;
                    if (p.base)
                        v = __fadd_rn(__fmul_rn(p.w_base, p.base[(size_t)b * (size_t)p.base_stride + (size_t)r]),
                                      __fmul_rn(p.w_lex, acc));
                    bool cand = p.min_score ? v >= p.min_score[b] : v == v; // a NaN is never selected
                    if (cand && p.keep)
                        cand = (p.keep[r >> 5] >> (r & 31)) & 1u;
                    if (cand) // -0 ranks as +0 (and is returned as +0): the order is that of the float compare
                        key = ((unsigned long long)~order_key(v == 0.0f ? 0.0f : v) << 32) | (unsigned)li;
                }
                keys[li] = key;
            }
        }
    } else if (!ALL) {
        for (int t = tid; t < k; t += LEX_THREADS)
            keys[t] = LEX_EMPTY;
    }
    if (ALL)
        return;
    __syncthreads();

    if (n0 < p.N) {
        // The P = 2^ceil(log2 k) smallest keys, ascending = (value desc, index asc), the non-candidates last -- a bitonic sort
        // that stops caring about what cannot be among them.  One stage: compare-exchange at distance j2 inside the first n
        // keys, ascending where bit k2 of the position is clear.
        auto stage = [&](int n, int k2, int j2) {
#pragma unroll
            for (int u = 0; u < LEX_CHUNK / 2 / LEX_THREADS; ++u) {
                const int t = tid + u * LEX_THREADS;
                if (t < n / 2) {
                    const int i = 2 * t - (t & (j2 - 1)), l = i + j2; // i has bit j2 clear
                    const unsigned long long x = keys[i], y = keys[l];
                    if (((i & k2) == 0) == (x > y)) {
                        keys[i] = y;
                        keys[l] = x;
                    }
                }
            }
            __syncthreads();
        };
        int P = 1;
        while (P < k)
            P <<= 1;
        // 1. blocks of P sorted, ascending and descending in turn
        for (int k2 = 2; k2 <= P; k2 <<= 1)
            for (int j2 = k2 >> 1; j2 > 0; j2 >>= 1)
                stage(LEX_CHUNK, k2, j2);
        // 2. halve: an ascending block and its descending neighbour form a bitonic sequence whose P smallest are the
        //    elementwise minima (bitonic themselves); the minima move to the front half, are merged into sorted blocks of
        //    alternating direction again, and so on down to one block
        for (int n = LEX_CHUNK; n > P;) {
            unsigned long long lo[LEX_CHUNK / 2 / LEX_THREADS];
#pragma unroll
            for (int u = 0; u < LEX_CHUNK / 2 / LEX_THREADS; ++u) {
                const int t = tid + u * LEX_THREADS;
                if (t < n / 2) {
                    const int at = 2 * t - (t & (P - 1)); // block 2m, position i: t = m P + i
                    const unsigned long long x = keys[at], y = keys[at + P];
                    lo[u] = x < y ? x : y;
                }
            }
            __syncthreads(); // every pair is read before the front half is overwritten
#pragma unroll
            for (int u = 0; u < LEX_CHUNK / 2 / LEX_THREADS; ++u) {
                const int t = tid + u * LEX_THREADS;
                if (t < n / 2)
                    keys[t] = lo[u];
            }
            __syncthreads();
            n >>= 1;
            for (int j2 = P >> 1; j2 > 0; j2 >>= 1)
                stage(n, P, j2);
        }
    }
    const size_t out = ((size_t)b * p.n_lists + blockIdx.x) * (size_t)k;
    for (int t = tid; t < k; t += LEX_THREADS) {
        const unsigned long long key = keys[t];
        const bool has = key != LEX_EMPTY;
        p.pval[out + t] = has ? order_key_to_float(~(unsigned)(key >> 32)) : -INFINITY;
        p.pidx[out + t] = has ? p.idx_offset + n0 + (int64_t)(unsigned)key : -1;
    }
}

// The partial lists of a search: n_chunks chunks in `groups` merge groups of `per` lists (one group: the direct merge).
struct LexPlan {
    int n_chunks, per, groups;
    int lists() const { return per * groups; }
};

LexPlan lex_plan(int64_t N)
{
    const int64_t nc = N > 0 ? (N + LEX_CHUNK - 1) / LEX_CHUNK : 1;
    LexPlan pl{(int)nc, (int)nc, 1};
    if (nc > LEX_DIRECT) {
        int per = (int)ceil(sqrt((double)nc));
        pl.per = per;
        pl.groups = (int)((nc + per - 1) / per);
    }
    return pl;
}

struct LexLayout {
    size_t pval, pidx, mval, midx, bytes;
};

LexLayout lex_layout(int B, int64_t N, int k)
{
    const LexPlan pl = lex_plan(N);
    const size_t n = (size_t)B * pl.lists() * k, m = pl.groups > 1 ? (size_t)B * pl.groups * k : 0;
    TTWorkspace ws;
    LexLayout l;
    l.pval = ws.take(n * sizeof(float));
    l.pidx = ws.take(n * sizeof(int64_t));
    l.mval = ws.take(m * sizeof(float));
    l.midx = ws.take(m * sizeof(int64_t));
    l.bytes = ws.off;
    return l;
}

// The checks the two entry points share: sizes, F, the corpus and the queries.
int lex_check_inputs(const char *who, const int64_t *indptr, const int32_t *cols, const float *vals, int64_t N, int F,
                     const int64_t *q_indptr, const int32_t *q_cols, const float *q_vals, int B)
{
    if (B < 0 || N < 0 || F <= 0)
        return tt_fail(TT_ERR_BAD_SHAPE, "%s: B=%d N=%lld F=%d", who, B, (long long)N, F);
    if (N >= (1ll << 31) - 64)
        return tt_fail(TT_ERR_UNSUPPORTED, "%s: N=%lld (need N < 2^31 - 64 per call: pass slices)", who, (long long)N);
    if (F > TT_LEXICAL_FMAX)
        return tt_fail(TT_ERR_UNSUPPORTED, "%s: F=%d > TT_LEXICAL_FMAX=%d", who, F, TT_LEXICAL_FMAX);
    if (B > 65535)
        return tt_fail(TT_ERR_UNSUPPORTED, "%s: B=%d > 65535 (one launch)", who, B);
    if (B == 0)
        return TT_OK;
    // cols / vals / q_cols / q_vals may be NULL when nothing is stored; only the device knows
    if (!indptr || !q_indptr)
        return tt_fail(TT_ERR_BAD_SHAPE, "%s: null indptr or q_indptr", who);
    if ((((uintptr_t)indptr | (uintptr_t)q_indptr) & 7) ||
        (((uintptr_t)cols | (uintptr_t)vals | (uintptr_t)q_cols | (uintptr_t)q_vals) & 3))
        return tt_fail(TT_ERR_BAD_SHAPE, "%s: indptr and q_indptr must be 8-byte aligned, columns and values 4-byte", who);
    return TT_OK;
}

} // namespace

TT_EXPORT int tt_lexical_chunk_docs(void) { return LEX_CHUNK; }

TT_EXPORT size_t tt_lexical_workspace_bytes(int B, int64_t N, int k)
{
    if (B <= 0 || N < 0 || N >= (1ll << 31) - 64 || k <= 0 || k > TT_TOPK_LARGE_KMAX)
        return 0;
    return lex_layout(B, N, k).bytes;
}

TT_EXPORT int tt_lexical_score_topk_f32(const int64_t *indptr, const int32_t *cols, const float *vals, int64_t N, int F,
                                        const int64_t *q_indptr, const int32_t *q_cols, const float *q_vals, int B,
                                        const uint32_t *keep, const float *min_score, const float *base, int64_t base_stride,
                                        float w_base, float w_lex, int k, int64_t idx_offset, float *out_val, int64_t *out_idx,
                                        void *workspace, size_t workspace_bytes, tt_stream_t stream)
{
    const char *who = "tt_lexical_score_topk_f32";
    if (k <= 0)
        return tt_fail(TT_ERR_BAD_SHAPE, "%s: k=%d", who, k);
    if (k > TT_TOPK_LARGE_KMAX)
        return tt_fail(TT_ERR_UNSUPPORTED, "%s: k=%d > %d", who, k, TT_TOPK_LARGE_KMAX);
    TT_RC_CHECK(lex_check_inputs(who, indptr, cols, vals, N, F, q_indptr, q_cols, q_vals, B));
    if (B == 0)
        return TT_OK;
    if (base && base_stride < N)
        return tt_fail(TT_ERR_BAD_SHAPE, "%s: base_stride=%lld < N=%lld", who, (long long)base_stride, (long long)N);
    if (!out_val || !out_idx)
        return tt_fail(TT_ERR_BAD_SHAPE, "%s: null output", who);
    if ((((uintptr_t)out_val | (uintptr_t)keep | (uintptr_t)min_score | (uintptr_t)base) & 3) || ((uintptr_t)out_idx & 7))
        return tt_fail(TT_ERR_BAD_SHAPE, "%s: out_idx must be 8-byte aligned, out_val, keep, min_score and base 4-byte", who);
    const LexLayout l = lex_layout(B, N, k);
    if (!workspace || workspace_bytes < l.bytes || ((uintptr_t)workspace & 7))
        return tt_fail(TT_ERR_WORKSPACE, "%s: workspace %zu bytes, need %zu (8-byte aligned)", who, workspace_bytes, l.bytes);

    const LexPlan pl = lex_plan(N);
    char *ws = (char *)workspace;
    LexParams p{indptr, cols, vals, N, F, q_indptr, q_cols, q_vals, keep, min_score, base, base_stride, w_base, w_lex,
                k, pl.lists(), idx_offset, (float *)(ws + l.pval), (int64_t *)(ws + l.pidx), nullptr};
    hipLaunchKernelGGL(lexical_kernel<false>, dim3(pl.lists(), B), dim3(LEX_THREADS), 0, (hipStream_t)stream, p);
    TT_LAUNCH_CHECK();
    if (pl.groups == 1)
        return tt_topk_merge_large(p.pval, p.pidx, B, pl.lists() * k, k, out_val, out_idx, stream);
    float *mval = (float *)(ws + l.mval);
    int64_t *midx = (int64_t *)(ws + l.midx);
    TT_RC_CHECK(tt_topk_merge_large(p.pval, p.pidx, B * pl.groups, pl.per * k, k, mval, midx, stream));
    return tt_topk_merge_large(mval, midx, B, pl.groups * k, k, out_val, out_idx, stream);
}

TT_EXPORT int tt_lexical_score_all_f32(const int64_t *indptr, const int32_t *cols, const float *vals, int64_t N, int F,
                                       const int64_t *q_indptr, const int32_t *q_cols, const float *q_vals, int B, float *S,
                                       tt_stream_t stream)
{
    const char *who = "tt_lexical_score_all_f32";
    TT_RC_CHECK(lex_check_inputs(who, indptr, cols, vals, N, F, q_indptr, q_cols, q_vals, B));
    if (B == 0 || N == 0)
        return TT_OK;
    if (!S || ((uintptr_t)S & 3))
        return tt_fail(TT_ERR_BAD_SHAPE, "%s: S null or not 4-byte aligned", who);
    LexParams p{indptr, cols, vals, N, F, q_indptr, q_cols, q_vals, nullptr, nullptr, nullptr, 0, 0.0f, 0.0f,
                0, 0, 0, nullptr, nullptr, S};
    hipLaunchKernelGGL(lexical_kernel<true>, dim3((unsigned)lex_plan(N).n_chunks, B), dim3(LEX_THREADS), 0, (hipStream_t)stream, p);
    TT_LAUNCH_CHECK();
    return TT_OK;
}
