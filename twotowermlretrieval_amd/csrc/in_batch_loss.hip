// K9 softmax contrastive loss of B queries over a pool of M >= B documents (forward + gradient) on the f32-input MFMA (gfx950).
//
//   qh_i = q_i / max(||q_i||, eps)     Dh_j = D_j / max(||D_j||, eps)     eps = 1e-8
//   s_ij = (qh_i . Dh_j) / temperature      loss = mean_i (logsumexp_j s_ij - s_{i, pos_offset + i})       i < B, j < M
//
// Two entries on the same kernels: tt_contrastive_loss_f32 (one contiguous pool `docs` [M,H]: the passages gathered from all
// ranks, or several negatives per query) and tt_in_batch_loss_f32 (D = [p; n] as two pointers: M = 2B, pos_offset = 0).
//
// Grouped negatives (tt_contrastive_loss_grouped_f32, the GROUPED instantiations): int64 labels qg [B], dg [M]; the pair (i, j)
// is IGNORED iff j != pos_offset + i, qg[i] >= 0 and dg[j] == qg[i] -- another positive of the same query is no negative.  An
// ignored pair is left out of the maximum and of the sum of exponentials exactly as a document past M is, and its G entry is 0
// on both gradient sides.  The positive is always kept, so lse_i is finite; but a tile, a lane's share of a slice or a whole
// slice may hold no kept document for a query: such a partial is (max, sum) = (-inf, 0), every combine skips a zero sum before it
// forms exp(max - total max), and no exp(-inf - -inf) is ever evaluated.  A query whose every other row is ignored has
// lse_i = s_{i,pos} + log(1): row loss 0.0f and G row exp(0) - 1 = 0.  The ungrouped instantiations read no label and keep their
// arithmetic and order.
//
// Soft targets (tt_contrastive_loss_soft_f32, the SOFT instantiations; never together with GROUPED): f32 weights t [B][M] in
// place of the one positive per query,
//   w_i = sum_j t_ij     loss = mean_i (w_i lse_i - sum_j t_ij s_ij)     d loss / d s_ij = (w_i exp(s_ij - lse_i) - t_ij) / B
// the cross-entropy of the row softmax against t_i.  The softmax statistics are the plain instantiation's, statement for
// statement; beside them a lane sums tw += t and ts = fmaf(t, s, ts) over its documents in the same order (16 per tile in
// register order, tiles ascending, the 8 partials of a query in wave * 2 + half order, slices ascending).  A one-hot row gives
// w = 1.0f and ts = s_pos exactly (zeros leave an fmaf chain where it is), so w lse - ts and w e - t are the pooled entry's
// lse - s_pos and e - onehot bit for bit; an all-zero row gives 0 lse - 0 and (0 e - 0) scale: nothing.  Targets are loaded
// like the labels -- unconditionally, at indices clamped into [0, B) x [0, M), element i M + j addressed in 64 bits -- and a pair
// past the end selects 0.
//
// Symmetric loss (tt_contrastive_loss_sym_f32, the ib_sym_* kernels; with or without labels, never SOFT): the positive document
// P_i = pos_offset + i is also classified among the B queries, down column P_i of the score matrix,
//   L_qd = mean_i (lse_i - s_{i,P_i})     L_dq = mean_i (clse_i - s_{i,P_i})     clse_c = logsumexp_{i'<B} s_{i',pos_offset+c}
//   loss = (1 - alpha) L_qd + alpha L_dq      B T dL/ds_ij = (1 - alpha) (e^{s_ij - lse_i} - [j == P_i])
//                                                            + alpha [0 <= c < B] (e^{s_ij - clse_c} - [j == P_i]),  c = j - pos_offset
// Only the B positive columns have a softmax of their own; every other document is a negative of the row direction alone.
// The column statistics are the row statistics with the roles swapped (ib_stats_body<.., COLS>): a workgroup owns the 32
// documents of an ALIGNED tile of the image that meets [pos_offset, pos_offset + B) (pos_offset need not be a multiple of 32:
// a lane whose document is no positive column computes and writes nothing; every tile lies inside the padded image) and walks
// a slice of the queries, ib_slices(B, B).  A query past B is a zero image row that scores a finite 0: it is masked out of
// the column sums exactly as a document past M is masked out of the rows.  With labels the one ignore predicate takes the
// pair out of row i's sum, of column j's sum and of G; column c always keeps (c, P_c), so clse_c is finite, and a column
// whose every other query is ignored has clse_c = s_{c,P_c} + log(1): column loss 0.0f.  The row statistics, lse_i and the
// sum of the mixed row losses are the plain kernels' statements; the row loss is (1 - alpha) a + alpha b and G likewise, so
// alpha = 0 gives the plain (grouped) entry's bits (1 a + 0 b = a for finite b), and alpha = 1 gives an exact zero in every
// G entry outside the positive columns.  Launches: 1, ib_sym_stats_kernel (2 with the column tiles behind the row tiles in one
// grid), ib_sym_lse_kernel (3, also clse and the two directions' row losses), 4 three times (loss, L_qd, L_dq),
// ib_sym_grad_kernel (5), 6.
//
// Device-resident logit scale (tt_contrastive_loss_ls_f32 = plain / grouped / soft, tt_contrastive_loss_sym_ls_f32; the *_ls
// and *_dots kernels): the temperature is no argument but a word l = log(1 / T) in device memory that the kernels read WHEN THEY
// RUN (a graph replay sees what the word holds then).  The first thread of launch 1 forms T = expf(-clamp(l, lo, hi)) once --
// the clamp as comparisons, so a NaN stays a NaN -- and stores it in the workspace (and in temperature_out); launches 2 and 5 load
// that word and are otherwise the float entries' bodies with `temperature` = it: scores acc / T, scale 1 / (B T), statement
// for statement, so the float entry called at the T read back writes the same bytes.  The scale's gradient needs nothing new:
// with G = (dL/ds) / T the matrix launch 5 forms and c_ij = qh_i . Dh_j,
//   dL/dl = dL/d log(1/T) = sum_ij (dL/ds_ij) s_ij = sum_ij G_ij c_ij = sum_{i<B} qh_i . dqh_i        (dqh = G Dh)
// for every variant (dqh carries every term of G), and qh_i . dqh_i is the dot launch 6 forms for its back-projection (which is
// why dq cannot give it back: q_i . dq_i = 0).  ib_project_dots_kernel stores it per query -- +0.0f where the clamp holds
// gradient back, by a select -- and one more ib_sum_kernel adds the B dots, scale 1, in its fixed order.  No address depends on T.
//
// Six launches on one stream (four without gradients), no cross-workgroup wait, no atomics:
//   1 ib_prep_kernel     one wave per row: clamped norm, normalised zero-padded images qh [Bq][Hp], Dh [Dp][Hp]
//   2 ib_stats_kernel    a workgroup per (32 queries, slice of the documents): S^T tiles on v_mfma_f32_32x32x2_f32, online
//                        (max, sum exp) per lane, fixed-order combine -> the slice's (max, sum exp) per query
//   3 ib_lse_kernel      a thread per query: the slices' partials in ascending order -> lse_i, row loss_i
//   4 ib_sum_kernel      fixed-order mean of the row losses
//   5 ib_grad_kernel     a workgroup per (32 queries, slice of the documents): recomputes S^T, G = (exp(s - lse) - onehot) /
//                        (B temperature) through LDS, partial dqh = G Dh; and, in the same launch with the roles swapped, a
//                        workgroup per (32 documents, slice of the queries): partial dDh = G^T qh
//   6 ib_project_kernel  one wave per row: the slices' partials in ascending order, back-projection through the norm
//                        -> dq, ddocs (dp, dn)
// [B,M] never reaches memory.  Every sum has one fixed order (the MFMA's k order, chunks of 128 rows ascending, slices
// ascending, xor trees), and the slicing depends on (B, M, H) alone, so the result is bit-reproducible and independent of what
// the workspace held.
#include <float.h>

#include "tt_common.h"

namespace {

constexpr int IB_TILE = 32;    // rows a workgroup owns (query-tile height / document-tile width): one MFMA tile
constexpr int IB_CHUNK = 128;  // rows of the other side per iteration: one 32-row tile per wave
constexpr int IB_MAX_H = 512;
constexpr float IB_EPS = 1e-8f;
constexpr int IB_WANT_WGS = 256;  // workgroups a pass aims at (a constant, not the device's CU count: same bits everywhere)
constexpr int IB_MAX_SLICES = 8;
constexpr int IB_KB = 8;  // MFMA k-steps (of 2 rows) per prefetched batch of the gradient product

// The rows a pass walks, cut into slices of whole chunks: n_slices slices of `per` chunks, none empty.
struct IBSlices {
    int per, n;
};
IBSlices ib_slices(int walked_rows, int owner_rows)
{
    const int chunks = (walked_rows + IB_CHUNK - 1) / IB_CHUNK, tiles = (owner_rows + IB_TILE - 1) / IB_TILE;
    int want = IB_WANT_WGS / tiles;
    want = want > IB_MAX_SLICES ? IB_MAX_SLICES : (want < 1 ? 1 : want);
    want = want > chunks ? chunks : want;
    const int per = (chunks + want - 1) / want;
    return {per, (chunks + per - 1) / per};
}

struct IBPlan {
    int Hp, Bq, Dp;   // image width (H up to a multiple of 32), image heights (B, M up to multiples of IB_CHUNK)
    IBSlices sq, sd;  // slices of the documents a query tile walks / of the queries a document tile walks
    size_t qh, dh, den, flag, lse, rows, pm, pl, pos, part_q, part_d, total;
    size_t pw, pt, w;  // soft targets only, behind everything else
    IBSlices sc;       // symmetric only: slices of the queries a tile of positive columns walks (statistics)
    size_t cpm, cpl, clse, rows_qd, rows_dq;  // symmetric only, behind everything else
    size_t tword, dots;  // device-resident scale only, behind everything else
};

IBPlan ib_plan(int B, int M, int H, bool soft = false, bool sym = false, bool ls = false)
{
    IBPlan P;
    P.Hp = (H + 31) / 32 * 32;
    P.Bq = (B + IB_CHUNK - 1) / IB_CHUNK * IB_CHUNK;
    P.Dp = (M + IB_CHUNK - 1) / IB_CHUNK * IB_CHUNK;
    TTWorkspace w;
    P.qh = w.take(sizeof(float) * (size_t)P.Bq * P.Hp);
    P.dh = w.take(sizeof(float) * (size_t)P.Dp * P.Hp);
    P.den = w.take(sizeof(float) * (size_t)(P.Bq + P.Dp));   // max(norm, eps): queries, then documents
    P.flag = w.take(sizeof(float) * (size_t)(P.Bq + P.Dp));  // 1 where norm >= eps (the clamp passes gradient), else 0
    P.lse = w.take(sizeof(float) * (size_t)P.Bq);
    P.rows = w.take(sizeof(float) * (size_t)P.Bq);
    P.sq = ib_slices(M, B);
    P.sd = ib_slices(B, M);
    P.pm = w.take(sizeof(float) * (size_t)P.sq.n * P.Bq);  // per (slice, query): running maximum, sum of exponentials
    P.pl = w.take(sizeof(float) * (size_t)P.sq.n * P.Bq);
    P.pos = w.take(sizeof(float) * (size_t)P.Bq);          // s_{i, pos_offset + i}
    P.part_q = w.take(sizeof(float) * (size_t)P.sq.n * P.Bq * P.Hp);  // per slice: partial dqh [Bq][Hp], dDh [Dp][Hp]
    P.part_d = w.take(sizeof(float) * (size_t)P.sd.n * P.Dp * P.Hp);
    P.pw = P.pt = P.w = 0;
    if (soft) {  // (appended: the offsets above are the plain plan's)
        P.pw = w.take(sizeof(float) * (size_t)P.sq.n * P.Bq);  // per (slice, query): sum of the targets, sum of target * score
        P.pt = w.take(sizeof(float) * (size_t)P.sq.n * P.Bq);
        P.w = w.take(sizeof(float) * (size_t)P.Bq);            // w_i, padded like lse
    }
    P.sc = ib_slices(B, B);
    P.cpm = P.cpl = P.clse = P.rows_qd = P.rows_dq = 0;
    if (sym) {  // (appended likewise)
        P.cpm = w.take(sizeof(float) * (size_t)P.sc.n * P.Bq);  // per (slice, positive column): maximum, sum of exponentials
        P.cpl = w.take(sizeof(float) * (size_t)P.sc.n * P.Bq);
        P.clse = w.take(sizeof(float) * (size_t)P.Bq);          // clse_c, padded like lse
        P.rows_qd = w.take(sizeof(float) * (size_t)P.Bq);       // lse_i - s_pos, clse_i - s_pos
        P.rows_dq = w.take(sizeof(float) * (size_t)P.Bq);
    }
    P.tword = P.dots = 0;
    if (ls) {  // (appended likewise)
        P.tword = w.take(sizeof(float) * 4);               // T = exp(-clamp(l)); 1 where the clamp passes gradient, else 0
        P.dots = w.take(sizeof(float) * (size_t)P.Bq);     // qh_i . dqh_i
    }
    P.total = w.off;
    return P;
}

// ------------------------------------------------------------------ 1: norms and images
// The documents as the caller holds them: rows [0, split) at `lo`, rows [split, M) at `hi` (one contiguous pool: split = M).
struct IBDocs {
    const float *lo, *hi;
    int split;
};
struct IBDocGrads {
    float *lo, *hi;
    int split;
};

// Row r of [queries (Bq rows); documents (Dp rows)]; rows past B / M and columns past H are written as zeros.
__device__ __forceinline__ void ib_prep_body(const float *__restrict__ q, IBDocs docs, int B, int M, int H, int Hp, int Bq,
                                             int Dp, float *__restrict__ qh, float *__restrict__ dh,
                                             float *__restrict__ den, float *__restrict__ flag)
{
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= Bq + Dp)
        return;
    const float *src = nullptr;
    float *dst;
    if (r < Bq) {
        src = r < B ? q + (size_t)r * H : nullptr;
        dst = qh + (size_t)r * Hp;
    } else {
        const int j = r - Bq;
        src = j < docs.split ? docs.lo + (size_t)j * H : (j < M ? docs.hi + (size_t)(j - docs.split) * H : nullptr);
        dst = dh + (size_t)j * Hp;
    }
    float ss = 0.0f;
    if (src)
        for (int u = lane; u < H; u += 64)
            ss += src[u] * src[u];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1)
        ss += __shfl_xor(ss, off);
    const float norm = sqrtf(ss);
    const float d = fmaxf(norm, IB_EPS);
    for (int u = lane; u < Hp; u += 64)
        dst[u] = (src && u < H) ? src[u] / d : 0.0f;
    if (lane == 0) {
        den[r] = d;
        flag[r] = norm >= IB_EPS ? 1.0f : 0.0f;
    }
}

__global__ __launch_bounds__(256) void ib_prep_kernel(const float *__restrict__ q, IBDocs docs, int B, int M, int H, int Hp,
                                                      int Bq, int Dp,
                                                      float *__restrict__ qh, float *__restrict__ dh,
                                                      float *__restrict__ den, float *__restrict__ flag)
{
    ib_prep_body(q, docs, B, M, H, Hp, Bq, Dp, qh, dh, den, flag);
}

// The device-resident scale (the *_ls entries): the same launch, and its first thread forms the temperature of the whole call
// from the word l = *log_scale as it is NOW, when the kernel runs (a graph replay reads what the word holds at replay):
//   T = expf(-clamp(l, lo, hi)) -> tw[0] (and t_out);  tw[1] = 1 where lo <= l <= hi (the clamp passes gradient), else 0.
// The clamp is comparisons, not fminf/fmaxf: a NaN l fails both and stays a NaN (and its gate is 1: the NaN reaches every
// output that depends on T).  Every later launch of the call reads tw[0]; no address depends on it.
__global__ __launch_bounds__(256) void ib_prep_ls_kernel(const float *__restrict__ q, IBDocs docs, int B, int M, int H, int Hp,
                                                         int Bq, int Dp, float *__restrict__ qh, float *__restrict__ dh,
                                                         float *__restrict__ den, float *__restrict__ flag,
                                                         const float *__restrict__ log_scale, float lo, float hi,
                                                         float *__restrict__ tw, float *__restrict__ t_out)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const float l = log_scale[0];
        const float lc = l < lo ? lo : (l > hi ? hi : l);
        const float T = expf(-lc);
        tw[0] = T;
        tw[1] = (l < lo || l > hi) ? 0.0f : 1.0f;
        if (t_out)
            t_out[0] = T;
    }
    ib_prep_body(q, docs, B, M, H, Hp, Bq, Dp, qh, dh, den, flag);
}

// S^T tile on the matrix pipe: acc[reg] = A_row(a0 + rho(reg) + 4 * (lane >> 5)) . B_row(b0 + (lane & 31)), rho(reg) =
// (reg & 3) + 8 * (reg >> 2).  Both images are [rows][Hp] with Hp % 32 == 0; each lane loads 4 consecutive k of its row for
// four MFMA steps (the k order inside a group of 8 is permuted identically for both operands).  Two accumulators (even and odd
// groups of 8) are added at the end.  One wave per SIMD has nobody to hide a load behind, so the loop is software-pipelined:
// the 32 columns of the next step are in flight while the 16 MFMAs (1024 cycles) of this one issue.
// after_first(): further loads of the caller's (the grouped kernels' labels), issued BEHIND the first step's operands, so that
// the wait in front of the first MFMA does not cover them (loads retire in order) and they land behind the products.
struct IBFrag {
    f32x4 a[4], b[4];
};
__device__ __forceinline__ IBFrag ib_frag(const float *__restrict__ ap, const float *__restrict__ bp, int k)
{
    IBFrag f;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        f.a[g] = *(const f32x4 *)(ap + k + 8 * g);
        f.b[g] = *(const f32x4 *)(bp + k + 8 * g);
    }
    return f;
}
template <class AfterFirst>
__device__ __forceinline__ f32x16 ib_scores(const float *__restrict__ A, int a0, const float *__restrict__ Bm, int b0,
                                            int Hp, int lane, AfterFirst after_first)
{
    const float *ap = A + (size_t)(a0 + (lane & 31)) * Hp + 4 * (lane >> 5);
    const float *bp = Bm + (size_t)(b0 + (lane & 31)) * Hp + 4 * (lane >> 5);
    f32x16 acc0 = {}, acc1 = {};
    IBFrag cur = ib_frag(ap, bp, 0);
    after_first();
    for (int k = 0; k < Hp; k += 32) {  // Hp % 32 == 0
        IBFrag nxt = cur;
        if (k + 32 < Hp)
            nxt = ib_frag(ap, bp, k + 32);
#pragma unroll
        for (int g = 0; g < 4; g += 2)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(cur.a[g][e], cur.b[g][e], acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(cur.a[g + 1][e], cur.b[g + 1][e], acc1, 0, 0, 0);
            }
        cur = nxt;
    }
    return acc0 + acc1;
}

__device__ __forceinline__ int ib_rho(int reg) { return (reg & 3) + 8 * (reg >> 2); }

// The labels of the 16 rows y0 + rho(r) + 4 * half a lane meets in an S^T tile.  Rows past n read row n - 1 (n >= 1): every load
// is in bounds and unconditional (no branch around a load), and what such a row holds is never used -- the pair is out of range.
__device__ __forceinline__ void ib_labels(const int64_t *__restrict__ g, int y0, int half, int n, int64_t (&out)[16])
{
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int y = y0 + ib_rho(r) + 4 * half;
        out[r] = g[y < n ? y : n - 1];
    }
}

// The targets t[i][y0 + rho(r) + 4 * half] (ALONG: the lane's own query i, 16 documents: row stride M between lanes) or
// t[y0 + rho(r) + 4 * half][j] (!ALONG: 16 queries, the lane's own document j: consecutive lanes, consecutive addresses).  Like
// ib_labels: both indices clamped into the array, every load in bounds and unconditional; what a pair past the end loads is
// replaced by 0 where it is used.  The element index is formed in 64 bits (B * M passes 2^32).
template <bool ALONG>
__device__ __forceinline__ void ib_targets(const float *__restrict__ t, int own, int n_own, int y0, int half, int n_oth, int M,
                                           float (&out)[16])
{
    const size_t fixed = (size_t)(own < n_own ? own : n_own - 1);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int y = y0 + ib_rho(r) + 4 * half;
        const size_t yc = (size_t)(y < n_oth ? y : n_oth - 1);
        out[r] = ALONG ? t[fixed * (size_t)M + yc] : t[yc * (size_t)M + fixed];
    }
}

// ------------------------------------------------------------------ 2: row statistics
// Workgroup = 32 queries (on the lanes) x slice blockIdx.y of the documents; wave w takes the 32-document tiles w, w + 4, ... of
// the slice.  Each lane keeps a running maximum and a sum of exponentials over the documents it sees; the 8 partials of a
// query (4 waves x 2 lane halves) are combined in a fixed order into the slice's pair.  Ungrouped, a slice holds a valid
// document for every query (slices are whole chunks, none empty).  GROUPED, every document of a slice may be ignored for a
// query: its partials are (-inf, 0), the combine below skips them (part_l > 0) and the slice's pair is (-inf, 0).
// GROUPED: the lane loads its query's label once and, per tile, the labels of its 16 documents behind the first operands of the
// products (ib_scores: after_first), so that they arrive behind the MFMAs.
// SOFT: the lane loads the 16 targets of its query's row in the same place and sums (t, t * s) beside (max, sum exp): per lane
// in register order, tiles ascending; the 8 partials of a query in the order of the combine below; pos[] is not written.
template <bool GROUPED, bool SOFT>
__global__ __launch_bounds__(256) void ib_stats_kernel(const float *__restrict__ qh, const float *__restrict__ dh,
                                                       const int64_t *__restrict__ qg, const int64_t *__restrict__ dg, int B, int M,
                                                       int pos_offset, int Hp, int Bq, int tiles_per_slice, float temperature,
                                                       float *__restrict__ pm, float *__restrict__ pl,
                                                       float *__restrict__ pos, const float *__restrict__ tg,
                                                       float *__restrict__ pw, float *__restrict__ pt)
{
    __shared__ float part_m[8][IB_TILE], part_l[8][IB_TILE];
    __shared__ float part_w[SOFT ? 8 : 1][IB_TILE], part_t[SOFT ? 8 : 1][IB_TILE];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), half = lane >> 5;
    const int i0 = blockIdx.x * IB_TILE, i = i0 + (lane & 31);
    const int ND = M;
    const int t_begin = blockIdx.y * tiles_per_slice;
    const int t_all = (ND + IB_TILE - 1) / IB_TILE, n_tiles = t_begin + tiles_per_slice < t_all ? t_begin + tiles_per_slice : t_all;
    float m = -INFINITY, l = 0.0f;
    int64_t own_g = -1, oth_g[16];
    if (GROUPED)
        own_g = qg[i < B ? i : B - 1];  // (a lane past B: any label, its statistics are not written)
    const bool grouped_q = own_g >= 0;
    float tw = 0.0f, ts = 0.0f, tv[16];
    for (int t = t_begin + wave; t < n_tiles; t += 4) {
        const int j0 = t * IB_TILE;
        const f32x16 acc = ib_scores(dh, j0, qh, i0, Hp, lane, [&] {
            if (GROUPED)
                ib_labels(dg, j0, half, ND, oth_g);
            if (SOFT)
                ib_targets<true>(tg, i, B, j0, half, ND, M, tv);
        });
        float x[16], tm = -INFINITY;
        bool keep[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int j = j0 + ib_rho(r) + 4 * half;
            x[r] = acc[r] / temperature;
            keep[r] = j < ND;
            if (GROUPED)  // (bitwise: one mask per pair, no branch per document)
                keep[r] = keep[r] & !(grouped_q & (oth_g[r] == own_g) & (j != i + pos_offset));
            if (keep[r])
                tm = fmaxf(tm, x[r]);
            if (!SOFT && j == i + pos_offset && i < B)
                pos[i] = x[r];  // (one lane of one wave of one slice, once)
            if (SOFT) {  // (a document past M: weight 0, and its score is that of a zero row: finite)
                const float tr = j < ND ? tv[r] : 0.0f;
                tw += tr;
                ts = fmaf(tr, x[r], ts);
            }
        }
        if (tm > -INFINITY) {  // (some document of the tile is valid, and kept, for this lane)
            const float mn = fmaxf(m, tm);
            float s = 0.0f;
#pragma unroll
            for (int r = 0; r < 16; ++r)
                if (keep[r])
                    s += expf(x[r] - mn);
            l = l * expf(m - mn) + s;  // (m = -inf: l = 0 and exp(-inf) = 0)
            m = mn;
        }
    }
    part_m[wave * 2 + half][lane & 31] = m;
    part_l[wave * 2 + half][lane & 31] = l;
    if (SOFT) {
        part_w[wave * 2 + half][lane & 31] = tw;
        part_t[wave * 2 + half][lane & 31] = ts;
    }
    __syncthreads();
    if (threadIdx.x < IB_TILE && i0 + (int)threadIdx.x < B) {
        const int c = threadIdx.x;
        float M = -INFINITY;
        for (int k = 0; k < 8; ++k)
            M = fmaxf(M, part_m[k][c]);
        float L = 0.0f;
        for (int k = 0; k < 8; ++k)
            if (part_l[k][c] > 0.0f)
                L += part_l[k][c] * expf(part_m[k][c] - M);
        pm[(size_t)blockIdx.y * Bq + i0 + c] = M;
        pl[(size_t)blockIdx.y * Bq + i0 + c] = L;
        if (SOFT) {
            float W = 0.0f, T = 0.0f;
            for (int k = 0; k < 8; ++k) {
                W += part_w[k][c];
                T += part_t[k][c];
            }
            pw[(size_t)blockIdx.y * Bq + i0 + c] = W;
            pt[(size_t)blockIdx.y * Bq + i0 + c] = T;
        }
    }
}

// ib_stats_kernel's body as a function of (tile, slice), for the symmetric loss's statistics launch.  !COLS: the statements of
// the kernel above, one for one (the kernel itself keeps its text: moving it behind a call changes what the compiler knows
// about its pointers, and with that its registers).
// COLS (the symmetric loss's column statistics; never SOFT): the roles swapped.  The workgroup owns the 32 DOCUMENTS of image
// tile `tile` (on the lanes) and walks slice `slice` of the QUERIES; the lane's column is c = document - pos_offset, and
// pm/pl are the column partials [slice][Bq] indexed by c, written for 0 <= c < B alone (a document tile is aligned to the
// image, not to pos_offset: the lanes in front of the first and behind the last positive column compute and write nothing
// that is kept).  A query past B is masked as a document past M is above; the pair (i', j) is ignored by the same predicate,
// read from the other side: the walked query's label is non-negative and equals the own document's, and i' != c.  pos[] is
// the row pass's to write.
template <bool GROUPED, bool SOFT, bool COLS>
__device__ __forceinline__ void ib_stats_body(const float *__restrict__ qh, const float *__restrict__ dh, const int64_t *__restrict__ qg,
                                              const int64_t *__restrict__ dg, int B, int M, int pos_offset, int Hp, int Bq,
                                              int tiles_per_slice, float temperature, float *__restrict__ pm,
                                              float *__restrict__ pl, float *__restrict__ pos, const float *__restrict__ tg,
                                              float *__restrict__ pw, float *__restrict__ pt, unsigned tile, unsigned slice)
{
    __shared__ float part_m[8][IB_TILE], part_l[8][IB_TILE];
    __shared__ float part_w[SOFT ? 8 : 1][IB_TILE], part_t[SOFT ? 8 : 1][IB_TILE];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), half = lane >> 5;
    const int i0 = tile * IB_TILE, i = i0 + (lane & 31);
    const int ND = COLS ? B : M;
    const int t_begin = slice * tiles_per_slice;
    const int t_all = (ND + IB_TILE - 1) / IB_TILE, n_tiles = t_begin + tiles_per_slice < t_all ? t_begin + tiles_per_slice : t_all;
    float m = -INFINITY, l = 0.0f;
    int64_t own_g = -1, oth_g[16];
    if (GROUPED)
        own_g = COLS ? dg[i < M ? i : M - 1] : qg[i < B ? i : B - 1];  // (a lane past the end: any label, its statistics are not written)
    const bool grouped_q = own_g >= 0;
    float tw = 0.0f, ts = 0.0f, tv[16];
    for (int t = t_begin + wave; t < n_tiles; t += 4) {
        const int j0 = t * IB_TILE;
        const f32x16 acc = ib_scores(COLS ? qh : dh, j0, COLS ? dh : qh, i0, Hp, lane, [&] {
            if (GROUPED)
                ib_labels(COLS ? qg : dg, j0, half, ND, oth_g);
            if (SOFT)
                ib_targets<true>(tg, i, B, j0, half, ND, M, tv);
        });
        float x[16], tm = -INFINITY;
        bool keep[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int j = j0 + ib_rho(r) + 4 * half;
            x[r] = acc[r] / temperature;
            keep[r] = j < ND;
            if (GROUPED && !COLS)  // (bitwise: one mask per pair, no branch per document)
                keep[r] = keep[r] & !(grouped_q & (oth_g[r] == own_g) & (j != i + pos_offset));
            if (GROUPED && COLS)   // (j is the walked query, i the own document)
                keep[r] = keep[r] & !((oth_g[r] >= 0) & (oth_g[r] == own_g) & (i != j + pos_offset));
            if (keep[r])
                tm = fmaxf(tm, x[r]);
            if (!SOFT && !COLS && j == i + pos_offset && i < B)
                pos[i] = x[r];  // (one lane of one wave of one slice, once)
            if (SOFT) {  // (a document past M: weight 0, and its score is that of a zero row: finite)
                const float tr = j < ND ? tv[r] : 0.0f;
                tw += tr;
                ts = fmaf(tr, x[r], ts);
            }
        }
        if (tm > -INFINITY) {  // (some document of the tile is valid, and kept, for this lane)
            const float mn = fmaxf(m, tm);
            float s = 0.0f;
#pragma unroll
            for (int r = 0; r < 16; ++r)
                if (keep[r])
                    s += expf(x[r] - mn);
            l = l * expf(m - mn) + s;  // (m = -inf: l = 0 and exp(-inf) = 0)
            m = mn;
        }
    }
    part_m[wave * 2 + half][lane & 31] = m;
    part_l[wave * 2 + half][lane & 31] = l;
    if (SOFT) {
        part_w[wave * 2 + half][lane & 31] = tw;
        part_t[wave * 2 + half][lane & 31] = ts;
    }
    __syncthreads();
    // (the row this thread writes: the query i0 + c, or the positive column of document i0 + c)
    const int out0 = COLS ? i0 - pos_offset : i0;
    if (threadIdx.x < IB_TILE && out0 + (int)threadIdx.x < B && (!COLS || out0 + (int)threadIdx.x >= 0)) {
        const int c = threadIdx.x;
        float M = -INFINITY;
        for (int k = 0; k < 8; ++k)
            M = fmaxf(M, part_m[k][c]);
        float L = 0.0f;
        for (int k = 0; k < 8; ++k)
            if (part_l[k][c] > 0.0f)
                L += part_l[k][c] * expf(part_m[k][c] - M);
        pm[(size_t)slice * Bq + out0 + c] = M;
        pl[(size_t)slice * Bq + out0 + c] = L;
        if (SOFT) {
            float W = 0.0f, T = 0.0f;
            for (int k = 0; k < 8; ++k) {
                W += part_w[k][c];
                T += part_t[k][c];
            }
            pw[(size_t)slice * Bq + out0 + c] = W;
            pt[(size_t)slice * Bq + out0 + c] = T;
        }
    }
}

// The symmetric loss's statistics in one grid: blocks [0, tiles_q * slices_q) are the row statistics (block = slice * tiles_q
// + tile), statement for statement ib_stats_kernel<GROUPED, false>; the rest are the column statistics of the document tiles
// tile_c0 .. tile_c0 + tiles_c - 1 (the aligned tiles that meet the positive columns), the same way.
template <bool GROUPED>
__global__ __launch_bounds__(256) void ib_sym_stats_kernel(const float *__restrict__ qh, const float *__restrict__ dh,
                                                           const int64_t *__restrict__ qg, const int64_t *__restrict__ dg, int B,
                                                           int M, int pos_offset, int Hp, int Bq, int tiles_per_slice,
                                                           int tiles_per_slice_c, float temperature, int tiles_q, int slices_q,
                                                           int tile_c0, int tiles_c, float *__restrict__ pm,
                                                           float *__restrict__ pl, float *__restrict__ pos,
                                                           float *__restrict__ cpm, float *__restrict__ cpl)
{
    int b = blockIdx.x;
    if (b < tiles_q * slices_q) {
        ib_stats_body<GROUPED, false, false>(qh, dh, qg, dg, B, M, pos_offset, Hp, Bq,
                                             tiles_per_slice, temperature, pm, pl, pos, nullptr, nullptr, nullptr, b % tiles_q,
                                             b / tiles_q);
    } else {
        b -= tiles_q * slices_q;
        ib_stats_body<GROUPED, false, true>(qh, dh, qg, dg, B, M, pos_offset, Hp, Bq,
                                            tiles_per_slice_c, temperature, cpm, cpl, nullptr, nullptr, nullptr, nullptr,
                                            tile_c0 + b % tiles_c, b / tiles_c);
    }
}

// The statistics launch of the *_ls entries, every variant in one 1-D grid laid out like ib_sym_stats_kernel's (!SYM: no column
// blocks): the temperature is the word the first launch stored, read here, and the bodies are the ones above.
template <bool GROUPED, bool SOFT, bool SYM>
__global__ __launch_bounds__(256) void ib_stats_ls_kernel(const float *__restrict__ qh, const float *__restrict__ dh,
                                                          const int64_t *__restrict__ qg, const int64_t *__restrict__ dg, int B,
                                                          int M, int pos_offset, int Hp, int Bq, int tiles_per_slice,
                                                          int tiles_per_slice_c, const float *__restrict__ tw, int tiles_q,
                                                          int slices_q, int tile_c0, int tiles_c, float *__restrict__ pm,
                                                          float *__restrict__ pl, float *__restrict__ pos,
                                                          float *__restrict__ cpm, float *__restrict__ cpl,
                                                          const float *__restrict__ tg, float *__restrict__ pw,
                                                          float *__restrict__ pt)
{
    const float temperature = tw[0];
    int b = blockIdx.x;
    if (!SYM || b < tiles_q * slices_q) {
        ib_stats_body<GROUPED, SOFT, false>(qh, dh, qg, dg, B, M, pos_offset, Hp, Bq, tiles_per_slice, temperature, pm, pl, pos,
                                            tg, pw, pt, b % tiles_q, b / tiles_q);
    } else {
        b -= tiles_q * slices_q;
        ib_stats_body<GROUPED, false, true>(qh, dh, qg, dg, B, M, pos_offset, Hp, Bq, tiles_per_slice_c, temperature, cpm, cpl,
                                            nullptr, nullptr, nullptr, nullptr, tile_c0 + b % tiles_c, b / tiles_c);
    }
}

// The slices' pairs of a query in ascending order -> lse_i and the row's loss lse_i - s_{i, pos_offset + i}.  The slice of the
// positive has a finite maximum, so M is finite; a slice that is empty for the query (grouped labels) comes as (-inf, 0) and
// adds 0 * exp(-inf - M) = 0 * 0.
// SOFT: the slices' (sum t, sum t s) in the same ascending order -> w_i and the row's loss
// w_i lse_i - sum_j t_ij s_ij; pos is not read.  (One-hot targets: w = 1.0f and the sum is s_pos, so this is lse - s_pos whether
// or not the product is fused into the subtraction.)
template <bool SOFT>
__global__ __launch_bounds__(256) void ib_lse_kernel(const float *__restrict__ pm, const float *__restrict__ pl,
                                                     const float *__restrict__ pos, int B, int Bq, int n_slices,
                                                     float *__restrict__ lse, float *__restrict__ row_loss,
                                                     const float *__restrict__ pw, const float *__restrict__ pt,
                                                     float *__restrict__ w)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= B)
        return;
    float m[IB_MAX_SLICES], l[IB_MAX_SLICES];  // (all slices asked for at once, combined in ascending order)
#pragma unroll
    for (int s = 0; s < IB_MAX_SLICES; ++s) {
        m[s] = s < n_slices ? pm[(size_t)s * Bq + i] : -INFINITY;
        l[s] = s < n_slices ? pl[(size_t)s * Bq + i] : 0.0f;
    }
    float M = -INFINITY;
#pragma unroll
    for (int s = 0; s < IB_MAX_SLICES; ++s)
        M = fmaxf(M, m[s]);
    float L = 0.0f;
#pragma unroll
    for (int s = 0; s < IB_MAX_SLICES; ++s)
        if (s < n_slices)
            L += l[s] * expf(m[s] - M);
    const float v = M + logf(L);
    lse[i] = v;
    if (SOFT) {
        float W = 0.0f, T = 0.0f;
        for (int s = 0; s < n_slices; ++s) {
            W += pw[(size_t)s * Bq + i];
            T += pt[(size_t)s * Bq + i];
        }
        w[i] = W;
        row_loss[i] = W * v - T;
        return;
    }
    row_loss[i] = v - pos[i];
}

// The fold of ib_lse_kernel<false>, statement for statement: the n_slices pairs of entry i in ascending order -> M + log L.
__device__ __forceinline__ float ib_fold(const float *__restrict__ pm, const float *__restrict__ pl, int i, int Bq, int n_slices)
{
    float m[IB_MAX_SLICES], l[IB_MAX_SLICES];
#pragma unroll
    for (int s = 0; s < IB_MAX_SLICES; ++s) {
        m[s] = s < n_slices ? pm[(size_t)s * Bq + i] : -INFINITY;
        l[s] = s < n_slices ? pl[(size_t)s * Bq + i] : 0.0f;
    }
    float M = -INFINITY;
#pragma unroll
    for (int s = 0; s < IB_MAX_SLICES; ++s)
        M = fmaxf(M, m[s]);
    float L = 0.0f;
#pragma unroll
    for (int s = 0; s < IB_MAX_SLICES; ++s)
        if (s < n_slices)
            L += l[s] * expf(m[s] - M);
    return M + logf(L);
}

// Symmetric: a thread per query i, which is also positive column i.  lse_i as above; clse_i from the column partials the same
// way (column i keeps the pair (i, P_i), so its maximum is finite too).  a = lse_i - s_pos and b = clse_i - s_pos are the two
// directions' row losses; the mixed one is (1 - alpha) a + alpha b: a itself at alpha = 0 (b is finite), b at alpha = 1.
__global__ __launch_bounds__(256) void ib_sym_lse_kernel(const float *__restrict__ pm, const float *__restrict__ pl,
                                                         const float *__restrict__ cpm, const float *__restrict__ cpl,
                                                         const float *__restrict__ pos, int B, int Bq, int n_slices,
                                                         int n_slices_c, float alpha, float *__restrict__ lse,
                                                         float *__restrict__ clse, float *__restrict__ row_loss,
                                                         float *__restrict__ row_qd, float *__restrict__ row_dq)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= B)
        return;
    const float v = ib_fold(pm, pl, i, Bq, n_slices), cv = ib_fold(cpm, cpl, i, Bq, n_slices_c);
    lse[i] = v;
    clse[i] = cv;
    const float a = v - pos[i], b = cv - pos[i];
    row_qd[i] = a;
    row_dq[i] = b;
    row_loss[i] = (1.0f - alpha) * a + alpha * b;
}

// ------------------------------------------------------------------ 5: gradients of the images
// QOWN: the workgroup owns 32 queries and walks a slice of the documents (dqh = G Dh); else it owns 32 documents and walks a
// slice of the queries (dDh = G^T qh).  Per chunk of 128 rows of the other side: each wave recomputes one S^T tile
// [other 32][owner 32], turns it into G and stores it to LDS [128][32]; then wave w accumulates the 32-column slices w, w + 4, ...
// of the owner rows' gradient, dXh^T [h 32][owner 32] += Other^T [h][128] G [128][owner] (A operand straight from the image,
// coalesced; B operand from LDS).  A chunk's product starts from zero and is added to the running total (blocked summation).
// The epilogue turns the [h][owner] accumulators into rows through LDS and stores the slice's partial [32][Hp] coalesced.
// GROUPED: G = 0 for an ignored pair, on either side; the owner row's label is loaded once, the walked rows' labels per tile
// behind the lse loads and the first operands of the products (ib_scores: after_first).
// SOFT: G = (w_i exp(s - lse_i) - t_ij) scale.  w is fetched with lse (the owner's once, the walked queries' per tile; w[] is
// padded like lse[]); the 16 targets of a tile are loaded where the labels are: along the own query's row on the query-owned
// side, down the own document's column (coalesced over the lanes) on the document-owned side.
// SYM (never SOFT): G = ((1 - alpha) (exp(s - lse_i) - onehot) + alpha [0 <= c < B] (exp(s - clse_c) - onehot)) scale with
// c = j - pos_offset.  clse[] is padded like lse[]; it is loaded at c clamped into [0, B) -- in bounds, unconditional, and
// what a document off the positive columns loads is replaced by 0 where it is used: the walked documents' 16 per tile on the
// query-owned side, behind the first operands of the products where the labels go; the own document's once on the other.
// The second exponential is evaluated for pairs in positive columns alone.
template <bool QOWN, bool GROUPED, bool SOFT, bool SYM = false>
__device__ __forceinline__ void ib_grad_body(float *ib_lds, const float *__restrict__ qh, const float *__restrict__ dh,
                                             const float *__restrict__ lse, const int64_t *__restrict__ qg,
                                             const int64_t *__restrict__ dg, const float *__restrict__ tg,
                                             const float *__restrict__ wq, int B, int M, int pos_offset, int Hp,
                                             float temperature, int tile, int chunk_begin, int chunk_end,
                                             float *__restrict__ part, const float *__restrict__ clse = nullptr,
                                             float alpha = 0.0f)
{
    // (the wave index as a scalar: the compiler then branches on it instead of masking lanes)
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), half = lane >> 5, col = lane & 31;
    const float *own = QOWN ? qh : dh, *oth = QOWN ? dh : qh;
    const int n_oth = QOWN ? M : B;
    const int own0 = tile * IB_TILE, o = own0 + col;
    const int NT = Hp / 32;
    const float scale = 1.0f / ((float)B * temperature);
    const float lse_own = (QOWN && o < B) ? lse[o] : 0.0f;
    const float w_own = (SOFT && QOWN && o < B) ? wq[o] : 0.0f;
    const int n_own = QOWN ? B : M;
    int64_t own_g = -1, oth_g[16];
    if (GROUPED)
        own_g = (QOWN ? qg : dg)[o < n_own ? o : n_own - 1];  // (an owner row past the end: any label, its pairs are out of range)
    float cl_own = 0.0f;
    if (SYM && !QOWN) {
        const int c = o - pos_offset;
        cl_own = clse[c < 0 ? 0 : (c < B ? c : B - 1)];
    }
    const float beta = 1.0f - alpha;
    f32x16 tot[4] = {};
    for (int ch = chunk_begin; ch < chunk_end; ++ch) {
        const int c0 = ch * IB_CHUNK, y0 = c0 + IB_TILE * wave;
        f32x16 g = {};
        if (y0 < n_oth) {  // (wave-uniform; a tile wholly past the end stores zeros)
            // the walked queries' lse, asked for before the products so that they arrive behind them (entries past B hold
            // anything and are not used; the array is padded like the images)
            float ls_y[16], w_y[16], tv[16], cl_y[16];
#pragma unroll
            for (int r = 0; r < 16; ++r)
                ls_y[r] = QOWN ? lse_own : lse[y0 + ib_rho(r) + 4 * half];
            if (SOFT)
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    w_y[r] = QOWN ? w_own : wq[y0 + ib_rho(r) + 4 * half];
            const f32x16 acc = ib_scores(oth, y0, own, own0, Hp, lane, [&] {
                if (GROUPED)
                    ib_labels(QOWN ? dg : qg, y0, half, n_oth, oth_g);
                if (SOFT)
                    ib_targets<QOWN>(tg, o, n_own, y0, half, n_oth, M, tv);
                if (SYM)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int c = y0 + ib_rho(r) + 4 * half - pos_offset;
                        cl_y[r] = QOWN ? clse[c < 0 ? 0 : (c < B ? c : B - 1)] : cl_own;
                    }
            });
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int y = y0 + ib_rho(r) + 4 * half;
                const int iq = QOWN ? o : y, jd = QOWN ? y : o;
                float v = 0.0f;
                if (iq < B && jd < M) {
                    const float ls = ls_y[r];
                    if (SOFT)
                        v = (w_y[r] * expf(acc[r] / temperature - ls) - tv[r]) * scale;
                    else if (SYM) {
                        const float x = acc[r] / temperature, hot = jd == iq + pos_offset ? 1.0f : 0.0f;
                        const float u = expf(x - ls) - hot;
                        float uc = 0.0f;
                        if (jd >= pos_offset && jd - pos_offset < B)
                            uc = expf(x - cl_y[r]) - hot;
                        v = (beta * u + alpha * uc) * scale;
                    } else
                        v = (expf(acc[r] / temperature - ls) - (jd == iq + pos_offset ? 1.0f : 0.0f)) * scale;
                    if (GROUPED) {
                        const int64_t gq = QOWN ? own_g : oth_g[r], gd = QOWN ? oth_g[r] : own_g;
                        v = ((gq >= 0) & (gd == gq) & (jd != iq + pos_offset)) ? 0.0f : v;  // (bitwise: a select, no branch)
                    }
                }
                g[r] = v;
            }
        }
#pragma unroll
        for (int r = 0; r < 16; ++r)
            ib_lds[(IB_TILE * wave + ib_rho(r) + 4 * half) * IB_TILE + col] = g[r];
        __syncthreads();
        f32x16 acc[4] = {};
        // (rows < Bq / Dp: the images are padded to whole chunks.)  Software-pipelined like ib_scores: the A operands of the next
        // 8 k-steps (16 rows of the chunk) are in flight while this batch's MFMAs issue.
        const float *ap = oth + (size_t)(c0 + half) * Hp + 32 * wave + col;
        float cur[IB_KB][4], nxt[IB_KB][4];
#pragma unroll
        for (int s = 0; s < IB_KB; ++s)
#pragma unroll
            for (int t = 0; t < 4; ++t)
                cur[s][t] = wave + 4 * t < NT ? ap[(size_t)(2 * s) * Hp + 128 * t] : 0.0f;
        for (int k = 0; k < IB_CHUNK; k += 2 * IB_KB) {
#pragma unroll
            for (int s = 0; s < IB_KB; ++s)
#pragma unroll
                for (int t = 0; t < 4; ++t)
                    nxt[s][t] = (k + 2 * IB_KB < IB_CHUNK && wave + 4 * t < NT) ? ap[(size_t)(k + 2 * IB_KB + 2 * s) * Hp + 128 * t] : 0.0f;
#pragma unroll
            for (int s = 0; s < IB_KB; ++s) {
                const float b = ib_lds[(k + 2 * s + half) * IB_TILE + col];
#pragma unroll
                for (int t = 0; t < 4; ++t)
                    if (wave + 4 * t < NT)
                        acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(cur[s][t], b, acc[t], 0, 0, 0);
            }
#pragma unroll
            for (int s = 0; s < IB_KB; ++s)
#pragma unroll
                for (int t = 0; t < 4; ++t)
                    cur[s][t] = nxt[s][t];
        }
#pragma unroll
        for (int t = 0; t < 4; ++t)
            tot[t] += acc[t];
        __syncthreads();  // (the next chunk, or the epilogue, overwrites G)
    }
    // gradient tile [owner 32][Hp], the columns of row c rotated by c so that the 32 lanes of a store hit 32 banks
#pragma unroll
    for (int t = 0; t < 4; ++t)
        if (wave + 4 * t < NT)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                int u = 32 * (wave + 4 * t) + ib_rho(r) + 4 * half + col;
                u = u >= Hp ? u - Hp : u;
                ib_lds[col * Hp + u] = tot[t][r];
            }
    __syncthreads();
    // (all 32 rows: the partial buffers are padded to whole chunks like the images; rows past the end hold zeros)
    for (int c = wave * 8; c < wave * 8 + 8; ++c) {
        const float *gt = ib_lds + c * Hp;
        float *out = part + (size_t)(own0 + c) * Hp;
        for (int u = lane; u < Hp; u += 64)
            out[u] = gt[u + c >= Hp ? u + c - Hp : u + c];
    }
}

// Blocks [0, tiles_q * slices_q): query tiles (block = slice * tiles_q + tile); the rest: document tiles, the same way.
template <bool GROUPED, bool SOFT>
__global__ __launch_bounds__(256) void ib_grad_kernel(const float *__restrict__ qh, const float *__restrict__ dh,
                                                      const float *__restrict__ lse, const int64_t *__restrict__ qg,
                                                      const int64_t *__restrict__ dg, int B, int M, int pos_offset, int Hp,
                                                      int Bq, int Dp, float temperature, int tiles_q, int slices_q, int per_q, int tiles_d,
                                                      int per_d, float *__restrict__ part_q, float *__restrict__ part_d,
                                                      const float *__restrict__ tg, const float *__restrict__ wq)
{
    extern __shared__ __attribute__((aligned(16))) float ib_lds[];  // G [128][32], later the gradient tile [32][Hp]
    int b = blockIdx.x;
    if (b < tiles_q * slices_q) {
        const int slice = b / tiles_q, chunks = (M + IB_CHUNK - 1) / IB_CHUNK;
        const int end = (slice + 1) * per_q < chunks ? (slice + 1) * per_q : chunks;
        ib_grad_body<true, GROUPED, SOFT>(ib_lds, qh, dh, lse, qg, dg, tg, wq, B, M, pos_offset, Hp, temperature, b % tiles_q, slice * per_q,
                                    end, part_q + (size_t)slice * Bq * Hp);
    } else {
        b -= tiles_q * slices_q;
        const int slice = b / tiles_d, chunks = (B + IB_CHUNK - 1) / IB_CHUNK;
        const int end = (slice + 1) * per_d < chunks ? (slice + 1) * per_d : chunks;
        ib_grad_body<false, GROUPED, SOFT>(ib_lds, qh, dh, lse, qg, dg, tg, wq, B, M, pos_offset, Hp, temperature, b % tiles_d, slice * per_d,
                                     end, part_d + (size_t)slice * Dp * Hp);
    }
}

// The symmetric loss's gradient launch: ib_grad_kernel's grid and slicing, the SYM bodies.
template <bool GROUPED>
__global__ __launch_bounds__(256) void ib_sym_grad_kernel(const float *__restrict__ qh, const float *__restrict__ dh,
                                                          const float *__restrict__ lse, const float *__restrict__ clse,
                                                          const int64_t *__restrict__ qg, const int64_t *__restrict__ dg, int B,
                                                          int M, int pos_offset, int Hp, int Bq, int Dp, float temperature,
                                                          float alpha, int tiles_q, int slices_q, int per_q, int tiles_d, int per_d,
                                                          float *__restrict__ part_q, float *__restrict__ part_d)
{
    extern __shared__ __attribute__((aligned(16))) float ib_lds[];  // G [128][32], later the gradient tile [32][Hp]
    int b = blockIdx.x;
    if (b < tiles_q * slices_q) {
        const int slice = b / tiles_q, chunks = (M + IB_CHUNK - 1) / IB_CHUNK;
        const int end = (slice + 1) * per_q < chunks ? (slice + 1) * per_q : chunks;
        ib_grad_body<true, GROUPED, false, true>(ib_lds, qh, dh, lse, qg, dg, nullptr, nullptr, B, M, pos_offset, Hp, temperature,
                                                 b % tiles_q, slice * per_q, end, part_q + (size_t)slice * Bq * Hp, clse, alpha);
    } else {
        b -= tiles_q * slices_q;
        const int slice = b / tiles_d, chunks = (B + IB_CHUNK - 1) / IB_CHUNK;
        const int end = (slice + 1) * per_d < chunks ? (slice + 1) * per_d : chunks;
        ib_grad_body<false, GROUPED, false, true>(ib_lds, qh, dh, lse, qg, dg, nullptr, nullptr, B, M, pos_offset, Hp, temperature,
                                                  b % tiles_d, slice * per_d, end, part_d + (size_t)slice * Dp * Hp, clse, alpha);
    }
}

// The gradient launch of the *_ls entries, every variant: ib_grad_kernel's grid and slicing, the temperature read from the word
// the first launch stored.
template <bool GROUPED, bool SOFT, bool SYM>
__global__ __launch_bounds__(256) void ib_grad_ls_kernel(const float *__restrict__ qh, const float *__restrict__ dh,
                                                         const float *__restrict__ lse, const float *__restrict__ clse,
                                                         const int64_t *__restrict__ qg, const int64_t *__restrict__ dg, int B,
                                                         int M, int pos_offset, int Hp, int Bq, int Dp,
                                                         const float *__restrict__ tw, float alpha, int tiles_q, int slices_q,
                                                         int per_q, int tiles_d, int per_d, float *__restrict__ part_q,
                                                         float *__restrict__ part_d, const float *__restrict__ tg,
                                                         const float *__restrict__ wq)
{
    extern __shared__ __attribute__((aligned(16))) float ib_lds[];  // G [128][32], later the gradient tile [32][Hp]
    const float temperature = tw[0];
    int b = blockIdx.x;
    if (b < tiles_q * slices_q) {
        const int slice = b / tiles_q, chunks = (M + IB_CHUNK - 1) / IB_CHUNK;
        const int end = (slice + 1) * per_q < chunks ? (slice + 1) * per_q : chunks;
        ib_grad_body<true, GROUPED, SOFT, SYM>(ib_lds, qh, dh, lse, qg, dg, tg, wq, B, M, pos_offset, Hp, temperature, b % tiles_q,
                                               slice * per_q, end, part_q + (size_t)slice * Bq * Hp, clse, alpha);
    } else {
        b -= tiles_q * slices_q;
        const int slice = b / tiles_d, chunks = (B + IB_CHUNK - 1) / IB_CHUNK;
        const int end = (slice + 1) * per_d < chunks ? (slice + 1) * per_d : chunks;
        ib_grad_body<false, GROUPED, SOFT, SYM>(ib_lds, qh, dh, lse, qg, dg, tg, wq, B, M, pos_offset, Hp, temperature, b % tiles_d,
                                                slice * per_d, end, part_d + (size_t)slice * Dp * Hp, clse, alpha);
    }
}

// ------------------------------------------------------------------ 6: through the norms
// One wave per row of [q; documents]: the slices' partials in ascending order -> dxh, then
// dx = (dxh - xh (xh . dxh)) / ||x||, or dxh / eps for a row shorter than eps: (dxh - flag xh (xh . dxh)) / max(||x||, eps).
__global__ __launch_bounds__(256) void ib_project_kernel(const float *__restrict__ qh, const float *__restrict__ dh,
                                                         const float *__restrict__ den, const float *__restrict__ flag,
                                                         const float *__restrict__ part_q, const float *__restrict__ part_d,
                                                         int B, int M, int H, int Hp, int Bq, int Dp, int slices_q,
                                                         int slices_d, float *__restrict__ dq, IBDocGrads dd)
{
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= B + M)
        return;
    const bool is_q = r < B;
    const int row = is_q ? r : r - B;  // row of the image
    const float *xh = (is_q ? qh : dh) + (size_t)row * Hp;
    const float *part = (is_q ? part_q : part_d) + (size_t)row * Hp;
    const size_t stride = (size_t)(is_q ? Bq : Dp) * Hp;
    const int ns = is_q ? slices_q : slices_d, nr = is_q ? row : Bq + row;
    float gv[IB_MAX_H / 64], dot = 0.0f;
#pragma unroll
    for (int e = 0; e < IB_MAX_H / 64; ++e) {
        const int u = lane + 64 * e;
        float g = 0.0f;
        if (u < Hp) {
            float v[IB_MAX_SLICES];  // (all slices asked for at once, added in ascending order)
#pragma unroll
            for (int s = 0; s < IB_MAX_SLICES; ++s)
                v[s] = s < ns ? part[s * stride + u] : 0.0f;
            g = v[0];
#pragma unroll
            for (int s = 1; s < IB_MAX_SLICES; ++s)
                if (s < ns)
                    g += v[s];
            dot += xh[u] * g;
        }
        gv[e] = g;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1)
        dot += __shfl_xor(dot, off);
    const float d = den[nr], f = flag[nr] * dot;
    float *out = is_q ? dq + (size_t)row * H : (row < dd.split ? dd.lo + (size_t)row * H : dd.hi + (size_t)(row - dd.split) * H);
#pragma unroll
    for (int e = 0; e < IB_MAX_H / 64; ++e) {
        const int u = lane + 64 * e;
        if (u < H)
            out[u] = (gv[e] - f * xh[u]) / d;
    }
}

// The *_ls entries with d_log_scale: ib_project_kernel's statements, one for one (the kernel above keeps its text, as
// ib_stats_kernel does: behind a shared function its registers change), and a query's wave also stores its xh . dxh =
// qh_i . dqh_i to dots[i] -- the row's share of dL/d(log 1/T) = sum_ij G_ij c_ij -- or, where the clamp of the scale holds
// gradient back (tw[1] == 0), +0.0f: a select per row, so that no NaN of a clamped call reaches the sum.
__global__ __launch_bounds__(256) void ib_project_dots_kernel(const float *__restrict__ qh, const float *__restrict__ dh,
                                                              const float *__restrict__ den, const float *__restrict__ flag,
                                                              const float *__restrict__ part_q,
                                                              const float *__restrict__ part_d, int B, int M, int H, int Hp,
                                                              int Bq, int Dp, int slices_q, int slices_d,
                                                              float *__restrict__ dq, IBDocGrads dd,
                                                              const float *__restrict__ tw, float *__restrict__ dots)
{
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= B + M)
        return;
    const bool is_q = r < B;
    const int row = is_q ? r : r - B;  // row of the image
    const float *xh = (is_q ? qh : dh) + (size_t)row * Hp;
    const float *part = (is_q ? part_q : part_d) + (size_t)row * Hp;
    const size_t stride = (size_t)(is_q ? Bq : Dp) * Hp;
    const int ns = is_q ? slices_q : slices_d, nr = is_q ? row : Bq + row;
    float gv[IB_MAX_H / 64], dot = 0.0f;
#pragma unroll
    for (int e = 0; e < IB_MAX_H / 64; ++e) {
        const int u = lane + 64 * e;
        float g = 0.0f;
        if (u < Hp) {
            float v[IB_MAX_SLICES];  // (all slices asked for at once, added in ascending order)
#pragma unroll
            for (int s = 0; s < IB_MAX_SLICES; ++s)
                v[s] = s < ns ? part[s * stride + u] : 0.0f;
            g = v[0];
#pragma unroll
            for (int s = 1; s < IB_MAX_SLICES; ++s)
                if (s < ns)
                    g += v[s];
            dot += xh[u] * g;
        }
        gv[e] = g;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1)
        dot += __shfl_xor(dot, off);
    if (is_q && lane == 0)
        dots[row] = tw[1] != 0.0f ? dot : 0.0f;
    const float d = den[nr], f = flag[nr] * dot;
    float *out = is_q ? dq + (size_t)row * H : (row < dd.split ? dd.lo + (size_t)row * H : dd.hi + (size_t)(row - dd.split) * H);
#pragma unroll
    for (int e = 0; e < IB_MAX_H / 64; ++e) {
        const int u = lane + 64 * e;
        if (u < H)
            out[u] = (gv[e] - f * xh[u]) / d;
    }
}

// Fixed-order sum of x[0..n) by one block -> out[0] * scale.
__global__ __launch_bounds__(1024) void ib_sum_kernel(const float *__restrict__ x, int n, float scale, float *__restrict__ out)
{
    __shared__ float red[16];
    float s = 0.0f;
    for (int i = threadIdx.x; i < n; i += 1024)
        s += x[i];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1)
        s += __shfl_xor(s, off);
    if ((threadIdx.x & 63) == 0)
        red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        float t = 0.0f;
        for (int w = 0; w < 16; ++w)
            t += red[w];
        out[0] = t * scale;
    }
}

// The device-resident scale of a *_ls call (null for the float entries): the word, its clamp, and where T and dL/dl go.
struct IBScale {
    const float *log_scale;
    float lo, hi;
    float *t_out, *d_out;  // nullable each
};

// Launches 1 and 6 of every entry.  ls: the first thread of launch 1 also forms T (P is then an ls plan); with ls->d_out,
// launch 6 also stores the row dots and one more ib_sum_kernel adds them, scale 1, in its fixed order.
void ib_launch_prep(const IBPlan &P, const float *q, IBDocs docs, int B, int M, int H, const IBScale *ls, char *ws, hipStream_t st)
{
    float *qh = (float *)(ws + P.qh), *dh = (float *)(ws + P.dh), *den = (float *)(ws + P.den), *flag = (float *)(ws + P.flag);
    if (ls)
        hipLaunchKernelGGL(ib_prep_ls_kernel, dim3((P.Bq + P.Dp + 3) / 4), dim3(256), 0, st, q, docs, B, M, H, P.Hp, P.Bq, P.Dp, qh,
                           dh, den, flag, ls->log_scale, ls->lo, ls->hi, (float *)(ws + P.tword), ls->t_out);
    else
        hipLaunchKernelGGL(ib_prep_kernel, dim3((P.Bq + P.Dp + 3) / 4), dim3(256), 0, st, q, docs, B, M, H, P.Hp, P.Bq, P.Dp, qh, dh,
                           den, flag);
}
void ib_launch_project(const IBPlan &P, int B, int M, int H, float *dq, IBDocGrads dd, const IBScale *ls, char *ws, hipStream_t st)
{
    const float *qh = (const float *)(ws + P.qh), *dh = (const float *)(ws + P.dh), *den = (const float *)(ws + P.den);
    const float *flag = (const float *)(ws + P.flag), *part_q = (const float *)(ws + P.part_q);
    const float *part_d = (const float *)(ws + P.part_d);
    const dim3 grid((unsigned)(((size_t)B + M + 3) / 4));
    if (ls && ls->d_out) {
        float *dots = (float *)(ws + P.dots);
        hipLaunchKernelGGL(ib_project_dots_kernel, grid, dim3(256), 0, st, qh, dh, den, flag, part_q, part_d, B, M, H, P.Hp, P.Bq,
                           P.Dp, P.sq.n, P.sd.n, dq, dd, (const float *)(ws + P.tword), dots);
        hipLaunchKernelGGL(ib_sum_kernel, dim3(1), dim3(1024), 0, st, (const float *)dots, B, 1.0f, ls->d_out);
    } else
        hipLaunchKernelGGL(ib_project_kernel, grid, dim3(256), 0, st, qh, dh, den, flag, part_q, part_d, B, M, H, P.Hp, P.Bq, P.Dp,
                           P.sq.n, P.sd.n, dq, dd);
}

// The launches of one call; the entries have refused what they refuse.  dd.lo == nullptr: the loss only.  qg == nullptr: no
// labels (the ungrouped instantiations); else qg [B], dg [M].  tg != nullptr: soft targets [B][M] (P is the soft plan, no labels,
// pos_offset unused).  ls != nullptr: `temperature` is unused, launches 2 and 5 are the *_ls_kernel forms.
void ib_launch(const IBPlan &P, const float *q, IBDocs docs, int B, int M, int H, int pos_offset, const int64_t *qg,
               const int64_t *dg, const float *tg, float temperature, float *loss, float *dq, IBDocGrads dd, void *workspace,
               hipStream_t st, const IBScale *ls = nullptr)
{
    char *ws = (char *)workspace;
    float *qh = (float *)(ws + P.qh), *dh = (float *)(ws + P.dh);
    float *lse = (float *)(ws + P.lse), *rows = (float *)(ws + P.rows);
    ib_launch_prep(P, q, docs, B, M, H, ls, ws, st);
    float *pm = (float *)(ws + P.pm), *pl = (float *)(ws + P.pl), *pos = (float *)(ws + P.pos);
    float *part_q = (float *)(ws + P.part_q), *part_d = (float *)(ws + P.part_d);
    const int tiles_q = (B + IB_TILE - 1) / IB_TILE, tiles_d = (M + IB_TILE - 1) / IB_TILE;
    float *pw = tg ? (float *)(ws + P.pw) : nullptr, *pt = tg ? (float *)(ws + P.pt) : nullptr;
    float *wq = tg ? (float *)(ws + P.w) : nullptr;
    const float *tw = (const float *)(ws + P.tword);
    if (ls) {
        const auto stats_kernel = tg   ? ib_stats_ls_kernel<false, true, false>
                                  : qg ? ib_stats_ls_kernel<true, false, false>
                                       : ib_stats_ls_kernel<false, false, false>;
        hipLaunchKernelGGL(stats_kernel, dim3(tiles_q * P.sq.n), dim3(256), 0, st, (const float *)qh, (const float *)dh, qg, dg, B,
                           M, pos_offset, P.Hp, P.Bq, P.sq.per * (IB_CHUNK / IB_TILE), 0, tw, tiles_q, P.sq.n, 0, 0, pm, pl, pos,
                           (float *)nullptr, (float *)nullptr, tg, pw, pt);
    } else {
        const auto stats_kernel = tg ? ib_stats_kernel<false, true> : qg ? ib_stats_kernel<true, false> : ib_stats_kernel<false, false>;
        hipLaunchKernelGGL(stats_kernel, dim3(tiles_q, P.sq.n), dim3(256), 0, st, (const float *)qh, (const float *)dh, qg, dg, B, M,
                           pos_offset, P.Hp, P.Bq, P.sq.per * (IB_CHUNK / IB_TILE), temperature, pm, pl, pos, tg, pw, pt);
    }
    hipLaunchKernelGGL(tg ? ib_lse_kernel<true> : ib_lse_kernel<false>, dim3((B + 255) / 256), dim3(256), 0, st, (const float *)pm, (const float *)pl,
                       (const float *)pos, B, P.Bq, P.sq.n, lse, rows, (const float *)pw, (const float *)pt, wq);
    hipLaunchKernelGGL(ib_sum_kernel, dim3(1), dim3(1024), 0, st, (const float *)rows, B, 1.0f / (float)B, loss);
    if (dq) {
        const size_t g_bytes = sizeof(float) * IB_CHUNK * IB_TILE, t_bytes = sizeof(float) * IB_TILE * (size_t)P.Hp;
        const size_t lds = g_bytes > t_bytes ? g_bytes : t_bytes;  // <= 64 KiB at H = 512
        const dim3 grid(tiles_q * P.sq.n + tiles_d * P.sd.n);
        if (ls) {
            const auto grad_kernel = tg   ? ib_grad_ls_kernel<false, true, false>
                                     : qg ? ib_grad_ls_kernel<true, false, false>
                                          : ib_grad_ls_kernel<false, false, false>;
            hipLaunchKernelGGL(grad_kernel, grid, dim3(256), lds, st, (const float *)qh, (const float *)dh, (const float *)lse,
                               (const float *)nullptr, qg, dg, B, M, pos_offset, P.Hp, P.Bq, P.Dp, tw, 0.0f, tiles_q, P.sq.n,
                               P.sq.per, tiles_d, P.sd.per, part_q, part_d, tg, (const float *)wq);
        } else {
            const auto grad_kernel = tg ? ib_grad_kernel<false, true> : qg ? ib_grad_kernel<true, false> : ib_grad_kernel<false, false>;
            hipLaunchKernelGGL(grad_kernel, grid, dim3(256), lds, st, (const float *)qh, (const float *)dh, (const float *)lse, qg, dg, B, M, pos_offset,
                               P.Hp, P.Bq, P.Dp, temperature, tiles_q, P.sq.n, P.sq.per, tiles_d, P.sd.per, part_q, part_d, tg, (const float *)wq);
        }
        ib_launch_project(P, B, M, H, dq, dd, ls, ws, st);
    }
}

// The launches of one symmetric call (P is the sym plan; the entry has refused what it refuses).  qg == nullptr: no labels.
// loss_dirs == nullptr: the two directions' means are not written (their row losses are).  ls as in ib_launch.
void ib_sym_launch(const IBPlan &P, const float *q, const float *docs, int B, int M, int H, int pos_offset, const int64_t *qg,
                   const int64_t *dg, float temperature, float alpha, float *loss, float *loss_dirs, float *dq, float *ddocs,
                   void *workspace, hipStream_t st, const IBScale *ls = nullptr)
{
    char *ws = (char *)workspace;
    float *qh = (float *)(ws + P.qh), *dh = (float *)(ws + P.dh);
    float *lse = (float *)(ws + P.lse), *rows = (float *)(ws + P.rows);
    float *pm = (float *)(ws + P.pm), *pl = (float *)(ws + P.pl), *pos = (float *)(ws + P.pos);
    float *part_q = (float *)(ws + P.part_q), *part_d = (float *)(ws + P.part_d);
    float *cpm = (float *)(ws + P.cpm), *cpl = (float *)(ws + P.cpl), *clse = (float *)(ws + P.clse);
    float *rows_qd = (float *)(ws + P.rows_qd), *rows_dq = (float *)(ws + P.rows_dq);
    const int tiles_q = (B + IB_TILE - 1) / IB_TILE, tiles_d = (M + IB_TILE - 1) / IB_TILE;
    // the aligned document tiles that meet the positive columns [pos_offset, pos_offset + B)
    const int tile_c0 = pos_offset / IB_TILE, tiles_c = (pos_offset + B - 1) / IB_TILE - tile_c0 + 1;
    const float *tw = (const float *)(ws + P.tword);
    ib_launch_prep(P, q, IBDocs{docs, nullptr, M}, B, M, H, ls, ws, st);
    const dim3 stats_grid(tiles_q * P.sq.n + tiles_c * P.sc.n);
    if (ls) {
        const auto stats_kernel = qg ? ib_stats_ls_kernel<true, false, true> : ib_stats_ls_kernel<false, false, true>;
        hipLaunchKernelGGL(stats_kernel, stats_grid,
                           dim3(256), 0, st, (const float *)qh, (const float *)dh, qg, dg, B, M, pos_offset, P.Hp, P.Bq,
                           P.sq.per * (IB_CHUNK / IB_TILE), P.sc.per * (IB_CHUNK / IB_TILE), tw, tiles_q, P.sq.n, tile_c0, tiles_c,
                           pm, pl, pos, cpm, cpl, (const float *)nullptr, (float *)nullptr, (float *)nullptr);
    } else
        hipLaunchKernelGGL(qg ? ib_sym_stats_kernel<true> : ib_sym_stats_kernel<false>, stats_grid,
                           dim3(256), 0, st, (const float *)qh, (const float *)dh, qg, dg, B, M, pos_offset, P.Hp, P.Bq,
                           P.sq.per * (IB_CHUNK / IB_TILE), P.sc.per * (IB_CHUNK / IB_TILE), temperature, tiles_q, P.sq.n, tile_c0,
                           tiles_c, pm, pl, pos, cpm, cpl);
    hipLaunchKernelGGL(ib_sym_lse_kernel, dim3((B + 255) / 256), dim3(256), 0, st, (const float *)pm, (const float *)pl,
                       (const float *)cpm, (const float *)cpl, (const float *)pos, B, P.Bq, P.sq.n, P.sc.n, alpha, lse, clse, rows,
                       rows_qd, rows_dq);
    hipLaunchKernelGGL(ib_sum_kernel, dim3(1), dim3(1024), 0, st, (const float *)rows, B, 1.0f / (float)B, loss);
    if (loss_dirs) {
        hipLaunchKernelGGL(ib_sum_kernel, dim3(1), dim3(1024), 0, st, (const float *)rows_qd, B, 1.0f / (float)B, loss_dirs);
        hipLaunchKernelGGL(ib_sum_kernel, dim3(1), dim3(1024), 0, st, (const float *)rows_dq, B, 1.0f / (float)B, loss_dirs + 1);
    }
    if (dq) {
        const size_t g_bytes = sizeof(float) * IB_CHUNK * IB_TILE, t_bytes = sizeof(float) * IB_TILE * (size_t)P.Hp;
        const size_t lds = g_bytes > t_bytes ? g_bytes : t_bytes;  // <= 64 KiB at H = 512
        const dim3 grid(tiles_q * P.sq.n + tiles_d * P.sd.n);
        if (ls) {
            const auto grad_kernel = qg ? ib_grad_ls_kernel<true, false, true> : ib_grad_ls_kernel<false, false, true>;
            hipLaunchKernelGGL(grad_kernel, grid, dim3(256),
                               lds, st, (const float *)qh, (const float *)dh, (const float *)lse, (const float *)clse, qg, dg, B, M,
                               pos_offset, P.Hp, P.Bq, P.Dp, tw, alpha, tiles_q, P.sq.n, P.sq.per, tiles_d, P.sd.per, part_q, part_d,
                               (const float *)nullptr, (const float *)nullptr);
        } else
            hipLaunchKernelGGL(qg ? ib_sym_grad_kernel<true> : ib_sym_grad_kernel<false>, grid,
                               dim3(256), lds, st, (const float *)qh, (const float *)dh, (const float *)lse, (const float *)clse, qg,
                               dg, B, M, pos_offset, P.Hp, P.Bq, P.Dp, temperature, alpha, tiles_q, P.sq.n, P.sq.per, tiles_d,
                               P.sd.per, part_q, part_d);
        ib_launch_project(P, B, M, H, dq, IBDocGrads{ddocs, nullptr, M}, ls, ws, st);
    }
}

constexpr int IB_MAX_B = 1 << 24, IB_MAX_M = 1 << 25;

bool ib_shape_ok(int B, int M, int H) { return B >= 1 && B <= IB_MAX_B && M >= B && M <= IB_MAX_M && H >= 1 && H <= IB_MAX_H; }

} // namespace

TT_EXPORT size_t tt_in_batch_loss_workspace_bytes(int B, int H)
{
    if (B < 1 || H < 1 || H > IB_MAX_H || B > IB_MAX_B)
        return 0;
    return ib_plan(B, 2 * B, H).total;
}

TT_EXPORT int tt_in_batch_loss_f32(const float *q, const float *p, const float *n, int B, int H, float temperature,
                                   float *loss, float *dq, float *dp, float *dn, void *workspace, size_t workspace_bytes,
                                   tt_stream_t stream)
{
    if (B < 1 || B > IB_MAX_B || H < 1 || H > IB_MAX_H)
        return tt_fail(TT_ERR_BAD_SHAPE, "tt_in_batch_loss_f32: B=%d H=%d (B >= 1, 1 <= H <= %d)", B, H, IB_MAX_H);
    if (!(temperature > 0.0f && temperature <= FLT_MAX))  // (NaN fails both comparisons)
        return tt_fail(TT_ERR_BAD_SHAPE, "tt_in_batch_loss_f32: temperature=%g must be finite and > 0", (double)temperature);
    if (!q || !p || !n || !loss || !workspace)
        return tt_fail(TT_ERR_BAD_SHAPE, "tt_in_batch_loss_f32: null pointer");
    if ((dq || dp || dn) && !(dq && dp && dn))
        return tt_fail(TT_ERR_BAD_SHAPE, "tt_in_batch_loss_f32: dq, dp, dn must be all null or all non-null");
    if ((uintptr_t)workspace & 15)
        return tt_fail(TT_ERR_BAD_SHAPE, "tt_in_batch_loss_f32: the workspace must be 16-byte aligned");
    const IBPlan P = ib_plan(B, 2 * B, H);
    if (workspace_bytes < P.total)
        return tt_fail(TT_ERR_BAD_SHAPE, "tt_in_batch_loss_f32: workspace %zu < %zu bytes", workspace_bytes, P.total);
    // D = [p; n]: the pool of M = 2B documents in two pieces, the positive of query i in row i
    ib_launch(P, q, IBDocs{p, n, B}, B, 2 * B, H, 0, nullptr, nullptr, nullptr, temperature, loss, dq, IBDocGrads{dp, dn, B}, workspace,
              (hipStream_t)stream);
    TT_LAUNCH_CHECK();
    return TT_OK;
}

namespace {

// The pool entries behind their names: `who` opens every message; grouped: the call brings labels (both non-null); soft: it
// brings targets [B][M] (non-null), no labels, and pos_offset 0.
int ib_pool_call(const char *who, bool grouped, bool soft, const float *q, int B, const float *docs, int M, int H, int pos_offset,
                 const int64_t *q_groups, const int64_t *doc_groups, const float *targets, float temperature, float *loss, float *dq, float *ddocs,
                 void *workspace, size_t workspace_bytes, tt_stream_t stream)
{
    if (!ib_shape_ok(B, M, H))
        return tt_fail(TT_ERR_BAD_SHAPE, "%s: B=%d M=%d H=%d (1 <= B <= %d, B <= M <= %d, 1 <= H <= %d)", who, B, M, H, IB_MAX_B,
                       IB_MAX_M, IB_MAX_H);
    if (pos_offset < 0 || pos_offset > M - B)
        return tt_fail(TT_ERR_BAD_SHAPE, "%s: pos_offset=%d outside [0, M - B = %d]", who, pos_offset, M - B);
    if (!(temperature > 0.0f && temperature <= FLT_MAX))  // (NaN fails both comparisons)
        return tt_fail(TT_ERR_BAD_SHAPE, "%s: temperature=%g must be finite and > 0", who, (double)temperature);
    if (!q || !docs || !loss || !workspace || (grouped && (!q_groups || !doc_groups)) || (soft && !targets))
        return tt_fail(TT_ERR_BAD_SHAPE, "%s: null pointer", who);
    if (!dq != !ddocs)
        return tt_fail(TT_ERR_BAD_SHAPE, "%s: dq, ddocs must be both null or both non-null", who);
    if ((uintptr_t)workspace & 15)
        return tt_fail(TT_ERR_BAD_SHAPE, "%s: the workspace must be 16-byte aligned", who);
    const IBPlan P = ib_plan(B, M, H, soft);
    if (workspace_bytes < P.total)
        return tt_fail(TT_ERR_BAD_SHAPE, "%s: workspace %zu < %zu bytes", who, workspace_bytes, P.total);
    ib_launch(P, q, IBDocs{docs, nullptr, M}, B, M, H, pos_offset, grouped ? q_groups : nullptr, grouped ? doc_groups : nullptr,
              soft ? targets : nullptr, temperature, loss, dq, IBDocGrads{ddocs, nullptr, M}, workspace, (hipStream_t)stream);
    TT_LAUNCH_CHECK();
    return TT_OK;
}

} // namespace

TT_EXPORT size_t tt_contrastive_loss_workspace_bytes(int B, int M, int H)
{
    return ib_shape_ok(B, M, H) ? ib_plan(B, M, H).total : 0;
}

TT_EXPORT int tt_contrastive_loss_f32(const float *q, int B, const float *docs, int M, int H, int pos_offset, float temperature,
                                      float *loss, float *dq, float *ddocs, void *workspace, size_t workspace_bytes,
                                      tt_stream_t stream)
{
    return ib_pool_call("tt_contrastive_loss_f32", false, false, q, B, docs, M, H, pos_offset, nullptr, nullptr, nullptr, temperature, loss, dq,
                        ddocs, workspace, workspace_bytes, stream);
}

TT_EXPORT int tt_contrastive_loss_grouped_f32(const float *q, int B, const float *docs, int M, int H, int pos_offset,
                                              const int64_t *q_groups, const int64_t *doc_groups, float temperature, float *loss,
                                              float *dq, float *ddocs, void *workspace, size_t workspace_bytes, tt_stream_t stream)
{
    return ib_pool_call("tt_contrastive_loss_grouped_f32", true, false, q, B, docs, M, H, pos_offset, q_groups, doc_groups, nullptr, temperature,
                        loss, dq, ddocs, workspace, workspace_bytes, stream);
}

TT_EXPORT size_t tt_contrastive_loss_soft_workspace_bytes(int B, int M, int H)
{
    return ib_shape_ok(B, M, H) ? ib_plan(B, M, H, true).total : 0;
}

TT_EXPORT int tt_contrastive_loss_soft_f32(const float *q, int B, const float *docs, int M, int H, const float *targets,
                                           float temperature, float *loss, float *dq, float *ddocs, void *workspace,
                                           size_t workspace_bytes, tt_stream_t stream)
{
    return ib_pool_call("tt_contrastive_loss_soft_f32", false, true, q, B, docs, M, H, 0, nullptr, nullptr, targets, temperature,
                        loss, dq, ddocs, workspace, workspace_bytes, stream);
}

TT_EXPORT size_t tt_contrastive_loss_sym_workspace_bytes(int B, int M, int H)
{
    return ib_shape_ok(B, M, H) ? ib_plan(B, M, H, false, true).total : 0;
}

TT_EXPORT int tt_contrastive_loss_sym_f32(const float *q, int B, const float *docs, int M, int H, int pos_offset,
                                          const int64_t *q_groups, const int64_t *doc_groups, float temperature, float alpha,
                                          float *loss, float *loss_dirs, float *dq, float *ddocs, void *workspace,
                                          size_t workspace_bytes, tt_stream_t stream)
{
    const char *who = "tt_contrastive_loss_sym_f32";
    if (!ib_shape_ok(B, M, H))
        return tt_fail(TT_ERR_BAD_SHAPE, "%s: B=%d M=%d H=%d (1 <= B <= %d, B <= M <= %d, 1 <= H <= %d)", who, B, M, H, IB_MAX_B,
                       IB_MAX_M, IB_MAX_H);
    if (pos_offset < 0 || pos_offset > M - B)
        return tt_fail(TT_ERR_BAD_SHAPE, "%s: pos_offset=%d outside [0, M - B = %d]", who, pos_offset, M - B);
    if (!(temperature > 0.0f && temperature <= FLT_MAX))  // (NaN fails both comparisons)
        return tt_fail(TT_ERR_BAD_SHAPE, "%s: temperature=%g must be finite and > 0", who, (double)temperature);
    if (!(alpha >= 0.0f && alpha <= 1.0f))  // (NaN fails both comparisons)
        return tt_fail(TT_ERR_BAD_SHAPE, "%s: alpha=%g outside [0, 1]", who, (double)alpha);
    if (!q_groups != !doc_groups)
        return tt_fail(TT_ERR_BAD_SHAPE, "%s: q_groups, doc_groups must be both null or both non-null", who);
    if (!q || !docs || !loss || !workspace)
        return tt_fail(TT_ERR_BAD_SHAPE, "%s: null pointer", who);
    if (!dq != !ddocs)
        return tt_fail(TT_ERR_BAD_SHAPE, "%s: dq, ddocs must be both null or both non-null", who);
    if ((uintptr_t)workspace & 15)
        return tt_fail(TT_ERR_BAD_SHAPE, "%s: the workspace must be 16-byte aligned", who);
    const IBPlan P = ib_plan(B, M, H, false, true);
    if (workspace_bytes < P.total)
        return tt_fail(TT_ERR_BAD_SHAPE, "%s: workspace %zu < %zu bytes", who, workspace_bytes, P.total);
    ib_sym_launch(P, q, docs, B, M, H, pos_offset, q_groups, doc_groups, temperature, alpha, loss, loss_dirs, dq, ddocs, workspace,
                  (hipStream_t)stream);
    TT_LAUNCH_CHECK();
    return TT_OK;
}

namespace {

// What the two *_ls entries refuse beyond their float entries' refusals.
int ib_scale_check(const char *who, const float *log_scale, float lo, float hi, const float *d_log_scale, const float *dq)
{
    if (!log_scale)
        return tt_fail(TT_ERR_BAD_SHAPE, "%s: null log_scale", who);
    if (!(lo >= -80.0f && hi <= 80.0f && lo <= hi))  // (NaN fails a comparison)
        return tt_fail(TT_ERR_BAD_SHAPE, "%s: log-scale bounds [%g, %g] must satisfy -80 <= min <= max <= 80", who, (double)lo,
                       (double)hi);
    if (d_log_scale && !dq)
        return tt_fail(TT_ERR_BAD_SHAPE, "%s: d_log_scale without dq", who);
    return TT_OK;
}

} // namespace

TT_EXPORT size_t tt_contrastive_loss_ls_workspace_bytes(int B, int M, int H, int soft)
{
    return ib_shape_ok(B, M, H) ? ib_plan(B, M, H, soft != 0, false, true).total : 0;
}

TT_EXPORT int tt_contrastive_loss_ls_f32(const float *q, int B, const float *docs, int M, int H, int pos_offset,
                                         const int64_t *q_groups, const int64_t *doc_groups, const float *targets,
                                         const float *log_scale, float min_log_scale, float max_log_scale, float *loss,
                                         float *temperature_out, float *d_log_scale, float *dq, float *ddocs, void *workspace,
                                         size_t workspace_bytes, tt_stream_t stream)
{
    const char *who = "tt_contrastive_loss_ls_f32";
    if (!ib_shape_ok(B, M, H))
        return tt_fail(TT_ERR_BAD_SHAPE, "%s: B=%d M=%d H=%d (1 <= B <= %d, B <= M <= %d, 1 <= H <= %d)", who, B, M, H, IB_MAX_B,
                       IB_MAX_M, IB_MAX_H);
    if (pos_offset < 0 || pos_offset > M - B)
        return tt_fail(TT_ERR_BAD_SHAPE, "%s: pos_offset=%d outside [0, M - B = %d]", who, pos_offset, M - B);
    if (!q_groups != !doc_groups)
        return tt_fail(TT_ERR_BAD_SHAPE, "%s: q_groups, doc_groups must be both null or both non-null", who);
    if (q_groups && targets)
        return tt_fail(TT_ERR_BAD_SHAPE, "%s: labels and targets exclude each other", who);
    if (!q || !docs || !loss || !workspace)
        return tt_fail(TT_ERR_BAD_SHAPE, "%s: null pointer", who);
    if (!dq != !ddocs)
        return tt_fail(TT_ERR_BAD_SHAPE, "%s: dq, ddocs must be both null or both non-null", who);
    if (const int rc = ib_scale_check(who, log_scale, min_log_scale, max_log_scale, d_log_scale, dq))
        return rc;
    if ((uintptr_t)workspace & 15)
        return tt_fail(TT_ERR_BAD_SHAPE, "%s: the workspace must be 16-byte aligned", who);
    const IBPlan P = ib_plan(B, M, H, targets != nullptr, false, true);
    if (workspace_bytes < P.total)
        return tt_fail(TT_ERR_BAD_SHAPE, "%s: workspace %zu < %zu bytes", who, workspace_bytes, P.total);
    const IBScale ls{log_scale, min_log_scale, max_log_scale, temperature_out, d_log_scale};
    ib_launch(P, q, IBDocs{docs, nullptr, M}, B, M, H, targets ? 0 : pos_offset, q_groups, doc_groups, targets, 0.0f, loss, dq,
              IBDocGrads{ddocs, nullptr, M}, workspace, (hipStream_t)stream, &ls);
    TT_LAUNCH_CHECK();
    return TT_OK;
}

TT_EXPORT size_t tt_contrastive_loss_sym_ls_workspace_bytes(int B, int M, int H)
{
    return ib_shape_ok(B, M, H) ? ib_plan(B, M, H, false, true, true).total : 0;
}

TT_EXPORT int tt_contrastive_loss_sym_ls_f32(const float *q, int B, const float *docs, int M, int H, int pos_offset,
                                             const int64_t *q_groups, const int64_t *doc_groups, const float *log_scale,
                                             float min_log_scale, float max_log_scale, float alpha, float *loss, float *loss_dirs,
                                             float *temperature_out, float *d_log_scale, float *dq, float *ddocs, void *workspace,
                                             size_t workspace_bytes, tt_stream_t stream)
{
    const char *who = "tt_contrastive_loss_sym_ls_f32";
    if (!ib_shape_ok(B, M, H))
        return tt_fail(TT_ERR_BAD_SHAPE, "%s: B=%d M=%d H=%d (1 <= B <= %d, B <= M <= %d, 1 <= H <= %d)", who, B, M, H, IB_MAX_B,
                       IB_MAX_M, IB_MAX_H);
    if (pos_offset < 0 || pos_offset > M - B)
        return tt_fail(TT_ERR_BAD_SHAPE, "%s: pos_offset=%d outside [0, M - B = %d]", who, pos_offset, M - B);
    if (!(alpha >= 0.0f && alpha <= 1.0f))  // (NaN fails both comparisons)
        return tt_fail(TT_ERR_BAD_SHAPE, "%s: alpha=%g outside [0, 1]", who, (double)alpha);
    if (!q_groups != !doc_groups)
        return tt_fail(TT_ERR_BAD_SHAPE, "%s: q_groups, doc_groups must be both null or both non-null", who);
    if (!q || !docs || !loss || !workspace)
        return tt_fail(TT_ERR_BAD_SHAPE, "%s: null pointer", who);
    if (!dq != !ddocs)
        return tt_fail(TT_ERR_BAD_SHAPE, "%s: dq, ddocs must be both null or both non-null", who);
    if (const int rc = ib_scale_check(who, log_scale, min_log_scale, max_log_scale, d_log_scale, dq))
        return rc;
    if ((uintptr_t)workspace & 15)
        return tt_fail(TT_ERR_BAD_SHAPE, "%s: the workspace must be 16-byte aligned", who);
    const IBPlan P = ib_plan(B, M, H, false, true, true);
    if (workspace_bytes < P.total)
        return tt_fail(TT_ERR_BAD_SHAPE, "%s: workspace %zu < %zu bytes", who, workspace_bytes, P.total);
    const IBScale ls{log_scale, min_log_scale, max_log_scale, temperature_out, d_log_scale};
    ib_sym_launch(P, q, docs, B, M, H, pos_offset, q_groups, doc_groups, 0.0f, alpha, loss, loss_dirs, dq, ddocs, workspace,
                  (hipStream_t)stream, &ls);
    TT_LAUNCH_CHECK();
    return TT_OK;
}
