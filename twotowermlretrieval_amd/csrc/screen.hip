// Screened exact top-k (gfx950): the path BruteForceIndex(screen=True) takes at every batch size.
//
// Exact fp32 scoring is bound by v_mfma_f32_32x32x2_f32 (157 TFLOP/s, 1/16 of the f16 MFMA rate).
// This path gets the SAME bit-exact result (oracle/tt_oracle.c:o_score_topk order and scores)
// through a rigorous filter:
//
//   1. screen   approximate scores s16 = <fp16(q), fp16(d)> with fp32 accumulation on
//               v_mfma_f32_16x16x32_f16 against an fp16 shadow copy of the corpus.  For every pair
//                   |s16 - s| <= eps_q  with  eps_q = 1.10e-3 |q| Dmax + 1e-6 (|q| + Dmax)
//               (fp16 rounding 2^-11 per operand, exact products, fp32 summation of 256 terms on
//               both sides, fp16 underflow; Dmax = largest document L2 norm; derivation in
//               DESIGN.md).  A document can be in the exact top-k only if
//               s16 >= A_k - 2 eps_q, where A_k is the k-th largest approximate score seen by
//               ANY subset of the corpus, so each workgroup keeps, per query, every candidate
//               within 2 eps_q of its running k-th best approximate score.
//   2. finish   per query: pool all candidates, A_k over the whole corpus, survivors
//               {s16 >= A_k - 2 eps_q}, EXACT fp32 FMA-chain rescoring of the survivors from the
//               fp32 corpus, exact top-k with (score desc, index asc).
//
// Anything that would break the guarantee (candidate buffer or survivor list overflow -- e.g.
// hundreds of near-duplicate documents around the k-th score --, |q| too large for fp16) raises a
// device flag; the caller then runs the plain exact kernel, predicated on that flag, so no host
// synchronisation is needed and the result is exact in every case.
//
// Three kernels share that scheme and the finish kernel:
//   q_image_kernel        once per search: queries -> f16 MFMA B-operand image, norms, initial flags
//   screen_kernel<.,NSET> B > 64: one workgroup (8 waves, one per CU) = 128 NSET queries x a contiguous chunk of
//                         documents; each wave keeps 16 NSET queries in registers; document tiles (32 docs x 256
//                         features f16 = 16 KiB) are DMA'd once per workgroup into an 8-deep LDS ring
//                         (global_load_lds, XOR-swizzled source) and read by all 8 waves
//   screen_stream_kernel  B <= 64: every wave an independent streaming engine (32 or 64 queries) with a private 4-slab ring; bound by
//                         HBM streaming of the fp16 copy (N * 512 B)
// The accumulators start at minus the query's threshold, so "any candidate in this wave-tile?" is one integer max.
//
// Seed.  A sample pass (the MAXONLY kernels over the first s_docs rows) gives the main pass its first threshold.  Streaming
// form: one maximum per 32-document sample tile, the seed is the k-th largest of them.  Shared-tile form (ONCHIP): the seed is
// the k-th largest of the KEPT SLICE MAXIMA.  A lane (n,g) of a wave holds, for a query, the scores of 8 documents of every
// tile -- rows 16u + 4g + r, a slice; the slices partition the sample -- and keeps the STOP = 2 largest slice maxima of its
// workgroup's tiles in registers (compare-and-swap on float order, entries start at -inf, rows at or beyond N and masked
// documents count as -inf).  Nothing is shuffled or stored in the tile loop; behind it every lane stores its STOP values
// once, [query][(chunk * 4 + g) * STOP + j], and the same select runs over those M = 4 STOP s_chunks <= 2048 values, from
// registers (the per-tile matrix was 4 883 values per query at 10M rows: 20 MB written, read back in four dependent passes).
// Validity: every kept value is the s16 of a document of its slice (the integer-max shortcut of full tiles still returns the
// score of a real document), different entries come from different slices, hence from different documents; so at least k
// distinct (kept) documents reach the k-th largest value of the union, which is all the A_k argument of step 1 uses.  With
// fewer than k finite values the select returns -inf and the floor threshold applies.  What the list can lose: when more than
// STOP of a query's k best slices meet in one of its 4 s_chunks streams (512 at B = 1024: about C(10,3) / 512^2 = 5e-4 per
// query at k = 10) the seed sits one rank lower -- a slightly weaker filter, never a wrong result; and slices are finer than
// tiles, so two of the k best in one tile now count twice (N = 1M, B = 1024, k = 10: 278.26 pooled candidates per query against
// 278.70, profiles/sample_onchip.md).  Below STOP_MIN_CHUNKS sample chunks (B beyond 2048 on 256 CUs) the per-tile maxima stay.
//
// Refresh (shared-tile main pass; SPlan::refresh: a seed, and chunks of REFRESH_MIN_TILES tiles or more).  Left alone every
// threshold stays at its seed for the whole pass: a workgroup sees N / n_chunks documents per query, fewer than the sample did,
// so its own running k-th never beats the seed, and at k = 10 12 % of the wave-tiles (48 % at k = 50) leave the fast path for
// candidates the finish kernel throws away.  The chip as a whole knows better: after a fraction f of the pass it has scored f N
// documents per query.  So every query has a LADDER of REFRESH_LEVELS counters in the workspace (ScreenParams::hist, zeroed by
// q_image_kernel), level j standing for the edge  e_j = base + (j - 1/4) w,  base = the query's initial threshold + 2 eps_q (the
// seed, whoever supplied it), w = REFRESH_STEP * 2 eps_q; every workgroup derives both from the same inputs.  The append path
// counts a lane's best stored candidate of a tile and query set, v >= base, at level min(L - 1, int((v - base) * (1 / w))) with
// one no-return atomic; at checkpoints T/32 .. T/2 into its own range of T tiles, and before every pool block, each wave reads
// its queries' ladders past the XCD's caches, sums them from the top level down, and raises the threshold to e_j - 2 eps_q for
// the highest level j whose suffix count reaches k (compaction raises with max as well; nothing ever lowers a threshold).
// Validity: every count is a distinct document of that query -- chunks and pool blocks partition the tiles, each (document,
// query) pair is scored once, and a lane counts at most one document per tile.  A count at level j' >= j means
// fl(fl(v - base) * fl(1 / w)) >= j, hence v - base >= j w (1 - 2^-20) >= (j - 1/8) w for j <= 15: three roundings of 2^-24 and a
// reciprocal within 2^-22 against a margin of w / 8, and the reader's fl(fma(j - 1/4, w, base)) lies below that by w / 8 less
// half an ulp of a score, thousands of times smaller than w >= 4e-6 (|q| + Dmax) (widths below 1e-30 count nothing).  So a
// suffix count >= k at level j means k distinct documents with s16 >= e_j: A_k >= e_j for that subset of the corpus, and
// every true top-k document has s16 >= e_j - 2 eps_q, the argument of step 1.  A stale view of the counters, candidates that a
// later compaction drops, documents a lane did not count (two candidates of one query among a lane's 8 documents of a tile)
// and visibility delays between XCDs only make the threshold lower, never wrong; no workgroup waits for another.  Under a
// keep-bitmask this is a fourth quantity formed from kept documents only: masked documents and rows at or beyond N are -inf
// before the append path sees them.  With lists of k = 50 seeded for k_seed = 10 (sharded search) the ladder is compared with
// p.k = 50: valid and conservative.  Results are bit-identical with and without; the pooled-candidate statistics depend on
// timing once the refresh is active, which is why the gate stays above the chunk lengths whose statistics tests compare.
// Measured (profiles/thr_refresh.md): 10M rows, B = 1024: 737 -> 98 pooled candidates per query at k = 10, 3669 -> 476 at
// k = 50; on 306-tile chunks (1.25M-row shard) the checkpoints cost more than they save, hence the gate.
//
// Under a keep-bitmask (MASKED instantiations; tt_score_topk_screened_masked_f32 and its kin).  Let K be the kept documents.
// A document's s16 and its exact score s depend on no other document, and |s16 - s| <= eps_q holds pair by pair; the
// guarantee of step 1 never uses tile or chunk boundaries.  Applied to the corpus D[K] it reads: a kept document can be in
// the exact top-k of K only if s16 >= A_k^K - 2 eps_q, A_k^K the k-th largest approximate score over any subset of K.  So it
// is enough that every quantity used as an A_k is formed from kept documents only.  There are three: (1) the sample maxima
// -- the seed is the k-th largest tile (shared-tile form: kept slice) maximum, "k distinct kept documents reach this", and a
// tile or slice with nothing kept contributes -inf; (2) the running k-th of a workgroup's candidate buffer (screen_compact); (3) the pooled A_k of
// screen_finish_kernel.  (2) and (3) see only what the append pass stored, so forcing a masked document's accumulators to
// -inf before either epilogue looks at them gives all three, with the finish kernel unchanged: the mechanism of the
// `partial` branch (rows at or beyond N), taken by every tile whose keep word is not all ones.  Masking the append pass
// alone would not do: a seed vouched for by documents that cannot be returned may exceed every kept score, and the main
// pass would then drop everything (tests/test_masked_screened_gpu.py, the plantings of test_threshold_passes_see_the_mask).
// The predicated fallback is the MASKED exact search.  A masked document is still streamed and multiplied.
#include "score_topk.h" // the predicated exact search (the fallback) and the threshold selections
#include "keep_word.h"  // the scalar load of a tile's keep word and its wait
#include <cmath>

#include <hip/hip_fp16.h>
#include <limits.h>
#include <math.h>

namespace {

typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef _Float16 h4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) void lds_void;
typedef const __attribute__((address_space(1))) void gbl_void;

#ifndef TT_SCREEN_STAGGER
#define TT_SCREEN_STAGGER 1
#endif
constexpr int SW = 8;                 // waves per workgroup
constexpr int STILE_BYTES = 32 * 512; // 32 docs x 256 f16
constexpr int SRING = 8;              // ring depth in tiles
constexpr int STPB = 2;               // tiles per barrier interval (waves drift freely inside one)
constexpr int SCAP = 128;             // candidate entries per (workgroup, query)
constexpr int SURV_MAX = 1024;        // survivors per query the finish kernel can rescore (256 until round 4: a cluster of ~200
                                      // near-duplicates plus a group of exact duplicates overflowed it, and on a clustered
                                      // corpus the predicated exact kernel then cost more than the screen saved: DESIGN K4s)
constexpr int POOL_MAX = 8192;        // candidates per query the finish kernel can pool
constexpr int FIN_MAX_CHUNKS = 2048;  // document chunks per query the finish kernel can pool
constexpr int STOP = 2;               // sample pass, shared-tile form: slice maxima a lane keeps per query (header, "Seed")
constexpr int STOP_MIN_CHUNKS = 64;   // ... when the sample has at least this many chunks (256 streams per query)
// Threshold refresh of the shared-tile main pass (header, "Refresh"): a ladder of REFRESH_LEVELS counters per query; a score
// v >= base is counted at level min(L - 1, floor((v - base) / w)), w = REFRESH_STEP * 2 eps_q, and level j stands for the edge
// base + (j - 1/4) w at the reader
constexpr int REFRESH_LEVELS = 16;       // four per lane (n,g): one 16-byte group of the query's ladder
constexpr int REFRESH_STEP = 2;          // level width in units of 2 eps_q
constexpr int REFRESH_FIRST_SHIFT = 5;   // checkpoints at T >> 5, T >> 4, .. T >> 1 tiles into a workgroup's own range of T tiles
constexpr int REFRESH_MIN_TILES = 1024;  // chunks shorter than this do not refresh (SPlan::refresh)

struct SCand {
    float v;
    int x;
};

// The derivation gives (2^-10 + 2^-22 + 2 * 1.53e-5 + threshold-in-accumulator terms) = 1.023e-3 (DESIGN 4 "K4s"); the worst
// input family the hardware test can build reaches 0.892 of 1.05e-3 (tests/test_screen_bound_gpu.py).  1.10e-3 leaves 7.5 % over
// the derivation instead of 2.6 %: a violation has no fallback (a true top-k document would be lost silently), and the
// wider slack costs about one more survivor per query.
__device__ __forceinline__ float screen_eps(float qnorm, float dmax)
{
    return 1.10e-3f * qnorm * dmax + 1e-6f * (qnorm + dmax);
}

// bf16 corpus (BF kernels): the LDS-DMA brings the bf16 rows -- the same 512 B per row, the same source swizzle -- and
// each wave converts the pieces it DMA'd itself, in place, once: bf16 -> fp32 (exact) -> fp16 with round-to-nearest-even,
// the cast build_from_bf16_kernel makes the fp16 shadow with, so the LDS image is the shadow's bit for bit.  NCH 16-byte
// chunks per lane at base + (i * 64 + lane) * 16; the caller waits for the DMA before and for lgkmcnt(0) after.
template <int NCH>
__device__ __forceinline__ void bf16_to_f16_lds(char *base, int lane)
{
    uint4 v[NCH];
#pragma unroll
    for (int i = 0; i < NCH; ++i)
        v[i] = *(const uint4 *)(base + (i * 64 + lane) * 16);
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
        unsigned w[4] = {v[i].x, v[i].y, v[i].z, v[i].w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const _Float16 lo = (_Float16)__uint_as_float(w[e] << 16);
            const _Float16 hi = (_Float16)__uint_as_float(w[e] & 0xffff0000u);
            w[e] = (unsigned)__builtin_bit_cast(unsigned short, lo) | ((unsigned)__builtin_bit_cast(unsigned short, hi) << 16);
        }
        *(uint4 *)(base + (i * 64 + lane) * 16) = uint4{w[0], w[1], w[2], w[3]};
    }
}

__device__ __forceinline__ SCand scand_load_l2(const SCand *p)
{
    unsigned long long u = __hip_atomic_load((const unsigned long long *)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    SCand c;
    c.v = __uint_as_float((unsigned)u);
    c.x = (int)(u >> 32);
    return c;
}

struct ScreenParams {
    // (the initialisers are the values of a launch that does not use the member; the host fills the rest: screen_params)
    const float *Q = nullptr;
    const _Float16 *D16 = nullptr;
    int B = 0, N = 0, k = 0;
    int n_chunks = 0, tiles_per_chunk = 0, n_tiles = 0;
    // Shared-tile main pass: tiles [0, static_tiles) are split evenly over the chunks; tiles [static_tiles, n_tiles) are a
    // POOL of tail_blocks blocks of tail_g tiles per query group that the workgroups draw from (tail_ctr[qgroup],
    // atomicAdd) once their own range is done.  static_tiles == n_tiles, tail_blocks == 0: everything static.
    int static_tiles = 0, tail_g = 1, tail_blocks = 0;
    int *tail_ctr = nullptr; // [n_qgroups], zeroed by q_image_kernel
    // Shared-tile main pass with a seed and long own ranges (SPlan::refresh), else null: hist[query][REFRESH_LEVELS], the chip-wide
    // count of stored candidates per threshold level, zeroed by q_image_kernel (Seeded phase: by the seed phase's, so one
    // seeded call per seed call on a workspace -- the contract tail_ctr already has, include/tt.h)
    unsigned *hist = nullptr;
    float dmax = 0.0f;
    SCand *cand = nullptr;   // [n_blocks][512][SCAP]
    int *pcnt = nullptr;     // [rows_pad][n_chunks]
    int *flag = nullptr;     // overflow / unsupported -> exact fallback
    // sample pass (MAXONLY): per-(tile, query) maximum approximate score
    float *max_val = nullptr;      // [rows_pad][n_tiles]
    // sample pass of the shared-tile form: instead of max_val, every lane's STOP largest slice maxima, stored once after the
    // last tile at top_val[query][(chunk * 4 + g) * STOP + j] (row stride n_chunks * 4 * STOP); null: per-tile maxima
    float *top_val = nullptr;
    const float *thr0 = nullptr;  // main pass: k-th largest sample maximum per query, stride thr0_stride (or null)
    int thr0_stride = 1;
    // queries as MFMA B operands, prepared once per search by q_image_kernel:
    // qimg[((S * 8 + s) * 64 + lane)] = 8 f16 of query 16 S + (lane & 15), features 32 s + 8 (lane >> 4) .. +7
    const h8 *qimg = nullptr;
    const float *qnorm = nullptr;  // |q| per (padded) query row
    // test-only (tt_debug_screen_s16): MAXONLY pass whose accumulators start at -dbg_thr[query] like the main
    // pass's, so the raw value t = fl(sum - thr) the filter compares with +0 can be observed; null in the product
    const float *dbg_thr = nullptr;
    // MASKED instantiations: keep-bitmask, one word per 32-document tile (bit n & 31 of word n >> 5 set -> document n of D16
    // may be returned; the sample pass reads the first words of the same mask); nullptr in every other launch
    const unsigned *keep = nullptr;
};

// store (v, x) at wave-uniform base + per-lane 32-bit byte offset (SGPR-base addressing: no 64-bit VALU math)
__device__ __forceinline__ void scand_store_async(const SCand *base, unsigned byte_off, float v, int x)
{
    const unsigned long long bits = ((unsigned long long)(unsigned)x << 32) | (unsigned long long)__float_as_uint(v);
    asm volatile("global_store_dwordx2 %0, %1, %2\n\ts_nop 1" ::"v"(byte_off), "v"(bits), "s"(base) : "memory");
}

// hist[...] += 1 at wave-uniform base + per-lane byte offset: no-return, agent scope (the encoding hipcc gives atomicAdd), and
// like the stores above invisible to the compiler's vmcnt bookkeeping
__device__ __forceinline__ void u32_inc_async(const unsigned *base, unsigned byte_off)
{
    asm volatile("global_atomic_add %0, %1, %2\n\ts_nop 0" ::"v"(byte_off), "v"(1u), "s"(base) : "memory");
}

// The ladder of a query (header, "Refresh"): the edge level j stands for at the reader, a quarter of a level below base + j w,
// and the level a stored score v >= base is counted at by the writer -- a count at level j or above implies v >= edge j with a
// margin of w / 8 over every rounding of the two expressions.
__device__ __forceinline__ float refresh_edge(int j, float width, float base) { return __fmaf_rn((float)j - 0.25f, width, base); }
__device__ __forceinline__ int refresh_level(float v, float base, float inv_width)
{
    return (int)fminf((v - base) * inv_width, (float)(REFRESH_LEVELS - 1)); // (clamped as a float: the product may exceed INT_MAX; NaN -> L - 1 never arises, v >= base is finite)
}
constexpr float REFRESH_MIN_WIDTH = 1e-30f;

__device__ __forceinline__ void f32_store_async(float *dst, float v)
{
    asm volatile("global_store_dword %0, %1, off\n\ts_nop 0" ::"v"(dst), "v"(v) : "memory");
}

// A query's 128-entry buffer is four 32-entry quarters, one per lane that holds scores of that query
// (16x16x32 MFMA: query n of a 16-query set sits in lanes n, n+16, n+32, n+48): lane (n,g) appends to
// quarter g with its OWN counter, so the append pass needs no cross-lane traffic at all.
// Compaction: keep every entry within `slack` of the k-th best of the union; rank r goes to quarter r&3,
// slot r>>2 (keeps the quarters balanced).  Lane t owns entries t and 64+t of the buffer.
constexpr int SQUART = SCAP / 4;                 // 32 entries per quarter
constexpr int SQ_TRIGGER = SQUART - 10;          // a tile adds at most 8 entries per lane: compact above this
constexpr int SQ_KEEP_MAX = 4 * SQ_TRIGGER - 4;  // more kept entries than this could not take another tile

__device__ __forceinline__ void screen_compact(SCand *base, const int (&n)[4], int k, float slack, int lane, int &n_new,
                                               float &thr_new, bool &have, bool &overflow)
{
    float v[2];
    int x[2], rank[2];
    bool live[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        v[i] = -INFINITY;
        x[i] = INT_MAX;
        rank[i] = 0;
        live[i] = (lane & 31) < ((lane >> 5) ? n[2 * i + 1] : n[2 * i]);
        if (live[i]) {
            const SCand c = scand_load_l2(base + 64 * i + lane);
            v[i] = c.v;
            x[i] = c.x;
        }
    }
#pragma unroll
    for (int i2 = 0; i2 < 2; ++i2) {
#pragma unroll
        for (int sub = 0; sub < 2; ++sub) {
            const int lim = n[2 * i2 + sub];
            for (int l2 = 0; l2 < lim; ++l2) {
                const float sv = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v[i2]), 32 * sub + l2));
                const int sx = __builtin_amdgcn_readlane(x[i2], 32 * sub + l2);
#pragma unroll
                for (int i = 0; i < 2; ++i)
                    rank[i] += (sv > v[i] || (sv == v[i] && sx < x[i])) ? 1 : 0;
            }
        }
    }
    const int total = n[0] + n[1] + n[2] + n[3];
    have = total >= k;
    overflow = false;
    n_new = total;
    thr_new = -INFINITY;
    if (have) {
        float kth = -INFINITY;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const unsigned long long bk = __ballot(live[i] && rank[i] == k - 1);
            if (bk)
                kth = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v[i]), __ffsll((long long)bk) - 1));
        }
        thr_new = kth - slack;
        n_new = 0;
#pragma unroll
        for (int i = 0; i < 2; ++i)
            n_new += __popcll(__ballot(live[i] && v[i] >= thr_new));
        if (n_new > SQ_KEEP_MAX) { // a quarter could not take one more tile: exact fallback (this pass's result is discarded)
            overflow = true;
            n_new = k;
        }
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
        if (live[i] && rank[i] < n_new) {
            SCand c;
            c.v = v[i];
            c.x = x[i];
            base[SQUART * (rank[i] & 3) + (rank[i] >> 2)] = c;
        }
}

// Once per search: the queries in the register image the screen kernels keep as MFMA B operands (one coalesced
// 1-KiB load per k-step and set instead of 64 scattered 16-byte row reads in every workgroup's prologue: the
// per-workgroup set-up was ~40 us of a 0.7 ms shard step, paid in the sample pass and again in the main pass),
// their norms, and the initial fallback flags (2 = fp16 cannot hold a query of this 32-query tile, else 0).
// One workgroup of two waves per 32-query tile, one wave per 16-query set; rows >= B read as zeros.
__global__ __launch_bounds__(128) void q_image_kernel(const float *__restrict__ Q, int B, h8 *__restrict__ img,
                                                      float *__restrict__ qnorm, int *__restrict__ flag, int n_flags,
                                                      int *__restrict__ tail_ctr, int n_ctr, unsigned *__restrict__ hist)
{
    __shared__ int any_bad[2];
    if (blockIdx.x == 0)
        for (int i = threadIdx.x; i < n_ctr; i += 128)
            tail_ctr[i] = 0;
    if (hist) // the ladders of this workgroup's 32 query rows (rows_pad = 32 gridDim.x)
        for (int i = threadIdx.x; i < 32 * REFRESH_LEVELS; i += 128)
            hist[(size_t)blockIdx.x * (32 * REFRESH_LEVELS) + i] = 0u;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int S = blockIdx.x * 2 + wv;
    const int g = lane >> 4, n = lane & 15;
    const int qrow = 16 * S + n;
    const bool live = qrow < B;
    const float *qp = Q + (size_t)min(qrow, B - 1) * 256 + 8 * g;
    float ss = 0.0f;
    bool bad = false;
#pragma unroll
    for (int s = 0; s < 8; ++s) {
        const f32x4 a = *(const f32x4 *)(qp + 32 * s);
        const f32x4 b = *(const f32x4 *)(qp + 32 * s + 4);
        h8 hv;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float x0 = live ? a[e] : 0.0f, x1 = live ? b[e] : 0.0f;
            ss += x0 * x0 + x1 * x1;
            bad |= !(fabsf(x0) <= 60000.0f) || !(fabsf(x1) <= 60000.0f);
            hv[e] = (_Float16)x0;
            hv[4 + e] = (_Float16)x1;
        }
        img[((size_t)S * 8 + s) * 64 + lane] = hv;
    }
    ss += __shfl_xor(ss, 16);
    ss += __shfl_xor(ss, 32);
    if (g == 0)
        qnorm[qrow] = sqrtf(ss);
    const bool wave_bad = __ballot(bad && live) != 0ull;
    if (lane == 0)
        any_bad[wv] = wave_bad ? 1 : 0;
    __syncthreads();
    if (threadIdx.x == 0 && (int)blockIdx.x < n_flags)
        flag[blockIdx.x] = (any_bad[0] | any_bad[1]) ? 2 : 0;
}

// NSET = 16-query sets per wave: 4 (512 queries per workgroup) for large batches; 2 / 1 (256 / 128 queries per
// workgroup) spread a mid-size batch over all eight waves instead of leaving most of them without queries; 3 (384 per
// workgroup, round 4) for the batches a 512-query group would leave a quarter or more empty: B = 257 .. 384 (one group) and
// 513 .. 768 (two groups of 384 instead of a full one and a nearly empty one -- a group costs a pass whatever it holds: B = 513
// took 3.6 ms where 512 took 2.1, profiles/r04_p_batch_sweep.log).
// MASKED: p.keep decides which documents may be returned.  A masked document is multiplied like any other and dropped in the
// epilogue (accumulators -> -inf, what `partial` does to the rows at or beyond N), in the main pass and in the sample pass
// alike; a tile whose word is 0 skips the append pass (every accumulator is -inf).  The word is wave-uniform and read by keep_word_issue under the
// tile's MFMAs -- never a compiler-visible global access in the tile loop, which would drain the DMA ring.
// ONCHIP (with MAXONLY; the product's sample pass): p.top_val instead of p.max_val.  A template mode because the run-time test
// cost screen_kernel<true, 4> -- 246 VGPRs without it -- 12 to 36 bytes of scratch per lane.
template <bool MAXONLY, int NSET, bool BF = false, bool MASKED = false, bool ONCHIP = false>
__global__ __launch_bounds__(SW * 64, 2) void screen_kernel(ScreenParams p)
{
    extern __shared__ __attribute__((aligned(16))) char ring[]; // [SRING][STILE_BYTES]
    // NSET < 4 (B <= 256): one query group, so every tile is read once by one workgroup: nt policy like the streaming
    // form (TSTREAM_AUX; here -2.5 % at B = 33 .. 128, -1.5 % at 256, A/B on one box); NSET == 4 may have two groups per
    // chunk that share the tile through L2: default policy
    constexpr int DMA_AUX = NSET < 3 ? 2 : 0;
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int chunk = blockIdx.x % p.n_chunks;
    const int qgroup = blockIdx.x / p.n_chunks;
    int t0 = chunk * p.tiles_per_chunk;                   // this workgroup's own range first, then blocks of the pool
    int t1 = min(t0 + p.tiles_per_chunk, p.static_tiles);
    __shared__ int next_block;
    const int k = p.k;
    const int g = lane >> 4, n = lane & 15;
    constexpr int QW = 16 * NSET, QB = SW * QW; // queries per wave / per workgroup
    const int qbase = qgroup * QB + w * QW;
    const bool wave_live = qbase < p.B;
    // Refresh (main pass, p.hist): the ladder's base per query of this workgroup = its initial threshold + 2 eps_q, the seed
    // whoever supplied it -- every workgroup derives it from the same inputs.  In LDS: the kernel has no register to spare.
    __shared__ float ladder_base[SW * 64];
    const bool refresh = !MAXONLY && p.hist != nullptr;
    const unsigned *const hwave = p.hist + (size_t)qbase * REFRESH_LEVELS;

    // ---- query operands (B of v_mfma_f32_16x16x32_f16): set c holds queries qbase + 16c + n;
    //      lane (n,g) keeps features 32s + 8g .. +7 of k-step s ----
    // Main pass: the accumulators start at -thr (the MFMA's C operand of the first k-step is negthr[c]), so a
    // score passes its query's threshold iff its sign bit is clear and ONE integer max over a wave-tile's 32
    // accumulator registers decides whether anything in the tile needs a second look.  thr is always finite:
    // without a seed it is a lower bound of every possible score, -(1.01 |q| Dmax).
    h8 qreg[NSET][8];
    float eps2[NSET];
    f32x4 negthr[NSET];
    int cnt[NSET];
#pragma unroll
    for (int c = 0; c < NSET; ++c)
        cnt[c] = 0;
#pragma unroll
    for (int c = 0; c < NSET; ++c) {
        const int qrow = qbase + 16 * c + n;
        const bool live = qrow < p.B;
        float qn = 0.0f;
        if (wave_live) { // (a wave without queries only helps with the DMA)
            const h8 *src = p.qimg + ((size_t)(qbase / 16 + c) * 8) * 64 + lane;
#pragma unroll
            for (int s = 0; s < 8; ++s)
                qreg[c][s] = src[s * 64];
            qn = p.qnorm[qrow];
        }
        eps2[c] = 2.0f * screen_eps(qn, p.dmax);
        // A_k over any subset of the corpus, minus 2 eps, never exceeds the approximate score of a
        // true top-k document: the sample pass's k-th largest maximum seeds the threshold.
        const float floor_thr = -(1.01f * qn * p.dmax + 1e-30f);
        const float t_init = live ? ((!MAXONLY && p.thr0) ? fmaxf(p.thr0[(size_t)qrow * p.thr0_stride + p.thr0_stride - 1] - eps2[c], floor_thr)
                                                    : floor_thr)
                            : INFINITY; // dead query rows: accumulators stay at -inf, never a candidate
        float c_init = -t_init;
        if (MAXONLY) // sample pass: plain scores (C = +0); the debug export may plant a threshold instead
            c_init = (p.dbg_thr && live) ? -p.dbg_thr[qrow] : 0.0f;
        negthr[c] = f32x4{c_init, c_init, c_init, c_init};
        if (!MAXONLY && g == 0) // (dead rows: +inf, no score reaches it; read behind the first tile's barrier at the earliest)
            ladder_base[w * QW + 16 * c + n] = t_init + eps2[c];
    }

    SCand *const cwave = p.cand + ((size_t)blockIdx.x * QB + w * QW) * SCAP;

    auto compact_where = [&](int c, unsigned qmask) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        while (qmask) {
            const int q = __ffs((int)qmask) - 1;
            qmask &= qmask - 1;
            const int nq[4] = {__builtin_amdgcn_readlane(cnt[c], q), __builtin_amdgcn_readlane(cnt[c], q + 16),
                               __builtin_amdgcn_readlane(cnt[c], q + 32), __builtin_amdgcn_readlane(cnt[c], q + 48)};
            const float slack = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, eps2[c]), q));
            int n_new;
            float tn;
            bool have, ovf;
            screen_compact(cwave + (size_t)(16 * c + q) * SCAP, nq, k, slack, lane, n_new, tn, have, ovf);
            if (ovf && lane == 0)
                atomicOr(p.flag + ((qbase + 16 * c) >> 5), 1);
            if (n == q) {
                cnt[c] = (n_new - g + 3) >> 2; // ranks r < n_new with r & 3 == g
                if (have) { // raise, never overwrite: a refresh may already have put the threshold above this workgroup's own k-th
                    const float nt = fminf(negthr[c][0], -tn);
                    negthr[c] = f32x4{nt, nt, nt, nt};
                }
            }
        }
    };

    // Refresh: each lane (n,g) reads levels 4g .. 4g+3 of its queries' ladders (agent scope: past the XCD's own caches), forms
    // the suffix counts from the top level down, and the query's threshold rises to the edge of the highest level that k stored
    // candidates have reached, minus 2 eps_q.  A cold branch like compact_where: drain, then plain code.  The caller holds no
    // accumulator computed under the old threshold (the epilogue forms v = acc + thr).
    auto refresh_thresholds = [&]() {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        // (the lane index passes through an empty asm so that the addresses below are formed here, in the cold branch, and
        //  not hoisted into registers that would live across the tile loop: screen_kernel<false, 4> has none to spare)
        int ln = lane;
        asm volatile("" : "+v"(ln));
        const int n = ln & 15, g = ln >> 4;
#pragma unroll
        for (int c = 0; c < NSET; ++c) {
            const unsigned *hp = hwave + (unsigned)((16 * c + n) * REFRESH_LEVELS + 4 * g);
            int sfx[4]; // sfx[i]: candidates at levels >= 4g + i
            int run = 0;
#pragma unroll
            for (int i = 3; i >= 0; --i) {
                run += (int)__hip_atomic_load(hp + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                sfx[i] = run;
            }
            const int x16 = (ln ^ 16) << 2, x32 = (ln ^ 32) << 2; // (ds_bpermute addresses, formed here for the same reason)
            const int t16 = __builtin_amdgcn_ds_bpermute(x16, run), t32 = __builtin_amdgcn_ds_bpermute(x32, run),
                      t48 = __builtin_amdgcn_ds_bpermute(x32, t16); // the totals of lanes g^1, g^2, g^3
            const int above = ((g ^ 1) > g ? t16 : 0) + ((g ^ 2) > g ? t32 : 0) + ((g ^ 3) > g ? t48 : 0);
            int jtop = -1;
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (above + sfx[i] >= k)
                    jtop = 4 * g + i;
            jtop = max(jtop, __builtin_amdgcn_ds_bpermute(x16, jtop));
            jtop = max(jtop, __builtin_amdgcn_ds_bpermute(x32, jtop));
            if (jtop > 0) { // (level 0 is the initial threshold itself)
                const float base = ladder_base[w * QW + 16 * c + n];
                float le = eps2[c];
                asm volatile("" : "+v"(le));
                const float nt = fminf(negthr[c][0], le - refresh_edge(jtop, (float)REFRESH_STEP * le, base));
                negthr[c] = f32x4{nt, nt, nt, nt};
            }
            __builtin_amdgcn_sched_barrier(0); // one set at a time: its loads and sums are not hoisted over the previous set's
        }
    };

    // ---- DMA: tile = 16 wave-instructions of 1 KiB (2 docs x 512 B); wave w issues 2w, 2w+1 ----
    const char *D = (const char *)p.D16;
    const char *rowp[2];
    auto set_rows = [&](int tile) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int row = 2 * (2 * w + i) + (lane >> 5);  // doc within the tile
            const int doc = min(tile * 32 + row, p.N - 1);
            const int chunk16 = (lane & 31) ^ (row & 15);   // source swizzle: logical = physical ^ (row & 15)
            rowp[i] = D + (size_t)doc * 512 + chunk16 * 16;
        }
    };
    auto dma_issue = [&](int tile, int stage) {
        set_rows(min(tile, t1 - 1));
        char *dst = ring + stage * STILE_BYTES + (2 * w) * 1024;
        __builtin_amdgcn_global_load_lds((gbl_void *)rowp[0], (lds_void *)dst, 16, 0, DMA_AUX);
        __builtin_amdgcn_global_load_lds((gbl_void *)rowp[1], (lds_void *)(dst + 1024), 16, 0, DMA_AUX);
    };
    // one of a tile's two pieces (the addresses were prepared by set_rows)
    auto dma_piece = [&](int i, int stage) {
        char *dst = ring + stage * STILE_BYTES + (2 * w + i) * 1024;
        __builtin_amdgcn_global_load_lds((gbl_void *)rowp[i], (lds_void *)dst, 16, 0, DMA_AUX);
    };

    // ONCHIP: lane (n,g) sees, for query set c, the scores of 8 documents of every
    // tile (rows 16u + 4g + r: a SLICE) and keeps the STOP largest slice maxima of its workgroup's tiles here, best first.  No
    // shuffle and no store in the tile loop; one store per lane behind it.
    float top[ONCHIP ? NSET : 1][STOP];
#pragma unroll
    for (int c = 0; c < (ONCHIP ? NSET : 1); ++c)
#pragma unroll
        for (int j = 0; j < STOP; ++j)
            top[c][j] = -INFINITY;

    for (;;) { // segments: the own range, then pool blocks
    if (t0 < t1) {
        // DMA runs SRING - STPB tiles ahead; one barrier per STPB tiles.
#pragma unroll
        for (int gi = 0; gi < SRING - STPB; ++gi)
            dma_issue(t0 + gi, gi);
        int stage = 0;
        const int rd_base = n * 512; // A row (document) n of sub-tile 0; sub-tile 1 is 16 rows = 8 KiB further
        // acc[u][c][r] = s16(doc tile*32 + 16u + 4g + r, query qbase + 16c + n) (main pass: minus the query's threshold)
        f32x4 acc[2][NSET];
        // Stagger: all eight waves run the same program between the same barriers, so left alone the two waves of a SIMD
        // reach their MFMA block, their LDS reads and their selection epilogue together.  Waves 4-7 (the second wave of
        // each SIMD) therefore DEFER a tile's selection until after the next tile iteration has started -- their
        // accumulators stay in registers across the barrier -- so that one half selects (VALU, stores) while the other
        // multiplies (MI355X_MICROARCH.md, "Two waves per SIMD", item 9).  Same work, same results, shifted by one phase.
        const bool late = TT_SCREEN_STAGGER && w >= 4;
        bool pending = false;
        int ptile = 0;
        unsigned pkw = 0xffffffffu; // MASKED: the deferred tile's keep word travels with its accumulators
        // kw: the tile's keep word (MASKED; landed: keep_word_wait ran behind the tile's MFMAs)
        auto epilogue = [&](int tile, unsigned kw) {
                const int tile_base = tile * 32;
            const bool partial = tile_base + 32 > p.N;
            // MASKED: a word that is not all ones makes the tile partial in the same sense; bit 16u + r of kwg = the keep bit of
            // the lane's document (u, r) = row 16u + 4g + r (bits at or beyond N: the doc < N test stays)
            const bool holes = MASKED && kw != 0xffffffffu;
            const unsigned kwg = MASKED ? kw >> (4 * g) : 0xffffffffu;
            auto dropped = [&](int u, int r) {
                return tile_base + 16 * u + 4 * g + r >= p.N || (MASKED && ((kwg >> (16 * u + r)) & 1u) == 0u);
            };
            if (!MAXONLY) {
                // rows past the corpus (and masked documents) never pass: -inf has its sign bit set.  (A word of 0 leaves
                // nothing but -inf, so the gate below skips the append pass; a branch of its own around the epilogue cost
                // screen_kernel<., 4> -- at the 256-VGPR limit -- a spilled register)
                if (partial || holes) {
#pragma unroll
                    for (int u = 0; u < 2; ++u)
#pragma unroll
                        for (int r = 0; r < 4; ++r)
                            if (dropped(u, r)) {
#pragma unroll
                                for (int c = 0; c < NSET; ++c)
                                    acc[u][c][r] = -INFINITY;
                            }
                }
                // any score at or above its threshold <=> some accumulator has a clear sign bit
                // <=> the signed-integer maximum of the raw registers is >= 0
                int mall = INT_MIN;
#pragma unroll
                for (int u = 0; u < 2; ++u)
#pragma unroll
                    for (int c = 0; c < NSET; ++c)
#pragma unroll
                        for (int r = 0; r < 4; ++r)
                            mall = max(mall, __float_as_int(acc[u][c][r]));
                if (__ballot(mall >= 0) != 0ull) {
#pragma unroll
                    for (int c = 0; c < NSET; ++c) {
                        int mu[2];
#pragma unroll
                        for (int u = 0; u < 2; ++u)
                            mu[u] = max(max(__float_as_int(acc[u][c][0]), __float_as_int(acc[u][c][1])),
                                        max(__float_as_int(acc[u][c][2]), __float_as_int(acc[u][c][3])));
                        if (__ballot(max(mu[0], mu[1]) >= 0) == 0ull)
                            continue;
                        // append pass: every lane appends to its own quarter of the query's buffer with its
                        // own counter (no ballots), through inline-asm stores (a compiler-visible VMEM op here
                        // would put s_waitcnt vmcnt(0) on the hot path and drain the DMA ring)
                        const unsigned mine = (unsigned)(((16 * c + n) * SCAP + SQUART * g) * sizeof(SCand));
                        const float thr_c = -negthr[c][0];
#pragma unroll
                        for (int u = 0; u < 2; ++u) {
                            if (__ballot(mu[u] >= 0) == 0ull)
                                continue;
#pragma unroll
                            for (int r = 0; r < 4; ++r) {
                                if (__float_as_int(acc[u][c][r]) >= 0) {
                                    scand_store_async(cwave, mine + (unsigned)cnt[c] * (unsigned)sizeof(SCand),
                                                      acc[u][c][r] + thr_c, tile_base + 16 * u + 4 * g + r);
                                    ++cnt[c];
                                }
                            }
                        }
                        // Refresh: count the lane's best candidate of this tile and set on the query's ladder.  (One per lane
                        // and tile, not one per candidate: two candidates of one query among a lane's 8 documents of a tile are
                        // rare, a document left out only makes the count -- and the threshold -- lower, and the count runs
                        // here, behind the stores, where their operands are dead: the kernel has no register to spare.  The
                        // raw maximum of non-negative accumulators is their float maximum, as in the gate above.)
                        if (refresh) {
                            const int mbest = max(mu[0], mu[1]);
                            if (mbest >= 0) {
                                int lq = n; // (through an empty asm: the addresses and the level width are formed in this
                                float le = eps2[c]; // branch and not kept per set across the tile loop, see refresh_thresholds)
                                asm volatile("" : "+v"(lq), "+v"(le));
                                lq += 16 * c;
                                const float lwidth = (float)REFRESH_STEP * le;
                                const float lbase = ladder_base[w * QW + lq];
                                const float v = __int_as_float(mbest) + thr_c;
                                if (lwidth >= REFRESH_MIN_WIDTH && v >= lbase)
                                    u32_inc_async(hwave, (unsigned)((lq * REFRESH_LEVELS + refresh_level(v, lbase, 1.0f / lwidth)) * sizeof(unsigned)));
                            }
                        }
                        unsigned long long full = __ballot(cnt[c] > SQ_TRIGGER);
                        full = (full | (full >> 32));
                        full = (full | (full >> 16)) & 0xffffull;
                        if (full)
                            compact_where(c, (unsigned)full);
                    }
                }
            } else {
#pragma unroll
                for (int c = 0; c < NSET; ++c) { // one maximum per (tile, query), or per (slice, query) into the lane's list (ONCHIP)
                    float m = -INFINITY;
                    if (!partial && !holes) {
                        // signed-integer max of the raw bits = the float max when any value is >= 0, else the
                        // smallest one: still the score of a real document of this tile, which is all the
                        // threshold argument needs (v_max3_i32: no NaN canonicalisation, 4 instructions).
                        // (MASKED: valid for an all-ones word only -- "a real document" has to be a kept one)
                        int mi = INT_MIN;
#pragma unroll
                        for (int u = 0; u < 2; ++u)
#pragma unroll
                            for (int r = 0; r < 4; ++r)
                                mi = max(mi, __float_as_int(acc[u][c][r]));
                        m = __int_as_float(mi);
                    } else {
#pragma unroll
                        for (int u = 0; u < 2; ++u)
#pragma unroll
                            for (int r = 0; r < 4; ++r)
                                m = fmaxf(m, !dropped(u, r) ? acc[u][c][r] : -INFINITY);
                    }
                    if (ONCHIP) { // m = this slice's maximum: compare-and-swap into the lane's list
#pragma unroll
                        for (int j = 0; j < STOP; ++j) {
                            float &t = top[ONCHIP ? c : 0][j];
                            const float hi = fmaxf(t, m);
                            m = fminf(t, m);
                            t = hi;
                        }
                        continue;
                    }
                    m = fmaxf(m, __shfl_xor(m, 16));
                    m = fmaxf(m, __shfl_xor(m, 32));
                    const int qrow = qbase + 16 * c + n;
                    if (g == 0 && qrow < p.B)
                        f32_store_async(p.max_val + (size_t)qrow * p.n_tiles + tile, m);
                }
            }
                };
        // Refresh: checkpoints REFRESH_FIRST_SHIFT .. 1 halvings into the own range, each on a barrier tile; the tile loop runs
        // from one to the next and is itself unchanged.  A pool block has none (its thresholds were refreshed at the draw).
        int cp_shift = refresh && t0 < p.static_tiles ? REFRESH_FIRST_SHIFT : 0;
        int tile = t0;
        for (;;) {
        int tend = t1;
        while (cp_shift > 0) {
            const int cp = t0 + (((t1 - t0) >> cp_shift) & ~(STPB - 1));
            --cp_shift;
            if (cp > tile) {
                tend = cp;
                break;
            }
        }
        for (; tile < tend; ++tile) {
            if ((tile - t0) % STPB == 0) {
                // own DMAs of this interval's tiles have landed; the barrier extends that to every wave's
                // and guarantees every wave is done reading the tiles of the previous interval
                asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * (SRING - 2 * STPB)) : "memory");
                if (BF && tile == t0) { // bf16 rows, a segment's first interval: this wave's own two pieces of each of its
                                        // tiles, converted before the barrier publishes them (later intervals: below)
#pragma unroll
                    for (int i = 0; i < STPB; ++i)
                        bf16_to_f16_lds<2>(ring + ((stage + i) % SRING) * STILE_BYTES + (2 * w) * 1024, lane);
                    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                }
                __builtin_amdgcn_s_barrier();
            } else if (BF && (tile - t0) % STPB == STPB - 1) {
                // bf16 rows: the last tile of an interval converts the NEXT interval's pieces of this wave, off the barrier
                // path (the waves drift freely inside an interval).  The ring runs SRING - STPB tiles ahead, so those STPB
                // tiles have landed once at most the (SRING - 3 STPB + 1) younger tiles' pieces are pending; their slots
                // are read by nobody until the next barrier publishes them.  (Past the segment's end they hold the clamped
                // re-read of its last tile: converted, never read.)
                asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * (SRING - 3 * STPB + 1)) : "memory");
#pragma unroll
                for (int i = 1; i <= STPB; ++i)
                    bf16_to_f16_lds<2>(ring + ((stage + i) % SRING) * STILE_BYTES + (2 * w) * 1024, lane);
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            }
            // Every tile iteration refills the ring slot SRING - STPB tiles ahead (free since the last barrier);
            // the two LDS-DMA pieces go out between k-steps of the MFMA loop rather than in one burst behind
            // the barrier, where all eight waves would queue them at the same moment.
            const int fill_stage = (stage + SRING - STPB) % SRING;
            set_rows(min(tile + SRING - STPB, t1 - 1));
            if (!wave_live) {
                dma_piece(0, fill_stage);
                dma_piece(1, fill_stage);
            }
            if (wave_live) {
                if (late && pending)
                    epilogue(ptile, pkw);
                // acc[u][c][r] = s16(doc tile*32 + 16u + 4g + r, query qbase + 16c + n)
                // (main pass: minus the query's threshold, see negthr)
                const char *buf = ring + stage * STILE_BYTES + rd_base;
                // A fragments run two k-steps ahead of the MFMAs that consume them (three register sets);
                // the scheduling fences keep hipcc from sinking the reads back next to their use
                h8 a0[3], a1[3];
                auto a_read = [&](int s) {
                    const int off = ((4 * s + g) ^ n) << 4;
                    a0[s % 3] = *(const h8 *)(buf + off);
                    a1[s % 3] = *(const h8 *)(buf + 16 * 512 + off);
                };
                a_read(0);
                a_read(1);
                unsigned kw = 0xffffffffu; // the tile's keep word (MASKED)
#pragma unroll
                for (int s = 0; s < 8; ++s) {
                    if (s + 2 < 8)
                        a_read(s + 2);
                    // (MASKED: the word's load goes out in front of the tile's first MFMAs and is waited for behind its last,
                    //  so the whole multiply block covers it; tile is wave-uniform -- a pool draw arrives through LDS, hence
                    //  the readfirstlane -- and no LDS read of this tile is issued after k-step 5, so the counted lgkmcnt waits
                    //  hipcc puts in front of the MFMAs only get stricter by this one operation until it has landed)
                    if (MASKED && s == 0)
                        keep_word_issue(p.keep + __builtin_amdgcn_readfirstlane(tile), kw, a0[0]);
                    if (s == 2)
                        dma_piece(0, fill_stage);
                    if (s == 6)
                        dma_piece(1, fill_stage);
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int c = 0; c < NSET; ++c) {
                        const f32x4 c0 = s == 0 ? negthr[c] : acc[0][c];
                        const f32x4 c1 = s == 0 ? negthr[c] : acc[1][c];
                        acc[0][c] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a0[s % 3], qreg[c][s], c0, 0, 0, 0);
                        acc[1][c] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a1[s % 3], qreg[c][s], c1, 0, 0, 0);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
                if (MASKED)
                    keep_word_wait(kw, acc[1][NSET - 1]); // (the block's last MFMA writes this one)
                if (late) { // this tile's selection runs after the next barrier, beside the other half's MFMAs
                    pending = true;
                    ptile = tile;
                    pkw = kw;
                } else {
                    epilogue(tile, kw);
                }
            }
            stage = (stage + 1) % SRING;
        }
        if (wave_live && late && pending) {
            epilogue(ptile, pkw);
            pending = false;
        }
        if (tend == t1)
            break;
        if (wave_live) // between the deferred selection above and the next tile's multiply: no accumulator is live
            refresh_thresholds();
        }
    }
    if (MAXONLY || p.tail_blocks == 0)
        break;
    // The chip's eight XCDs do not run this loop at one speed (per-workgroup clocks: 3.61 .. 3.97 ms for identical
    // 10M-document shares, the medians of the XCDs 3.62 .. 3.96): with equal static shares the launch ends with its
    // slowest workgroup while the fastest idle for 9 % of it.  The last part of the corpus is therefore handed out in
    // blocks: whoever is done draws the next one (a fresh pipeline per block: ring primed again, ~3 us per ~30-50 us).
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // the clamped over-prefetch of the segment's end
    __builtin_amdgcn_s_barrier();                    // ... has landed for every wave; nobody reads the ring any more
    if (refresh && wave_live) // the ring is drained: what the chip has counted by now, for the pool block to come
        refresh_thresholds();
    if (threadIdx.x == 0)
        next_block = atomicAdd(p.tail_ctr + qgroup, 1);
    __syncthreads();
    const int blk = next_block;
    if (blk >= p.tail_blocks)
        break;
    t0 = p.static_tiles + blk * p.tail_g;
    t1 = min(t0 + p.tail_g, p.n_tiles);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier(); // no wave may leave while a sibling's LDS-DMA could still be consumed

    if (MAXONLY) {
        if (ONCHIP) {
#pragma unroll
            for (int c = 0; c < NSET; ++c) {
                const int qrow = qbase + 16 * c + n;
                if (qrow < p.B) {
                    float *dst = p.top_val + ((size_t)qrow * p.n_chunks + chunk) * (4 * STOP) + g * STOP;
#pragma unroll
                    for (int j = 0; j < STOP; ++j)
                        dst[j] = top[ONCHIP ? c : 0][j];
                }
            }
        }
        return;
    }
    // final compaction (bounds the pool the finish kernel sees) and counts out: quarter g's count in byte g
    int nf = n; // (through an empty asm: the query rows are formed again here instead of living in registers from the prologue on)
    asm volatile("" : "+v"(nf));
#pragma unroll
    for (int c = 0; c < NSET; ++c) {
        int tot = cnt[c] + __shfl_xor(cnt[c], 16);
        tot += __shfl_xor(tot, 32);
        const unsigned long long over = __ballot(tot > k) & 0xffffull;
        if (over)
            compact_where(c, (unsigned)over);
        int packed = cnt[c] << (8 * g);
        packed |= __shfl_xor(packed, 16);
        packed |= __shfl_xor(packed, 32);
        const int qrow = qbase + 16 * c + nf;
        if (g == 0 && qrow < p.B)
            p.pcnt[(size_t)qrow * p.n_chunks + chunk] = packed;
    }
}

// ------------------------------------------------------------------ small batches: streaming form
// For B <= 64 the shared-tile kernel above would leave most of a workgroup's eight waves without queries.  Here every
// WAVE is an independent streaming engine (the organisation of the exact kernel, score_topk.hip): it keeps one
// 32-query tile as B operands (64 VGPRs), walks its own range of documents through a private 4-slab LDS ring
// (slab = 32 documents x 64 features f16 = 4 KiB, 4 global_load_lds per slab, 3 slabs in flight, no barriers)
// and selects exactly like screen_kernel.  MFMA work is 1/16 of the exact kernel's, so the launch is bound by
// HBM streaming of the fp16 shadow corpus (N x 512 B).
constexpr int TW = 4;                    // waves per workgroup (2 workgroups per CU)
constexpr int TSLAB_BYTES = 32 * 128;    // 32 docs x 64 f16
constexpr int TSTAGE = 4;                // ring depth in slabs
constexpr int TDMA = 4;                  // DMA instructions per slab
// Cache policy of the document stream: nt (aux = 2).  Every byte is read once by one wave; with the default policy the
// same kernel reached 6.1-6.2 TB/s, with nt 6.8-6.9 (0.910 -> 0.816-0.824 ms per B = 32 search over 10M documents, A/B on
// one box; MI355X_MICROARCH.md 'nt-weights').  NOT for the exact kernel at large batches, whose 32 query tiles re-read a
// chunk from L2 (44.2 -> 52.9 ms at B = 1024 with nt), nor for the shared-tile screen (two workgroups per chunk).
constexpr int TSTREAM_AUX = 2;

// NQS = 16-query sets per wave: 2 (B <= 32), or 4 (33 <= B <= 64: ONE pass of the stream for 64 queries instead of the
// shared-tile form's 1.03 ms; twice the MFMAs per tile, still a fifth of what the stream allows)
// MASKED: as in screen_kernel; the word's load goes out in front of the tile's last slab of MFMAs, behind that slab's
// lgkmcnt(0) wait (the placement of the exact kernel's, score_topk.hip), and is waited for in front of the epilogue.
template <bool MAXONLY, int NQS = 2, bool BF = false, bool MASKED = false>
__global__ __launch_bounds__(TW * 64, 2) void screen_stream_kernel(ScreenParams p)
{
    constexpr int QPT = 16 * NQS; // queries per task
    extern __shared__ __attribute__((aligned(16))) char ring_all[]; // [TW][TSTAGE][TSLAB_BYTES]
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    char *const ring = ring_all + w * (TSTAGE * TSLAB_BYTES);
    const int task = blockIdx.x * TW + w;                 // = qtile * n_chunks + chunk
    const int n_qtiles = (p.B + QPT - 1) / QPT;
    if (task >= n_qtiles * p.n_chunks)
        return; // wave-uniform; this kernel has no workgroup barrier
    const int qtile = task / p.n_chunks, chunk = task % p.n_chunks;
    const int t0 = chunk * p.tiles_per_chunk;
    const int t1 = min(t0 + p.tiles_per_chunk, p.n_tiles);
    const int k = p.k;
    const int g = lane >> 4, n = lane & 15;
    const int qbase = qtile * QPT;

    // ---- query operands: set c holds queries qbase + 16c + n; lane (n,g) keeps features 32s + 8g .. +7 ----
    h8 qreg[NQS][8];
    float eps2[NQS];
    f32x4 negthr[NQS];
    int cnt[NQS];
#pragma unroll
    for (int c = 0; c < NQS; ++c) {
        cnt[c] = 0;
        const int qrow = qbase + 16 * c + n;
        const bool live = qrow < p.B;
        const h8 *src = p.qimg + ((size_t)(qbase / 16 + c) * 8) * 64 + lane;
#pragma unroll
        for (int s = 0; s < 8; ++s)
            qreg[c][s] = src[s * 64];
        const float qn = p.qnorm[qrow];
        eps2[c] = 2.0f * screen_eps(qn, p.dmax);
        const float floor_thr = -(1.01f * qn * p.dmax + 1e-30f);
        const float t_init = live ? ((!MAXONLY && p.thr0) ? fmaxf(p.thr0[(size_t)qrow * p.thr0_stride + p.thr0_stride - 1] - eps2[c], floor_thr)
                                                    : floor_thr)
                            : INFINITY;
        float c_init = -t_init;
        if (MAXONLY)
            c_init = (p.dbg_thr && live) ? -p.dbg_thr[qrow] : 0.0f;
        negthr[c] = f32x4{c_init, c_init, c_init, c_init};
    }

    SCand *const cwave = p.cand + (size_t)task * QPT * SCAP;

    auto compact_where = [&](int c, unsigned qmask) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        while (qmask) {
            const int q = __ffs((int)qmask) - 1;
            qmask &= qmask - 1;
            const int nq[4] = {__builtin_amdgcn_readlane(cnt[c], q), __builtin_amdgcn_readlane(cnt[c], q + 16),
                               __builtin_amdgcn_readlane(cnt[c], q + 32), __builtin_amdgcn_readlane(cnt[c], q + 48)};
            const float slack = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, eps2[c]), q));
            int n_new;
            float tn;
            bool have, ovf;
            screen_compact(cwave + (size_t)(16 * c + q) * SCAP, nq, k, slack, lane, n_new, tn, have, ovf);
            if (ovf && lane == 0)
                atomicOr(p.flag + ((qbase + 16 * c) >> 5), 1);
            if (n == q) {
                cnt[c] = (n_new - g + 3) >> 2;
                if (have)
                    negthr[c] = f32x4{-tn, -tn, -tn, -tn};
            }
        }
    };

    // ---- DMA: slab (tile, kq) = features 64kq..64kq+63 of the tile's 32 documents.  Instruction jj moves rows
    //      8jj..8jj+7: lane -> (row 8jj + lane/8, physical 16-B chunk lane%8); logical chunk = physical ^ (row & 7).
    const char *D = (const char *)p.D16;
    int dma_tile = t0, dma_kq = 0;
    const char *rowp[TDMA];
    auto set_rows = [&](int tile) {
#pragma unroll
        for (int jj = 0; jj < TDMA; ++jj) {
            const int row = 8 * jj + (lane >> 3);
            const int doc = min(tile * 32 + row, p.N - 1);
            rowp[jj] = D + (size_t)doc * 512 + (((lane & 7) ^ (row & 7)) << 4);
        }
    };
    auto dma_issue = [&](int stage) {
        char *dst = ring + stage * TSLAB_BYTES;
#pragma unroll
        for (int jj = 0; jj < TDMA; ++jj)
            __builtin_amdgcn_global_load_lds((gbl_void *)(rowp[jj] + dma_kq * 128), (lds_void *)(dst + jj * 1024), 16, 0, TSTREAM_AUX);
        if (++dma_kq == 4) {
            dma_kq = 0;
            dma_tile = min(dma_tile + 1, t1 - 1); // past the end: harmless re-read
            set_rows(dma_tile);
        }
    };

    if (t0 < t1) {
        set_rows(t0);
#pragma unroll
        for (int i = 0; i < TSTAGE - 1; ++i)
            dma_issue(i);
        int stage = 0;
        // A row (document) n of sub-tile 0 / 16 + n of sub-tile 1; both have row & 7 == n & 7
        const char *rd_row = ring + n * 128;
        const int rsw = n & 7;
        for (int tile = t0; tile < t1; ++tile) {
            f32x4 acc[2][NQS]; // acc[u][c][r] = s16(doc tile*32 + 16u + 4g + r, query qbase + 16c + n) - thr
            unsigned kw = 0xffffffffu; // the tile's keep word (MASKED)
#pragma unroll
            for (int kq = 0; kq < 4; ++kq) {
                // slab (tile,kq) has landed once at most TSTAGE-2 younger slabs are pending (candidate stores
                // also count in vmcnt: they only make this wait stricter)
                asm volatile("s_waitcnt vmcnt(%0)" ::"n"(TDMA * (TSTAGE - 2)) : "memory");
                if (BF) { // bf16 rows: the wave's own slab, converted in place before its reads
                    bf16_to_f16_lds<TSLAB_BYTES / 1024>(ring + stage * TSLAB_BYTES, lane);
                    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                }
                const char *buf = rd_row + stage * TSLAB_BYTES;
                h8 a[2][2];
#pragma unroll
                for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
                    for (int u = 0; u < 2; ++u)
                        a[u][s2] = *(const h8 *)(buf + u * 2048 + (((4 * s2 + g) ^ rsw) << 4));
                // the ring slot consumed one step ago is free once its reads have returned
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                // (MASKED: right behind the asm wait above, which already ends a scheduling region; no LDS read of this tile
                //  follows, so nothing else waits on lgkmcnt until keep_word_wait)
                if (MASKED && kq == 3)
                    keep_word_issue(p.keep + tile, kw, a[0][0]);
                dma_issue((stage + TSTAGE - 1) % TSTAGE);
#pragma unroll
                for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
                    for (int c = 0; c < NQS; ++c)
#pragma unroll
                        for (int u = 0; u < 2; ++u) {
                            const f32x4 cin = (kq == 0 && s2 == 0) ? negthr[c] : acc[u][c];
                            acc[u][c] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[u][s2], qreg[c][2 * kq + s2], cin, 0, 0, 0);
                        }
                stage = (stage + 1) % TSTAGE;
            }
            const int tile_base = tile * 32;
            const bool partial = tile_base + 32 > p.N;
            // MASKED: see screen_kernel's epilogue
            if (MASKED)
                keep_word_wait(kw, acc[1][NQS - 1]); // (the slab's last MFMA writes this one)
            const bool holes = MASKED && kw != 0xffffffffu;
            const unsigned kwg = MASKED ? kw >> (4 * g) : 0xffffffffu;
            auto dropped = [&](int u, int r) {
                return tile_base + 16 * u + 4 * g + r >= p.N || (MASKED && ((kwg >> (16 * u + r)) & 1u) == 0u);
            };
            if (!MAXONLY) {
                if (MASKED && kw == 0u)
                    continue; // nothing kept: no candidate can come from this tile
                if (partial || holes) {
#pragma unroll
                    for (int u = 0; u < 2; ++u)
#pragma unroll
                        for (int r = 0; r < 4; ++r)
                            if (dropped(u, r)) {
#pragma unroll
                                for (int c = 0; c < NQS; ++c)
                                    acc[u][c][r] = -INFINITY;
                            }
                }
                int mall = INT_MIN;
#pragma unroll
                for (int u = 0; u < 2; ++u)
#pragma unroll
                    for (int c = 0; c < NQS; ++c)
#pragma unroll
                        for (int r = 0; r < 4; ++r)
                            mall = max(mall, __float_as_int(acc[u][c][r]));
                if (__ballot(mall >= 0) != 0ull) {
#pragma unroll
                    for (int c = 0; c < NQS; ++c) {
                        const unsigned mine = (unsigned)(((16 * c + n) * SCAP + SQUART * g) * sizeof(SCand));
                        const float thr_c = -negthr[c][0];
#pragma unroll
                        for (int u = 0; u < 2; ++u)
#pragma unroll
                            for (int r = 0; r < 4; ++r) {
                                if (__float_as_int(acc[u][c][r]) >= 0) {
                                    scand_store_async(cwave, mine + (unsigned)cnt[c] * (unsigned)sizeof(SCand),
                                                      acc[u][c][r] + thr_c, tile_base + 16 * u + 4 * g + r);
                                    ++cnt[c];
                                }
                            }
                        unsigned long long full = __ballot(cnt[c] > SQ_TRIGGER);
                        full = (full | (full >> 32));
                        full = (full | (full >> 16)) & 0xffffull;
                        if (full)
                            compact_where(c, (unsigned)full);
                    }
                }
            } else {
#pragma unroll
                for (int c = 0; c < NQS; ++c) {
                    float m = -INFINITY;
#pragma unroll
                    for (int u = 0; u < 2; ++u)
#pragma unroll
                        for (int r = 0; r < 4; ++r)
                            m = fmaxf(m, ((!partial && !holes) || !dropped(u, r)) ? acc[u][c][r] : -INFINITY);
                    m = fmaxf(m, __shfl_xor(m, 16));
                    m = fmaxf(m, __shfl_xor(m, 32));
                    const int qrow = qbase + 16 * c + n;
                    if (g == 0 && qrow < p.B)
                        f32_store_async(p.max_val + (size_t)qrow * p.n_tiles + tile, m);
                }
            }
        }
    }
    // LDS-DMA still in flight would land after the wave has ended: drain it (and the stores)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (MAXONLY)
        return;
#pragma unroll
    for (int c = 0; c < NQS; ++c) {
        int tot = cnt[c] + __shfl_xor(cnt[c], 16);
        tot += __shfl_xor(tot, 32);
        const unsigned long long over = __ballot(tot > k) & 0xffffull;
        if (over)
            compact_where(c, (unsigned)over);
        int packed = cnt[c] << (8 * g);
        packed |= __shfl_xor(packed, 16);
        packed |= __shfl_xor(packed, 32);
        const int qrow = qbase + 16 * c + n;
        if (g == 0 && qrow < p.B)
            p.pcnt[(size_t)qrow * p.n_chunks + chunk] = packed;
    }
}

// ------------------------------------------------------------------ finish
struct FinishParams {
    const float *Q;
    const float *D32;
    const unsigned *Dbf; // bf16 corpus instead of D32 (512-B rows of bf16 pairs), or null
    int B, N, k, n_chunks;
    float dmax;
    const SCand *cand;
    const int *pcnt;
    int *flag;
    int64_t idx_offset;
    float *out_val;
    int64_t *out_idx;
    int q_per_block; // candidate layout [query group][chunk][q_per_block][SCAP]: 512 (shared tiles) or 32 (streaming)
    int *stats;      // [B][2]: pooled candidates, survivors (>= A_k - 2 eps) of each query -- what the filter let through
};

__device__ __forceinline__ bool before_f(float sa, int ia, float sb, int ib) { return sa > sb || (sa == sb && ia < ib); }

// float <-> unsigned with the same ordering (for the radix select)
__device__ __forceinline__ unsigned f32_order_key(float f)
{
    const unsigned b = __float_as_uint(f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float f32_from_order_key(unsigned k)
{
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// Four workgroups per CU, so that the B = 1024 workgroups of the bench step are one round on 256 CUs (three per CU -- 43 296 B
// of LDS, 140 VGPRs -- made it a round and a third: 44.1 -> 31.9 us, profiles/sample_onchip.md): 39 200 B static + 1 028 B
// dynamic at 128 chunks <= 40 960 B, and the launch bound holds the registers at 128 or fewer (92, no scratch).
__global__ __launch_bounds__(256, 4) void screen_finish_kernel(FinishParams p)
{
    __shared__ float pool_v[POOL_MAX];
    __shared__ float qs[256];
    float *const sv_v = pool_v; // [SURV_MAX]: the pool is dead behind the survivor selection, whose closing barrier precedes the first write
    __shared__ int sv_x[SURV_MAX];
    __shared__ float red_v[4];
    __shared__ int hist[256];
    // per-chunk tables sized at launch (2 n_chunks + 1 ints): the shared-tile form has <= 255 chunks, which keeps
    // the workgroup under 40 KB of LDS and four of them on a CU; the streaming form needs up to FIN_MAX_CHUNKS
    extern __shared__ int fin_dyn[];
    int *const ccnt = fin_dyn;                  // packed quarter counts per chunk
    int *const pre = fin_dyn + p.n_chunks;      // exclusive prefix of the per-chunk totals (n_chunks + 1)
    __shared__ int sel[2];
    __shared__ int n_pool, n_surv;
    const int row = blockIdx.x, tid = threadIdx.x;
    if (tid == 0)
        n_pool = n_surv = 0;
    qs[tid] = p.Q[(size_t)row * 256 + tid];
    __syncthreads();
    // |q| (fixed-order enough: any fp32 rounding is covered by the safety factor in screen_eps)
    float ss = qs[tid] * qs[tid];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1)
        ss += __shfl_xor(ss, off);
    if ((tid & 63) == 0)
        red_v[tid >> 6] = ss;
    __syncthreads();
    const float eps2 = 2.0f * screen_eps(sqrtf(red_v[0] + red_v[1] + red_v[2] + red_v[3]), p.dmax);
    __syncthreads();

    // ---- pool every workgroup's candidates for this query (counts -> prefix -> parallel copy) ----
    const int qgroup = row / p.q_per_block, qin = row % p.q_per_block;
    bool too_many = false;
    // per-chunk totals: thread t owns chunks [t*per, t*per+per); its sum -> hist[t]; thread 0 scans the 256 sums
    const int per = (p.n_chunks + 255) / 256;
    {
        int sum = 0;
        for (int c = tid * per; c < min(tid * per + per, p.n_chunks); ++c) {
            const int v = p.pcnt[(size_t)row * p.n_chunks + c]; // quarter counts, one per byte
            ccnt[c] = v;
            sum += (v & 0xff) + ((v >> 8) & 0xff) + ((v >> 16) & 0xff) + ((v >> 24) & 0xff);
        }
        // exclusive scan of the 256 per-thread sums: shuffles inside each wave, then the 4 wave totals
        int inc = sum;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int v = __shfl_up(inc, off);
            if ((tid & 63) >= off)
                inc += v;
        }
        if ((tid & 63) == 63)
            hist[tid >> 6] = inc; // wave totals in hist[0..3] (hist is free until the select)
        __syncthreads();
        int base = 0;
        for (int wv = 0; wv < (tid >> 6); ++wv)
            base += hist[wv];
        if (tid == 255)
            n_pool = base + inc;
        __syncthreads();
        hist[tid] = base + inc - sum;
    }
    __syncthreads();
    {
        int run = hist[tid];
        for (int c = tid * per; c < min(tid * per + per, p.n_chunks); ++c) {
            pre[c] = run;
            const int v = ccnt[c];
            run += (v & 0xff) + ((v >> 8) & 0xff) + ((v >> 16) & 0xff) + ((v >> 24) & 0xff);
        }
        if (tid == 255)
            pre[p.n_chunks] = n_pool;
    }
    __syncthreads();
    const int total = n_pool;
    if (total > POOL_MAX)
        too_many = true;
    // pooled position m -> its entry in the candidate buffers (chunk by binary search, then quarter and slot).
    // Only the scores are pooled in LDS; the few survivors fetch their document index through the same mapping.
    auto locate = [&](int m) -> const SCand * {
        int lo = 0, hi = p.n_chunks; // largest c with pre[c] <= m
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (pre[mid] <= m)
                lo = mid;
            else
                hi = mid;
        }
        int o = m - pre[lo], slot = 0; // quarter g of the buffer starts at entry 32 g
#pragma unroll
        for (int gq = 0; gq < 4; ++gq) {
            const int ng = (ccnt[lo] >> (8 * gq)) & 0xff;
            if (o >= 0 && o < ng)
                slot = SQUART * gq + o;
            o -= ng;
            if (o < 0)
                o = INT_MIN / 2;
        }
        return p.cand + ((size_t)(qgroup * p.n_chunks + lo) * p.q_per_block + qin) * SCAP + slot;
    };
    for (int m = tid; m < total && m < POOL_MAX; m += 256)
        pool_v[m] = locate(m)->v;
    __syncthreads();
    const int np = min(n_pool, POOL_MAX);
    // ---- A_k = k-th best approximate score over the whole corpus: 4-pass radix select on the
    //      order-preserving integer image of the scores (cost independent of k) ----
    float kth = -INFINITY;
    const int found = np >= p.k ? p.k : np;
    if (np >= p.k) {
        unsigned prefix = 0u, mask = 0u;
        int k_rem = p.k;
#pragma unroll 1
        for (int pass = 0; pass < 4; ++pass) {
            const int shift = 24 - 8 * pass;
            hist[tid] = 0;
            __syncthreads();
            for (int m = tid; m < np; m += 256) {
                const unsigned key = f32_order_key(pool_v[m]);
                if ((key & mask) == prefix)
                    atomicAdd(&hist[(key >> shift) & 255u], 1);
            }
            __syncthreads();
            if (tid < 64) { // one wave: suffix sums over the 256 bins (4 per lane, high bins first)
                const int ln = tid;
                int c[4], sm = 0;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    c[i] = hist[255 - (ln * 4 + i)];
                    sm += c[i];
                }
                int incl = sm;
#pragma unroll
                for (int off = 1; off < 64; off <<= 1) {
                    const int y = __shfl_up(incl, off);
                    if (ln >= off)
                        incl += y;
                }
                int above = incl - sm;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    if (above < k_rem && above + c[i] >= k_rem) {
                        sel[0] = 255 - (ln * 4 + i);
                        sel[1] = above;
                    }
                    above += c[i];
                }
            }
            __syncthreads();
            prefix |= (unsigned)sel[0] << shift;
            mask |= 0xffu << shift;
            k_rem -= sel[1];
            __syncthreads();
        }
        kth = f32_from_order_key(prefix);
    }
    const float cut = found == p.k ? kth - eps2 : -INFINITY;
    // ---- survivors, exact fp32 FMA-chain rescoring (the oracle's order: features ascending) ----
    for (int m = tid; m < np; m += 256) {
        if (pool_v[m] >= cut) {
            const int slot = atomicAdd(&n_surv, 1);
            if (slot < SURV_MAX)
                sv_x[slot] = locate(m)->x;
            else
                too_many = true;
        }
    }
    __syncthreads();
    const int ns = min(n_surv, SURV_MAX);
    for (int sidx = tid; sidx < ns; sidx += 256) {
        // one thread per survivor (a second, third, fourth round only beyond 256 of them): the chain is sequential by
        // definition, but the row's loads are not -- 16 of them (256 B) are issued back to back before the 64 fmaf that
        // consume them, four batches per row (left to hipcc the loop waited for one 16-byte load per iteration: ~30 us of a
        // 46 us kernel at k = 50)
        float acc = 0.0f;
        if (p.Dbf) { // bf16 rows: widened exactly, the same fmaf chain
            const unsigned *brow = p.Dbf + (size_t)sv_x[sidx] * 128;
#pragma unroll 1
            for (int x0 = 0; x0 < 256; x0 += 64) {
                u32x4 dv[8];
#pragma unroll
                for (int i = 0; i < 8; ++i)
                    dv[i] = __builtin_nontemporal_load((const u32x4 *)(brow + x0 / 2 + 4 * i));
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const unsigned wv[4] = {dv[i].x, dv[i].y, dv[i].z, dv[i].w};
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        acc = fmaf(qs[x0 + 8 * i + 2 * e], __uint_as_float(wv[e] << 16), acc);
                        acc = fmaf(qs[x0 + 8 * i + 2 * e + 1], __uint_as_float(wv[e] & 0xffff0000u), acc);
                    }
                }
            }
            sv_v[sidx] = acc;
            continue;
        }
        const float *drow = p.D32 + (size_t)sv_x[sidx] * 256;
#pragma unroll 1
        for (int x0 = 0; x0 < 256; x0 += 64) {
            f32x4 dv[16];
#pragma unroll
            for (int i = 0; i < 16; ++i)
                dv[i] = __builtin_nontemporal_load((const f32x4 *)(drow + x0 + 4 * i));
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                acc = fmaf(qs[x0 + 4 * i], dv[i].x, acc);
                acc = fmaf(qs[x0 + 4 * i + 1], dv[i].y, acc);
                acc = fmaf(qs[x0 + 4 * i + 2], dv[i].z, acc);
                acc = fmaf(qs[x0 + 4 * i + 3], dv[i].w, acc);
            }
        }
        sv_v[sidx] = acc;
    }
    if (tid == 0) {
        p.stats[2 * row] = n_pool;
        p.stats[2 * row + 1] = n_surv;
    }
    if (__syncthreads_or(too_many) && tid == 0)
        atomicOr(p.flag + (row >> 5), 4);
    // ---- exact top-k of the survivors: every thread ranks its own survivor against all others ----
    __syncthreads();
    for (int sidx = tid; sidx < ns; sidx += 256) {
        const float mv = sv_v[sidx];
        const int mx = sv_x[sidx];
        int rank = 0;
        for (int u = 0; u < ns; ++u)
            rank += before_f(sv_v[u], sv_x[u], mv, mx) ? 1 : 0;
        if (rank < p.k) {
            p.out_val[(size_t)row * p.k + rank] = mv;
            p.out_idx[(size_t)row * p.k + rank] = p.idx_offset + mx;
        }
    }
    for (int r = ns + tid; r < p.k; r += 256) { // fewer survivors than k (tiny corpora)
        p.out_val[(size_t)row * p.k + r] = -INFINITY;
        p.out_idx[(size_t)row * p.k + r] = -1;
    }
}

// ------------------------------------------------------------------ fp16 shadow copy + corpus stats
__global__ __launch_bounds__(256) void build_f16_kernel(const float *__restrict__ D, int64_t N, int d,
                                                        _Float16 *__restrict__ out, unsigned *__restrict__ stats)
{
    __shared__ float red[8];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float nmax = 0.0f, amax = 0.0f;
    for (int64_t row = (int64_t)blockIdx.x * 4 + wave; row < N; row += (int64_t)gridDim.x * 4) {
        float ss = 0.0f;
        for (int x = lane * 4; x < d; x += 256) {
            const f32x4 v = *(const f32x4 *)(D + row * d + x);
            h4 hv;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                ss += v[e] * v[e];
                amax = fmaxf(amax, fabsf(v[e]));
                if (!(fabsf(v[e]) <= 3.0e38f))
                    amax = INFINITY; // NaN / inf anywhere disables the screen
                hv[e] = (_Float16)v[e];
            }
            *(h4 *)(out + row * d + x) = hv;
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1)
            ss += __shfl_xor(ss, off);
        nmax = fmaxf(nmax, sqrtf(ss));
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1)
        amax = fmaxf(amax, __shfl_xor(amax, off));
    if (lane == 0) {
        red[wave] = nmax;
        red[4 + wave] = amax;
    }
    __syncthreads();
    if (threadIdx.x == 0) { // non-negative floats order like their bit patterns; inf is the largest
        atomicMax(stats, __float_as_uint(fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]))));
        atomicMax(stats + 1, __float_as_uint(fmaxf(fmaxf(red[4], red[5]), fmaxf(red[6], red[7]))));
    }
}

// bf16 rows (streamed corpus blocks) -> fp32 rows (exact: bf16 is a truncated fp32) + fp16 shadow + stats
__global__ __launch_bounds__(256) void build_from_bf16_kernel(const unsigned short *__restrict__ S, int64_t N, int d,
                                                              float *__restrict__ out32, _Float16 *__restrict__ out16,
                                                              unsigned *__restrict__ stats)
{
    __shared__ float red[8];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float nmax = 0.0f, amax = 0.0f;
    for (int64_t row = (int64_t)blockIdx.x * 4 + wave; row < N; row += (int64_t)gridDim.x * 4) {
        float ss = 0.0f;
        for (int x = lane * 4; x < d; x += 256) {
            const uint2 raw = *(const uint2 *)(S + row * d + x);
            f32x4 v;
            v[0] = __uint_as_float(raw.x << 16);
            v[1] = __uint_as_float(raw.x & 0xffff0000u);
            v[2] = __uint_as_float(raw.y << 16);
            v[3] = __uint_as_float(raw.y & 0xffff0000u);
            h4 hv;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                ss += v[e] * v[e];
                amax = fmaxf(amax, fabsf(v[e]));
                if (!(fabsf(v[e]) <= 3.0e38f))
                    amax = INFINITY;
                hv[e] = (_Float16)v[e];
            }
            if (out32) // (null: tt_index_stats_bf16, the statistics alone)
                *(f32x4 *)(out32 + row * d + x) = v;
            if (out16)
                *(h4 *)(out16 + row * d + x) = hv;
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1)
            ss += __shfl_xor(ss, off);
        nmax = fmaxf(nmax, sqrtf(ss));
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1)
        amax = fmaxf(amax, __shfl_xor(amax, off));
    if (lane == 0) {
        red[wave] = nmax;
        red[4 + wave] = amax;
    }
    __syncthreads();
    if (threadIdx.x == 0 && stats) {
        atomicMax(stats, __float_as_uint(fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]))));
        atomicMax(stats + 1, __float_as_uint(fmaxf(fmaxf(red[4], red[5]), fmaxf(red[6], red[7]))));
    }
}

struct SPlan {
    bool stream;      // B <= STREAM_MAX_B: one independent streaming wave per (32-query tile, document chunk)
    int nset;         // shared-tile form: 16-query sets per wave (4, 3, 2 or 1)
    int n_qgroups;    // query groups of q_per_block rows (workgroup rows of 128 nset queries, or 32-query tiles when streaming)
    int q_per_block;
    int n_tiles, n_chunks, tiles_per_chunk;
    int static_tiles, tail_g, tail_blocks; // shared-tile main pass: see ScreenParams
    size_t tailctr_off;
    // Shared-tile main pass: thresholds are refreshed from the chip-wide ladders (ScreenParams::hist) when the search has a seed
    // and a chunk's share is at least REFRESH_MIN_TILES tiles long.  With refresh the pooled-candidate statistics
    // depend on timing (the results never do), so searches whose statistics the tests compare -- own ranges up to 245 tiles --
    // must stay below the gate.
    bool refresh;
    size_t hist_off; // [rows_pad][REFRESH_LEVELS] u32 (shared-tile form; 0: none)
    // sample pass
    bool sample;
    int s_tiles, s_chunks, s_tiles_per_chunk;
    int64_t s_docs;
    bool s_onchip; // the sample pass keeps its maxima in registers (ScreenParams::top_val)
    int s_vals;    // values per query the seed is selected from: s_chunks * 4 * STOP kept slice maxima, or s_tiles tile maxima
    size_t cand_off, pcnt_off, smax_val_off, sthr_val_off, qimg_off, qnorm_off, stats_off, ws_bytes;
    int rows_pad; // n_qgroups * q_per_block
};

constexpr int64_t SAMPLE_MIN_N = 65536;
constexpr int STREAM_MAX_B = 64; // one streaming pass: 32 queries per wave (2 sets) up to B = 32, 64 (4 sets) up to B = 64;
                                 // beyond that the shared-tile kernel wins (B = 65 .. 128: 1.20 ms against two passes)

// Document chunks per query group for one round of resident work: streaming, 8 resident waves per CU (2 workgroups of 4);
// shared-tile, one workgroup per CU (8 waves x 256 VGPRs) -- the per-workgroup set-up (query load + conversion, final
// compaction) is ~0.1 ms and would be paid once per round.
int one_round(bool stream, int n_qgroups)
{
    return stream ? (tt_device_cus() * 2 * TW + n_qgroups - 1) / n_qgroups : (tt_device_cus() + n_qgroups - 1) / n_qgroups;
}

SPlan make_splan(int B, int64_t N, int k)
{
    SPlan pl;
    pl.stream = B <= STREAM_MAX_B;
    if (B <= SW * 32) {
        pl.nset = B <= SW * 16 ? 1 : 2;
    } else { // as few groups as 512-query groups would need, as evenly filled as whole 16-query sets per wave allow
        const int groups = (B + SW * 64 - 1) / (SW * 64);
        pl.nset = (B + groups - 1) / groups <= SW * 48 ? 3 : 4;
    }
    pl.q_per_block = pl.stream ? (B <= 32 ? 32 : 64) : SW * 16 * pl.nset;
    pl.n_qgroups = (B + pl.q_per_block - 1) / pl.q_per_block;
    pl.n_tiles = (int)((N + 31) / 32);
    // streaming: with seeded thresholds a chunk rarely keeps anything; without them every chunk ends with >= k entries and
    // the finish kernel's pool bounds the number of chunks.  Shared-tile: room in that pool for k + slack entries per chunk.
    int max_chunks = pl.stream && N >= SAMPLE_MIN_N ? FIN_MAX_CHUNKS : POOL_MAX / (k + 16);
    if (!pl.stream)
        max_chunks = max_chunks > 255 ? 255 : max_chunks;
    const TTChunks c = tt_chunks(pl.n_tiles, one_round(pl.stream, pl.n_qgroups), max_chunks);
    pl.n_chunks = c.n_chunks;
    // pool = the last 1/TT_SCREEN_TAIL_DIV of every chunk's share (0: everything static), in blocks of a quarter of
    // that share, 8..32 tiles; only worth it when a share is long enough for several blocks
    const TTTailSplit t = tt_tail_split(c.tiles_per_chunk, c.n_chunks, pl.n_tiles,
                                        pl.stream ? 0 : TT_AB_SWITCH(TT_SCREEN_TAIL_DIV, 8), 16, 8, 32);
    pl.tiles_per_chunk = t.own;
    pl.static_tiles = t.static_tiles;
    pl.tail_g = t.tail_g;
    pl.tail_blocks = t.tail_blocks;
    const int n_tasks = pl.n_qgroups * pl.n_chunks;
    const size_t rows = (size_t)pl.n_qgroups * pl.q_per_block;
    pl.rows_pad = (int)rows;
    // sample pass: one maximum per 32-document tile of the sample; the k-th largest seeds the thresholds
    pl.sample = N >= SAMPLE_MIN_N;
    // Sample size: 1/64 of the corpus, or enough documents that the k-th sample maximum lets through about
    // one candidate per 32x32 score tile or fewer (k / s_docs per score): matters for small shards, large k.
    int64_t s_docs = N / 64;
    // measured on a 1.25M-document shard (B = 1024, A/B on one box): k = 10: 2048 -> 0.697, 4096 -> 0.664, 8192 -> 0.677 ms;
    // k = 50: 2048 -> 0.735, 4096 -> 0.767, 8192 -> 0.827 ms (the sample pass itself grows with k * per_k)
    const int per_k = k <= 16 ? 4096 : 2048;
    const int64_t s_min = (int64_t)k * per_k < N / 4 ? (int64_t)k * per_k : N / 4;
    s_docs = s_docs < s_min ? s_min : s_docs;
    s_docs = s_docs < 32 ? 32 : s_docs;
    pl.s_docs = (s_docs + 31) / 32 * 32;
    pl.s_tiles = (int)(pl.s_docs / 32);
    const TTChunks sc = tt_chunks(pl.s_tiles, one_round(pl.stream, pl.n_qgroups), INT_MAX); // one maximum per TILE
    pl.s_tiles_per_chunk = sc.tiles_per_chunk;
    pl.s_chunks = pl.sample ? sc.n_chunks : 0;
    // Shared-tile form: 4 s_chunks lanes ("streams") share a query's sample, each keeps STOP maxima.  With few streams (B beyond
    // 2048 on 256 CUs) several of a query's k best slices would often meet in one and the seed would sink by more than a rank:
    // the per-tile maxima stay.  (TT_SCREEN_SAMPLE_ONCHIP = 0, comparison build only: the per-tile maxima at every size.)
    // The kept maxima are dead once the seed is selected and the candidate buffers are first written by the main pass, so the
    // former lie in the latter (n_chunks KiB per query against 32 s_chunks bytes: it fits wherever both passes get a round of
    // chunks) and the workspace has no sample buffer of its own in this form.
    const size_t cand_bytes = (size_t)n_tasks * pl.q_per_block * SCAP * sizeof(SCand);
    pl.s_onchip = pl.sample && !pl.stream && pl.s_chunks >= STOP_MIN_CHUNKS && TT_AB_SWITCH(TT_SCREEN_SAMPLE_ONCHIP, 1) != 0 &&
                  rows * (size_t)pl.s_chunks * 4 * STOP * sizeof(float) <= cand_bytes;
    pl.s_vals = pl.s_onchip ? pl.s_chunks * 4 * STOP : pl.s_tiles;
    TTWorkspace ws;
    pl.cand_off = ws.take(cand_bytes);
    pl.pcnt_off = ws.take(rows * pl.n_chunks * sizeof(int));
    pl.sthr_val_off = ws.take(rows * sizeof(float));
    pl.qimg_off = ws.take(rows * 256 * sizeof(_Float16));
    pl.qnorm_off = ws.take(rows * sizeof(float));
    pl.tailctr_off = ws.take((size_t)pl.n_qgroups * sizeof(int));
    pl.stats_off = ws.take(rows * 2 * sizeof(int));
    pl.hist_off = pl.stream ? 0 : ws.take(rows * REFRESH_LEVELS * sizeof(unsigned));
    const int refresh_min = TT_AB_SWITCH(TT_SCREEN_REFRESH_MIN_TILES, REFRESH_MIN_TILES);
    // (the gate looks at a chunk's whole share, c.tiles_per_chunk, pool part included: the figure the plan is known by)
    pl.refresh = !pl.stream && TT_AB_SWITCH(TT_SCREEN_THR_REFRESH, 1) != 0 && c.tiles_per_chunk >= (refresh_min < 8 ? 8 : refresh_min);
    // (last: the one buffer that depends on the form of the sample pass, so every other offset is the same in both)
    pl.smax_val_off = pl.s_onchip ? pl.cand_off : ws.take(rows * (size_t)(pl.sample ? pl.s_tiles : 1) * sizeof(float));
    pl.ws_bytes = ws.off;
    return pl;
}

// Every screen kernel there is, by what a launch does with the scores, by the rows it reads (BF: bf16 rows, converted in LDS:
// bf16_to_f16_lds), by whether it runs under ScreenParams::keep (MASKED), and by form.
// KIND_MAIN: candidates.  KIND_MAXONLY: tile maxima only (the sample pass and tt_debug_screen_s16).  KIND_ONCHIP: the sample pass
// of the shared-tile form with its maxima kept in registers (ScreenParams::top_val).
enum ScreenKind { KIND_MAIN, KIND_MAXONLY, KIND_ONCHIP };
// form 0, 1: streaming with 2, 4 query sets per wave (q_per_block 32, 64); form 1 + nset: shared-tile, nset = 1..4 16-query sets
// per wave.  (KIND_ONCHIP has no streaming form: launch_screen refuses; the two places hold the MAXONLY kernels.)
#define SCREEN_FORMS(MAXONLY, BF, MASKED, ONCHIP)                                                                             \
    {(const void *)screen_stream_kernel<MAXONLY, 2, BF, MASKED>, (const void *)screen_stream_kernel<MAXONLY, 4, BF, MASKED>, \
     (const void *)screen_kernel<MAXONLY, 1, BF, MASKED, ONCHIP>, (const void *)screen_kernel<MAXONLY, 2, BF, MASKED, ONCHIP>, \
     (const void *)screen_kernel<MAXONLY, 3, BF, MASKED, ONCHIP>, (const void *)screen_kernel<MAXONLY, 4, BF, MASKED, ONCHIP>}
#define SCREEN_KIND(MAXONLY, ONCHIP)                                                             \
    {{SCREEN_FORMS(MAXONLY, false, false, ONCHIP), SCREEN_FORMS(MAXONLY, false, true, ONCHIP)}, \
     {SCREEN_FORMS(MAXONLY, true, false, ONCHIP), SCREEN_FORMS(MAXONLY, true, true, ONCHIP)}}
const void *const SCREEN_FN[3][2][2][6] = {SCREEN_KIND(false, false), SCREEN_KIND(true, false), SCREEN_KIND(true, true)}; // [kind][BF][MASKED][form]
#undef SCREEN_KIND
#undef SCREEN_FORMS

// One screen launch over pl's query groups x p.n_chunks document chunks: a wave per task when streaming, a workgroup otherwise.
// p says what it is: maxima into p.top_val or p.max_val, else candidates; the MASKED instantiation when p.keep is set.
int launch_screen(const SPlan &pl, ScreenParams p, bool bf16, hipStream_t st)
{
    if (p.top_val && pl.stream)
        return tt_fail(TT_ERR_UNSUPPORTED, "launch_screen: top_val outside the shared-tile sample pass");
    const ScreenKind kind = p.top_val ? KIND_ONCHIP : p.max_val ? KIND_MAXONLY : KIND_MAIN;
    const void *fn = SCREEN_FN[kind][bf16][p.keep != nullptr][pl.stream ? pl.q_per_block == 64 : 1 + pl.nset];
    const int n_tasks = pl.n_qgroups * p.n_chunks;
    const size_t lds = pl.stream ? (size_t)TW * TSTAGE * TSLAB_BYTES : (size_t)SRING * STILE_BYTES;
    const int blocks = pl.stream ? (n_tasks + TW - 1) / TW : n_tasks;
    TT_HIP_CHECK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    void *args[] = {&p};
    TT_HIP_CHECK(hipLaunchKernel(fn, dim3(blocks), dim3((pl.stream ? TW : SW) * 64), args, lds, st));
    return TT_OK;
}

// The exact fallback's workspace, which lies behind the screen's own (SPlan::ws_bytes): the k <= 64 search's over the same rows
size_t fallback_ws_bytes(int B, int64_t N, int d, int k, bool bf16)
{
    return bf16 ? tt_score_topk_bf16_workspace_bytes(B, N, d, k) : tt_score_topk_workspace_bytes(B, N, d, k);
}

// The screened size and offset queries: 0 for a shape without queries or documents; else `behind` + the plan's `what`
size_t splan_query(int B, int64_t N, int k, size_t SPlan::*what, size_t behind)
{
    return B <= 0 || N <= 0 ? 0 : make_splan(B, N, k).*what + behind;
}

} // namespace

TT_EXPORT int tt_index_build_f16(const float *D, int64_t N, int d, void *D16, float *stats, tt_stream_t stream)
{
    if (N < 0 || d <= 0 || (d & 3))
        return tt_fail(TT_ERR_BAD_SHAPE, "tt_index_build_f16: N=%lld d=%d", (long long)N, d);
    if (!stats || (N > 0 && (!D || !D16)))
        return tt_fail(TT_ERR_BAD_SHAPE, "tt_index_build_f16: null pointer");
    hipStream_t st = (hipStream_t)stream;
    TT_RC_CHECK(tt_zero_async(stats, 2 * sizeof(float), st));
    if (N == 0)
        return TT_OK;
    const int64_t want_blocks = (N + 3) / 4;
    hipLaunchKernelGGL(build_f16_kernel, dim3((unsigned)(want_blocks > 8192 ? 8192 : want_blocks)), dim3(256), 0, st, D,
                       N, d, (_Float16 *)D16, (unsigned *)stats);
    TT_LAUNCH_CHECK();
    return TT_OK;
}

TT_EXPORT int tt_index_build_from_bf16(const void *D_bf16, int64_t N, int d, float *D32, void *D16, float *stats,
                                       int reset_stats, tt_stream_t stream)
{
    if (N < 0 || d <= 0 || (d & 3))
        return tt_fail(TT_ERR_BAD_SHAPE, "tt_index_build_from_bf16: N=%lld d=%d", (long long)N, d);
    if (N > 0 && (!D_bf16 || !D32))
        return tt_fail(TT_ERR_BAD_SHAPE, "tt_index_build_from_bf16: null pointer");
    hipStream_t st = (hipStream_t)stream;
    if (stats && reset_stats)
        TT_RC_CHECK(tt_zero_async(stats, 2 * sizeof(float), st));
    if (N == 0)
        return TT_OK;
    const int64_t want_blocks = (N + 3) / 4;
    hipLaunchKernelGGL(build_from_bf16_kernel, dim3((unsigned)(want_blocks > 8192 ? 8192 : want_blocks)), dim3(256), 0,
                       st, (const unsigned short *)D_bf16, N, d, D32, (_Float16 *)D16, (unsigned *)stats);
    TT_LAUNCH_CHECK();
    return TT_OK;
}

// ---- the workspace of a screened call: over fp32 rows + fp16 shadow, over a bf16 corpus kept as bf16 (D_bf16 replaces
// D32 + D16, include/tt.h), and of the masked entries, which take either
TT_EXPORT size_t tt_score_topk_screened_workspace_bytes(int B, int64_t N, int d, int k)
{
    return splan_query(B, N, k, &SPlan::ws_bytes, fallback_ws_bytes(B, N, d, k, false));
}

TT_EXPORT size_t tt_score_topk_screened_bf16_workspace_bytes(int B, int64_t N, int d, int k)
{
    return splan_query(B, N, k, &SPlan::ws_bytes, fallback_ws_bytes(B, N, d, k, true));
}

TT_EXPORT size_t tt_score_topk_screened_masked_workspace_bytes(int B, int64_t N, int d, int k, int bf16)
{
    return splan_query(B, N, k, &SPlan::ws_bytes, fallback_ws_bytes(B, N, d, k, bf16 != 0));
}

// Where a finished screened search left its per-query statistics in the caller's workspace: int32 [B][2] = (pooled
// candidates, survivors within 2 eps of the k-th best approximate score) -- how much the filter let through on THIS data
// (bench.py reports it for encoder-produced corpora; queries recomputed by the exact fallback keep the screen's counts).
TT_EXPORT size_t tt_score_topk_screened_stats_offset(int B, int64_t N, int d, int k)
{
    (void)d;
    return splan_query(B, N, k, &SPlan::stats_off, 0);
}

namespace {
__global__ void seed_fill_kernel(float *seed, int n)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n)
        seed[i] = -3.0e38f; // no sample pass for this corpus size: no information (the floor threshold applies)
}

// What one screened call does, and with it which steps `screened` runs:
//                  query image   sample pass (plans with one), thresholds            main pass, finish, fallback
//   Whole          yes           k-th largest maximum -> the workspace               yes, under the workspace's thresholds
//   SeedThreshold  yes           k_seed-th largest -> seed[q]; no sample: filled     -
//   SeedList       yes           the k_seed largest -> seed[q][..]; no sample: filled -
//   Seeded         -             -                                                   yes, under the caller's seed[]
enum class Phase {
    Whole,         // the whole search
    SeedThreshold, // query image + sample pass; seed[q] <- the k_seed-th largest sample maximum (nothing else)
    SeedList,      // the same, but seed[q][0..k_seed) <- the k_seed LARGEST sample maxima, unordered (a shard's share of the
                   // union seed: tt_seed_union_f32)
    Seeded,        // the screen with the caller's seed[] as thresholds (the workspace still holds the seed phase's query
                   // image and flags), finish, predicated exact kernels
};

// One screened call as its entry point received it, in the four runs of arguments every entry has: an entry hands over four
// short braced lists of different types, not twenty positional arguments.
struct QueryArgs { const float *Q; int B, d, k; float dmax_norm; };
struct RowArgs {
    const void *D16; // the rows the screen reads: the fp16 shadow, or the bf16 corpus (converted in LDS)
    const void *D32; // the rows the finish kernel and the fallback read: fp32, or the same bf16 corpus (they widen it); the seed
                     // phases read none
    bool bf16;
    int64_t N;
    // keep-bitmask of the masked entries (nullptr: the unmasked search, launch for launch): the sample pass and the main pass run
    // their MASKED instantiations, the finish kernel sees kept documents only, the fallback is the masked exact search
    const unsigned *keep;
};
struct OutArgs { int64_t idx_offset; float *out_val; int64_t *out_idx; void *const *prof_events; }; // (all zero in the seed phases)
struct ScratchArgs { int32_t *fallback_flag; void *workspace; size_t workspace_bytes; hipStream_t stream; };
struct ScreenedCall : QueryArgs, RowArgs, OutArgs, ScratchArgs {
    const char *who; // the exported name of the entry that was called: every message starts with it
    Phase phase;
    int k_seed;  // the seed phases: which sample maxima become the seed (otherwise k)
    float *seed; // written by SeedThreshold [B] and SeedList [B][k_seed], read by Seeded [B]; Whole: nullptr
};

RowArgs f32_rows(const float *D32, const void *D16, int64_t N, const unsigned *keep) { return {D16, D32, false, N, keep}; }
RowArgs bf16_rows(const void *D_bf16, int64_t N, const unsigned *keep) { return {D_bf16, D_bf16, true, N, keep}; }

// Every argument check of a screened call, once; what lies below trusts them.  TT_OK: *pl is the call's plan.
int screened_validate(const ScreenedCall &c, SPlan *pl)
{
    const char *who = c.who;
    if (c.B <= 0 || c.N <= 0 || c.k <= 0) // (B == 0 is refused here; the exact entries answer TT_OK to it)
        return tt_fail(TT_ERR_BAD_SHAPE, "%s: B=%d N=%lld k=%d", who, c.B, (long long)c.N, c.k);
    if (c.d != 256)
        return tt_fail(TT_ERR_UNSUPPORTED, "%s: d=%d (supported: 256)", who, c.d);
    if (c.k > 64)
        return tt_fail(TT_ERR_UNSUPPORTED, "%s: k=%d > 64", who, c.k);
    if (c.N >= (int64_t)INT_MAX - 64)
        return tt_fail(TT_ERR_UNSUPPORTED, "%s: N too large; shard the corpus", who);
    if (!(c.dmax_norm >= 0.0f) || !(c.dmax_norm < 60000.0f))
        return tt_fail(TT_ERR_UNSUPPORTED, "%s: corpus norm %g outside the fp16 range", who, c.dmax_norm);
    const bool seed_only = c.phase == Phase::SeedThreshold || c.phase == Phase::SeedList;
    if (!c.Q || !c.D16 || !c.fallback_flag || (!seed_only && (!c.D32 || !c.out_val || !c.out_idx)) ||
        (c.phase != Phase::Whole && !c.seed))
        return tt_fail(TT_ERR_BAD_SHAPE, "%s: null pointer", who);
    if (seed_only && (c.k_seed < 1 || c.k_seed > c.k))
        return tt_fail(TT_ERR_BAD_SHAPE, "%s: k_seed=%d outside [1, k=%d]", who, c.k_seed, c.k);
    if ((uintptr_t)c.keep & 3)
        return tt_fail(TT_ERR_BAD_SHAPE, "%s: keep must be 4-byte aligned", who);
    *pl = make_splan(c.B, c.N, c.k);
    const size_t need = pl->ws_bytes + fallback_ws_bytes(c.B, c.N, c.d, c.k, c.bf16);
    // (a missing or misaligned workspace, and misaligned bf16 rows, are all reported as a workspace that is too small, in a
    //  message that may then compare a size with itself; the fp16 shadow has no alignment check.  Callers match the code.)
    if (!c.workspace || c.workspace_bytes < need || ((uintptr_t)c.workspace & 255) || (c.bf16 && ((uintptr_t)c.D16 & 15)))
        return tt_fail(TT_ERR_WORKSPACE, "%s: workspace %zu < %zu bytes", who, c.workspace_bytes, need);
    return TT_OK;
}

// ScreenParams is filled here and nowhere else: what every screen launch over pl's cut of the corpus reads.  What stays at its
// initialiser is not used by a launch until the step that needs it sets it.
ScreenParams screen_params(const ScreenedCall &c, const SPlan &pl)
{
    char *ws = (char *)c.workspace;
    ScreenParams sp;
    sp.Q = c.Q;
    sp.D16 = (const _Float16 *)c.D16;
    sp.B = c.B;
    sp.N = (int)c.N;
    sp.k = c.k;
    sp.n_chunks = pl.n_chunks;
    sp.tiles_per_chunk = pl.tiles_per_chunk;
    sp.n_tiles = pl.n_tiles;
    sp.static_tiles = pl.static_tiles;
    sp.tail_g = pl.tail_g;
    sp.tail_blocks = pl.tail_blocks;
    sp.dmax = c.dmax_norm;
    sp.flag = c.fallback_flag;
    sp.thr0_stride = c.k; // (read with thr0 only: main_pass)
    sp.qimg = (const h8 *)(ws + pl.qimg_off);
    sp.qnorm = (const float *)(ws + pl.qnorm_off);
    sp.keep = c.keep;
    return sp;
}

// ... and the buffers of a search: candidates and their counts, the pool counters, the ladders
ScreenParams search_params(const ScreenedCall &c, const SPlan &pl)
{
    char *ws = (char *)c.workspace;
    ScreenParams sp = screen_params(c, pl);
    sp.tail_ctr = (int *)(ws + pl.tailctr_off);
    // (the sample pass never reads it; a plan without a sample has a seed only when the caller brings one)
    sp.hist = pl.refresh && (pl.sample || c.phase == Phase::Seeded) ? (unsigned *)(ws + pl.hist_off) : nullptr;
    sp.cand = (SCand *)(ws + pl.cand_off);
    sp.pcnt = (int *)(ws + pl.pcnt_off);
    return sp;
}

// Query image and norms; resets the fallback flags, the pool counters and the ladders.
// (the flags are initialised by a kernel, not hipMemsetAsync: a 16-byte-multiple memset node captured in a HIP graph came back
//  with garbage from the second replay on; ROCm 7.2, found with GraphedSearch at B=128)
int query_image(const ScreenedCall &c, const SPlan &pl)
{
    char *ws = (char *)c.workspace;
    hipLaunchKernelGGL(q_image_kernel, dim3(pl.rows_pad / 32), dim3(128), 0, c.stream, c.Q, c.B, (h8 *)(ws + pl.qimg_off),
                       (float *)(ws + pl.qnorm_off), c.fallback_flag, (c.B + 31) / 32, (int *)(ws + pl.tailctr_off),
                       pl.n_qgroups, pl.hist_off ? (unsigned *)(ws + pl.hist_off) : nullptr);
    TT_LAUNCH_CHECK();
    return TT_OK;
}

float *sample_values(const ScreenedCall &c, const SPlan &pl) { return (float *)((char *)c.workspace + pl.smax_val_off); } // [rows][s_vals]

// The sample pass's launch: the search's over the first s_docs rows (masked: the first s_tiles words of the mask), everything
// static, maxima into s_val instead of candidates
ScreenParams sample_params(ScreenParams ss, const SPlan &pl, float *s_val)
{
    ss.N = (int)pl.s_docs;
    ss.n_tiles = pl.s_tiles;
    ss.n_chunks = pl.s_chunks;
    ss.tiles_per_chunk = pl.s_tiles_per_chunk;
    ss.static_tiles = pl.s_tiles;
    ss.tail_blocks = 0;
    (pl.s_onchip ? ss.top_val : ss.max_val) = s_val;
    return ss;
}

int sample_pass(const ScreenedCall &c, const SPlan &pl, const ScreenParams &sp)
{
    return launch_screen(pl, sample_params(sp, pl, sample_values(c, pl)), c.bf16, c.stream);
}

// From the sample maxima: the k-th largest per query into the workspace (Whole) or the k_seed-th largest into seed[]
// (SeedThreshold), or the k_seed largest into seed[] (SeedList).  A plan without a sample has nothing to select from: the
// seed phases fill seed[] with the floor, the whole search runs without thresholds.
int select_thresholds(const ScreenedCall &c, const SPlan &pl)
{
    const bool list = c.phase == Phase::SeedList;
    if (!pl.sample) {
        if (c.phase == Phase::Whole)
            return TT_OK;
        const int n = list ? c.B * c.k_seed : c.B;
        hipLaunchKernelGGL(seed_fill_kernel, dim3((n + 255) / 256), dim3(256), 0, c.stream, c.seed, n);
        TT_LAUNCH_CHECK();
        return TT_OK;
    }
    if (list)
        return tt_k_largest_list(sample_values(c, pl), c.B, pl.s_vals, c.k_seed, c.seed, c.stream);
    float *thr = c.phase == Phase::SeedThreshold ? c.seed : (float *)((char *)c.workspace + pl.sthr_val_off);
    return tt_kth_largest(sample_values(c, pl), c.B, pl.s_vals, c.phase == Phase::SeedThreshold ? c.k_seed : c.k, thr, c.stream);
}

// The main pass between the two profiling events, under the caller's seed (Seeded), the sample's thresholds, or none
int main_pass(const ScreenedCall &c, const SPlan &pl, ScreenParams sp)
{
    if (c.phase == Phase::Seeded || pl.sample) {
        sp.thr0 = c.phase == Phase::Seeded ? c.seed : (const float *)((char *)c.workspace + pl.sthr_val_off);
        sp.thr0_stride = 1;
    }
    if (c.prof_events)
        TT_HIP_CHECK(hipEventRecord((hipEvent_t)c.prof_events[0], c.stream));
    TT_RC_CHECK(launch_screen(pl, sp, c.bf16, c.stream));
    if (c.prof_events)
        TT_HIP_CHECK(hipEventRecord((hipEvent_t)c.prof_events[1], c.stream));
    return TT_OK;
}

// FinishParams is filled here and nowhere else.
int finish(const ScreenedCall &c, const SPlan &pl)
{
    char *ws = (char *)c.workspace;
    FinishParams fp;
    fp.Q = c.Q;
    fp.D32 = c.bf16 ? nullptr : (const float *)c.D32;
    fp.Dbf = c.bf16 ? (const unsigned *)c.D32 : nullptr;
    fp.B = c.B;
    fp.N = (int)c.N;
    fp.k = c.k;
    fp.n_chunks = pl.n_chunks;
    fp.q_per_block = pl.q_per_block;
    fp.dmax = c.dmax_norm;
    fp.cand = (const SCand *)(ws + pl.cand_off);
    fp.pcnt = (const int *)(ws + pl.pcnt_off);
    fp.flag = c.fallback_flag;
    fp.idx_offset = c.idx_offset;
    fp.out_val = c.out_val;
    fp.out_idx = c.out_idx;
    fp.stats = (int *)(ws + pl.stats_off);
    hipLaunchKernelGGL(screen_finish_kernel, dim3(c.B), dim3(256), (size_t)(2 * pl.n_chunks + 1) * sizeof(int), c.stream, fp);
    TT_LAUNCH_CHECK();
    return TT_OK;
}

// The exact k <= 64 search (masked under c.keep) in the workspace behind the screen's, predicated on the fallback flags: a
// no-op unless a workgroup raised one; then it rewrites every output row of the flagged 32-query tiles.  Its refusals carry
// the name of the public entry it stands for.
int fallback(const ScreenedCall &c, const SPlan &pl)
{
    const char *who = c.keep ? (c.bf16 ? "tt_score_topk_masked_bf16" : "tt_score_topk_masked_f32")
                             : (c.bf16 ? "tt_score_topk_bf16" : "tt_score_topk_f32");
    return exact_small(ExactCall{c.Q, c.B, c.d, c.D32, c.bf16, c.N, c.k, c.idx_offset, c.keep, c.out_val, c.out_idx,
                                 (char *)c.workspace + pl.ws_bytes, c.workspace_bytes - pl.ws_bytes, c.stream, who},
                       c.fallback_flag);
}

// One screened call: the Phase table above, step by step.
int screened(const ScreenedCall &c)
{
    SPlan pl;
    TT_RC_CHECK(screened_validate(c, &pl));
    const ScreenParams sp = search_params(c, pl);
    if (c.phase != Phase::Seeded) { // (Seeded: the workspace holds the seed phase's query image, the thresholds are seed[])
        TT_RC_CHECK(query_image(c, pl));
        if (pl.sample)
            TT_RC_CHECK(sample_pass(c, pl, sp));
        TT_RC_CHECK(select_thresholds(c, pl));
    }
    if (c.phase == Phase::SeedThreshold || c.phase == Phase::SeedList)
        return TT_OK;
    TT_RC_CHECK(main_pass(c, pl, sp));
    TT_RC_CHECK(finish(c, pl));
    return fallback(c, pl);
}

// The entries of one phase differ in their name, their rows and their mask only.
int whole_call(const char *who, const QueryArgs &q, const RowArgs &rows, const OutArgs &out, const ScratchArgs &s)
{
    return screened(ScreenedCall{q, rows, out, s, who, Phase::Whole, q.k, nullptr});
}

int seed_list_call(const char *who, const QueryArgs &q, const RowArgs &rows, int k_seed, float *list, const ScratchArgs &s)
{
    return screened(ScreenedCall{q, rows, OutArgs{}, s, who, Phase::SeedList, k_seed, list});
}

int seeded_call(const char *who, const QueryArgs &q, const RowArgs &rows, const OutArgs &out, const float *seed, const ScratchArgs &s)
{
    return screened(ScreenedCall{q, rows, out, s, who, Phase::Seeded, q.k, (float *)seed});
}
} // namespace

TT_EXPORT int tt_index_stats_bf16(const void *D_bf16, int64_t N, int d, float *stats, int reset_stats, tt_stream_t stream)
{
    hipStream_t st = (hipStream_t)stream;
    if (N < 0 || d <= 0 || d % 4 != 0 || d > 4096)
        return tt_fail(TT_ERR_BAD_SHAPE, "tt_index_stats_bf16: N=%lld d=%d", (long long)N, d);
    if (!stats || (N > 0 && !D_bf16))
        return tt_fail(TT_ERR_BAD_SHAPE, "tt_index_stats_bf16: null pointer");
    if (reset_stats)
        TT_RC_CHECK(tt_zero_async(stats, 2 * sizeof(float), st));
    if (N == 0)
        return TT_OK;
    const int64_t want_blocks = (N + 3) / 4;
    hipLaunchKernelGGL(build_from_bf16_kernel, dim3((unsigned)(want_blocks > 8192 ? 8192 : want_blocks)), dim3(256), 0,
                       st, (const unsigned short *)D_bf16, N, d, (float *)nullptr, (_Float16 *)nullptr, (unsigned *)stats);
    TT_LAUNCH_CHECK();
    return TT_OK;
}

// ---- over fp32 rows and their fp16 shadow
TT_EXPORT int tt_score_topk_screened_f32(const float *Q, int B, int d, const float *D32, const void *D16, int64_t N,
                                         int k, float dmax_norm, int64_t idx_offset, float *out_val, int64_t *out_idx,
                                         int32_t *fallback_flag, void *workspace, size_t workspace_bytes,
                                         void *const *prof_events, tt_stream_t stream)
{
    return whole_call("tt_score_topk_screened_f32", {Q, B, d, k, dmax_norm}, f32_rows(D32, D16, N, nullptr),
                 {idx_offset, out_val, out_idx, prof_events}, {fallback_flag, workspace, workspace_bytes, (hipStream_t)stream});
}

TT_EXPORT int tt_score_topk_screened_seed_f32(const float *Q, int B, int d, const void *D16, int64_t N, int k, int k_seed,
                                              float dmax_norm, int32_t *fallback_flag, float *seed, void *workspace,
                                              size_t workspace_bytes, tt_stream_t stream)
{
    return screened(ScreenedCall{{Q, B, d, k, dmax_norm}, f32_rows(nullptr, D16, N, nullptr), OutArgs{},
                                 {fallback_flag, workspace, workspace_bytes, (hipStream_t)stream},
                                 "tt_score_topk_screened_seed_f32", Phase::SeedThreshold, k_seed, seed});
}

TT_EXPORT int tt_score_topk_screened_seed_list_f32(const float *Q, int B, int d, const void *D16, int64_t N, int k, int k_seed,
                                                   float dmax_norm, int32_t *fallback_flag, float *seed_list, void *workspace,
                                                   size_t workspace_bytes, tt_stream_t stream)
{
    return seed_list_call("tt_score_topk_screened_seed_list_f32", {Q, B, d, k, dmax_norm}, f32_rows(nullptr, D16, N, nullptr), k_seed,
                       seed_list, {fallback_flag, workspace, workspace_bytes, (hipStream_t)stream});
}

TT_EXPORT int tt_score_topk_screened_seeded_f32(const float *Q, int B, int d, const float *D32, const void *D16, int64_t N,
                                                int k, float dmax_norm, int64_t idx_offset, float *out_val, int64_t *out_idx,
                                                int32_t *fallback_flag, const float *seed, void *workspace,
                                                size_t workspace_bytes, void *const *prof_events, tt_stream_t stream)
{
    return seeded_call("tt_score_topk_screened_seeded_f32", {Q, B, d, k, dmax_norm}, f32_rows(D32, D16, N, nullptr),
                  {idx_offset, out_val, out_idx, prof_events}, seed, {fallback_flag, workspace, workspace_bytes, (hipStream_t)stream});
}

// ---- the same over a bf16 corpus kept as bf16: D_bf16 replaces D32 + D16 (include/tt.h)
TT_EXPORT int tt_score_topk_screened_bf16(const float *Q, int B, int d, const void *D_bf16, int64_t N, int k, float dmax_norm,
                                          int64_t idx_offset, float *out_val, int64_t *out_idx, int32_t *fallback_flag,
                                          void *workspace, size_t workspace_bytes, void *const *prof_events, tt_stream_t stream)
{
    return whole_call("tt_score_topk_screened_bf16", {Q, B, d, k, dmax_norm}, bf16_rows(D_bf16, N, nullptr),
                 {idx_offset, out_val, out_idx, prof_events}, {fallback_flag, workspace, workspace_bytes, (hipStream_t)stream});
}

TT_EXPORT int tt_score_topk_screened_seed_list_bf16(const float *Q, int B, int d, const void *D_bf16, int64_t N, int k,
                                                    int k_seed, float dmax_norm, int32_t *fallback_flag, float *seed_list,
                                                    void *workspace, size_t workspace_bytes, tt_stream_t stream)
{
    return seed_list_call("tt_score_topk_screened_seed_list_bf16", {Q, B, d, k, dmax_norm}, bf16_rows(D_bf16, N, nullptr), k_seed,
                       seed_list, {fallback_flag, workspace, workspace_bytes, (hipStream_t)stream});
}

TT_EXPORT int tt_score_topk_screened_seeded_bf16(const float *Q, int B, int d, const void *D_bf16, int64_t N, int k,
                                                 float dmax_norm, int64_t idx_offset, float *out_val, int64_t *out_idx,
                                                 int32_t *fallback_flag, const float *seed, void *workspace,
                                                 size_t workspace_bytes, void *const *prof_events, tt_stream_t stream)
{
    return seeded_call("tt_score_topk_screened_seeded_bf16", {Q, B, d, k, dmax_norm}, bf16_rows(D_bf16, N, nullptr),
                  {idx_offset, out_val, out_idx, prof_events}, seed, {fallback_flag, workspace, workspace_bytes, (hipStream_t)stream});
}

// ---- the same six calls under a keep-bitmask (include/tt.h "Masked screened search"); keep == NULL is the unmasked call
TT_EXPORT int tt_score_topk_screened_masked_f32(const float *Q, int B, int d, const float *D32, const void *D16, int64_t N,
                                                const uint32_t *keep, int k, float dmax_norm, int64_t idx_offset, float *out_val,
                                                int64_t *out_idx, int32_t *fallback_flag, void *workspace, size_t workspace_bytes,
                                                void *const *prof_events, tt_stream_t stream)
{
    return whole_call("tt_score_topk_screened_masked_f32", {Q, B, d, k, dmax_norm}, f32_rows(D32, D16, N, keep),
                 {idx_offset, out_val, out_idx, prof_events}, {fallback_flag, workspace, workspace_bytes, (hipStream_t)stream});
}

TT_EXPORT int tt_score_topk_screened_masked_bf16(const float *Q, int B, int d, const void *D_bf16, int64_t N, const uint32_t *keep,
                                                 int k, float dmax_norm, int64_t idx_offset, float *out_val, int64_t *out_idx,
                                                 int32_t *fallback_flag, void *workspace, size_t workspace_bytes,
                                                 void *const *prof_events, tt_stream_t stream)
{
    return whole_call("tt_score_topk_screened_masked_bf16", {Q, B, d, k, dmax_norm}, bf16_rows(D_bf16, N, keep),
                 {idx_offset, out_val, out_idx, prof_events}, {fallback_flag, workspace, workspace_bytes, (hipStream_t)stream});
}

TT_EXPORT int tt_score_topk_screened_seed_list_masked_f32(const float *Q, int B, int d, const void *D16, int64_t N,
                                                          const uint32_t *keep, int k, int k_seed, float dmax_norm,
                                                          int32_t *fallback_flag, float *seed_list, void *workspace,
                                                          size_t workspace_bytes, tt_stream_t stream)
{
    return seed_list_call("tt_score_topk_screened_seed_list_masked_f32", {Q, B, d, k, dmax_norm}, f32_rows(nullptr, D16, N, keep), k_seed,
                       seed_list, {fallback_flag, workspace, workspace_bytes, (hipStream_t)stream});
}

TT_EXPORT int tt_score_topk_screened_seed_list_masked_bf16(const float *Q, int B, int d, const void *D_bf16, int64_t N,
                                                           const uint32_t *keep, int k, int k_seed, float dmax_norm,
                                                           int32_t *fallback_flag, float *seed_list, void *workspace,
                                                           size_t workspace_bytes, tt_stream_t stream)
{
    return seed_list_call("tt_score_topk_screened_seed_list_masked_bf16", {Q, B, d, k, dmax_norm}, bf16_rows(D_bf16, N, keep), k_seed,
                       seed_list, {fallback_flag, workspace, workspace_bytes, (hipStream_t)stream});
}

TT_EXPORT int tt_score_topk_screened_seeded_masked_f32(const float *Q, int B, int d, const float *D32, const void *D16, int64_t N,
                                                       const uint32_t *keep, int k, float dmax_norm, int64_t idx_offset,
                                                       float *out_val, int64_t *out_idx, int32_t *fallback_flag, const float *seed,
                                                       void *workspace, size_t workspace_bytes, void *const *prof_events,
                                                       tt_stream_t stream)
{
    return seeded_call("tt_score_topk_screened_seeded_masked_f32", {Q, B, d, k, dmax_norm}, f32_rows(D32, D16, N, keep),
                  {idx_offset, out_val, out_idx, prof_events}, seed, {fallback_flag, workspace, workspace_bytes, (hipStream_t)stream});
}

TT_EXPORT int tt_score_topk_screened_seeded_masked_bf16(const float *Q, int B, int d, const void *D_bf16, int64_t N,
                                                        const uint32_t *keep, int k, float dmax_norm, int64_t idx_offset,
                                                        float *out_val, int64_t *out_idx, int32_t *fallback_flag,
                                                        const float *seed, void *workspace, size_t workspace_bytes,
                                                        void *const *prof_events, tt_stream_t stream)
{
    return seeded_call("tt_score_topk_screened_seeded_masked_bf16", {Q, B, d, k, dmax_norm}, bf16_rows(D_bf16, N, keep),
                  {idx_offset, out_val, out_idx, prof_events}, seed, {fallback_flag, workspace, workspace_bytes, (hipStream_t)stream});
}

// ------------------------------------------------------------------ test-only: observe the screen's raw scores
// include/tt_debug.h.  Runs the REAL screen kernels (q_image_kernel + the MAXONLY form of screen_stream_kernel /
// screen_kernel<.,NSET>) over the whole corpus and returns one value per (query, 32-document tile): the tile
// maximum of s16 (thr == NULL: accumulators start at +0, the sample pass's arithmetic) or of
// t = fl(sum - thr[query]) (accumulators start at -thr, the main pass's arithmetic).  A test that fills every tile
// with 32 copies of one document reads that document's value.  Not bound by the Python package.
namespace {
// An SPlan with the caller's form in place of make_splan's choice, and a workspace of its own: query image, norms, flags.
// form 0: streaming, 32 queries per wave; form 1, 2, 4: shared-tile with that many query sets per wave.  The chunks are
// make_splan's without its finish-pool bound (there is no finish kernel here) and without the tail pool; what a search alone
// needs stays zero.  False: no such plan (the size query answers 0).
struct DbgPlan {
    SPlan s;
    size_t flag_off;
};
bool make_dbg_plan(int B, int64_t N, int form, DbgPlan *dp)
{
    if (B <= 0 || N <= 0 || (form != 0 && form != 1 && form != 2 && form != 4))
        return false;
    SPlan pl = {};
    pl.stream = form == 0;
    pl.nset = form;
    pl.q_per_block = form == 0 ? 32 : SW * 16 * form;
    pl.n_qgroups = (B + pl.q_per_block - 1) / pl.q_per_block;
    pl.rows_pad = pl.n_qgroups * pl.q_per_block;
    pl.n_tiles = (int)((N + 31) / 32);
    const TTChunks c = tt_chunks(pl.n_tiles, one_round(pl.stream, pl.n_qgroups), INT_MAX);
    pl.tiles_per_chunk = c.tiles_per_chunk;
    pl.n_chunks = c.n_chunks;
    pl.static_tiles = pl.n_tiles; // everything static
    pl.tail_g = 1;
    TTWorkspace ws;
    pl.qimg_off = ws.take((size_t)pl.rows_pad * 256 * sizeof(_Float16));
    pl.qnorm_off = ws.take((size_t)pl.rows_pad * sizeof(float));
    dp->flag_off = ws.take((size_t)(pl.rows_pad / 32 + 1) * sizeof(int));
    pl.ws_bytes = ws.off;
    dp->s = pl;
    return true;
}

// (both entries answer under the first one's name)
int debug_screen(const QueryArgs &q, const RowArgs &rows, const ScratchArgs &s, const float *thr, int form, float *out_t)
{
    DbgPlan dp;
    if (rows.N >= (int64_t)INT_MAX - 64 || !make_dbg_plan(q.B, rows.N, form, &dp))
        return tt_fail(TT_ERR_BAD_SHAPE, "tt_debug_screen_s16: B=%d N=%lld form=%d", q.B, (long long)rows.N, form);
    if (!q.Q || !rows.D16 || !out_t)
        return tt_fail(TT_ERR_BAD_SHAPE, "tt_debug_screen_s16: null pointer");
    if (!s.workspace || s.workspace_bytes < dp.s.ws_bytes || ((uintptr_t)s.workspace & 255))
        return tt_fail(TT_ERR_WORKSPACE, "tt_debug_screen_s16: workspace %zu < %zu bytes", s.workspace_bytes, dp.s.ws_bytes);
    char *ws = (char *)s.workspace;
    ScreenParams sp = screen_params(ScreenedCall{q, rows, OutArgs{}, s, "tt_debug_screen_s16", Phase::Whole, q.k, nullptr}, dp.s);
    sp.flag = (int *)(ws + dp.flag_off);
    sp.max_val = out_t; // [B][n_tiles]
    sp.dbg_thr = thr;
    hipLaunchKernelGGL(q_image_kernel, dim3(dp.s.rows_pad / 32), dim3(128), 0, s.stream, q.Q, q.B, (h8 *)(ws + dp.s.qimg_off),
                       (float *)(ws + dp.s.qnorm_off), sp.flag, dp.s.rows_pad / 32, (int *)nullptr, 0, (unsigned *)nullptr);
    TT_LAUNCH_CHECK();
    return launch_screen(dp.s, sp, rows.bf16, s.stream);
}
} // namespace

TT_EXPORT size_t tt_debug_screen_s16_workspace_bytes(int B, int64_t N, int form)
{
    DbgPlan dp;
    return make_dbg_plan(B, N, form, &dp) ? dp.s.ws_bytes : 0;
}

TT_EXPORT int tt_debug_screen_s16(const float *Q, int B, const void *D16, int64_t N, float dmax_norm, const float *thr,
                                  int form, float *out_t, void *workspace, size_t workspace_bytes, tt_stream_t stream)
{
    return debug_screen({Q, B, 256, 1, dmax_norm}, {D16, nullptr, false, N, nullptr},
                        {nullptr, workspace, workspace_bytes, (hipStream_t)stream}, thr, form, out_t);
}

TT_EXPORT int tt_debug_screen_s16_bf16(const float *Q, int B, const void *D_bf16, int64_t N, float dmax_norm, const float *thr,
                                       int form, float *out_t, void *workspace, size_t workspace_bytes, tt_stream_t stream)
{
    return debug_screen({Q, B, 256, 1, dmax_norm}, {D_bf16, nullptr, true, N, nullptr},
                        {nullptr, workspace, workspace_bytes, (hipStream_t)stream}, thr, form, out_t);
}
