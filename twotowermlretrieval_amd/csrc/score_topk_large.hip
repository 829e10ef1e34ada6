// K4L / K4m: exact top-k for 64 < k <= TT_TOPK_LARGE_KMAX, and under a keep-bitmask, on the main pass of score_topk.hip.
#include "score_topk.h"
#include "after_words.h"

#include <limits.h>
#include <math.h>

// ===========================================================================
// K4L: exact top-k for 64 < k <= TT_TOPK_LARGE_KMAX (DESIGN.md "Large k").
//
// Tier 0  the main pass of score_topk.hip, unchanged, with per-(wave, query) lists of m = 64 (seeded with the k-th -- not the 64th --
//         largest sample maximum); t_q = max(k-th largest entry of the union of the lists, seed).  The chunks are disjoint, so
//         k distinct documents score >= t_q: t_q <= the exact k-th score.  A list is SATURATED when it holds m entries and its
//         smallest is >= t_q (>=: a full list may have dropped a document that ties t_q).  No saturated list -> the union holds
//         every document scoring >= t_q, and the answer is the union's top-k (lk_final_kernel).
// Tier 1  a query with a saturated list is rescanned (lk_scan_kernel: the same ascending fp32 FMA chain, so the same bits):
//         every document scoring >= t_q goes to a per-query buffer of LK_CAP entries; if they fit, its top-k is the answer.
// Tier 2  otherwise the k-th (score, index) key is narrowed down by radix histograms of the 63-bit composite key
//         (order key of the score << 31 | 2^31-1 - doc): each pass scans the corpus once and fixes 11 more bits; as soon as
//         the documents at or above the current key prefix fit the buffer, one more scan collects them.  The composite key
//         orders (score desc, index asc), so ties at the k-th score resolve to the lowest indices however many there are.
// Every decision is taken on the device: the LK_ROUNDS (scan, decide) launches run for every call and skip the queries (and
// the query tiles) with nothing to do.
// ===========================================================================
namespace {
constexpr int LK_M = 64;              // list length of the main pass
constexpr int LK_CAP = 4096;          // rescan buffer entries per query
constexpr int LK_BINS = 2048;         // 11-bit digits of the composite key
constexpr int LK_ROUNDS = 8;          // collect, up to 6 histogram passes (63 bits), collect
constexpr int LK_SCAN_DOCS = 128;     // documents per scan tile
constexpr int LK_SCAN_BLOCKS = 2048;  // scan grid (each block walks doc tiles with this stride)
constexpr int LSEL_THREADS = 1024;    // one block per row: a few blocks (small B) must still stream a 131 072-entry union fast

enum { LK_DONE = 0, LK_COLLECT = 1, LK_HIST = 2 };

struct LkState {
    unsigned long long lo;  // collect / count only documents whose composite key is >= lo
    unsigned long long P;   // histogram passes: the k-th key lies in [P, P + 2^s)
    long long above;        // documents with key >= lo above that range
    int cnt;                // COLLECT: documents appended (may exceed LK_CAP)
    int mode;
    int s;
    int pad;
};

__device__ __forceinline__ unsigned lk_key(float f)
{
    return order_key(f == 0.0f ? 0.0f : f); // -0 and +0 compare equal: one key
}

__device__ __forceinline__ unsigned long long lk_comp(float v, int n)
{
    return ((unsigned long long)lk_key(v) << 31) | (unsigned long long)(0x7fffffff - n);
}

// ---- row selection: the k best of a row's candidates, (score desc, index asc), sorted; tail (-inf, -1) -----------------
// Radix select of the k-th score key over the valid entries (idx >= 0), then -- only when the k-th score's tie group is larger
// than the places left -- a radix select of the index that closes it, then compaction into LDS and a bitonic sort.  Exact for
// any tie group size: nothing but the k survivors is ever held in LDS.
struct SegSource { // topk_merge_kernel's layout: candidate m of row b in segment m / seg_len
    const float *val;
    const int64_t *idx;
    int M, seg_len;
    size_t seg_stride;
    __device__ int len(int) const { return M; }
    __device__ void load(int b, int m, float &v, int64_t &i) const
    {
        const int sg = m / seg_len, wi = m - sg * seg_len;
        v = ((const float *)((const char *)val + (size_t)sg * seg_stride))[(size_t)b * seg_len + wi];
        i = ((const int64_t *)((const char *)idx + (size_t)sg * seg_stride))[(size_t)b * seg_len + wi];
    }
};

struct SearchSource { // tier 0: the union of the partial lists [rows][M]; tiers 1, 2: the query's rescan buffer
    const float *pval;
    const int64_t *pidx;
    int M;
    const Cand *buf;
    const LkState *st;
    const int *tier;
    int64_t idx_offset;
    __device__ int len(int b) const { return tier[b] == 0 ? M : min(st[b].cnt, LK_CAP); }
    __device__ void load(int b, int m, float &v, int64_t &i) const
    {
        if (tier[b] == 0) {
            v = pval[(size_t)b * M + m];
            i = pidx[(size_t)b * M + m];
        } else {
            const Cand c = buf[(size_t)b * LK_CAP + m];
            v = c.v;
            i = idx_offset + c.x;
        }
    }
};

// One wave (threads 0..63): pick the bin of 256 (4 per lane; high bins first when desc) in which the rank-th entry lies.
// sel[0] = bin, sel[1] = entries in bins before it, sel[2] = its count, sel[3] = the row's total.
__device__ __forceinline__ void lk_pick_bin(const int *hist, int rank, bool desc, int *sel)
{
    const int lane = threadIdx.x & 63;
    int c[4], s = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int bin = desc ? 255 - (lane * 4 + i) : lane * 4 + i;
        c[i] = hist[bin];
        s += c[i];
    }
    int incl = s;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int y = __shfl_up(incl, off);
        if (lane >= off)
            incl += y;
    }
    const int total = __shfl(incl, 63);
    int before = incl - s;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (before < rank && before + c[i] >= rank) {
            sel[0] = desc ? 255 - (lane * 4 + i) : lane * 4 + i;
            sel[1] = before;
            sel[2] = c[i];
        }
        before += c[i];
    }
    if (lane == 0)
        sel[3] = total;
}

template <class S>
__device__ void lk_select_row(const S &src, int b, int k, float *out_val, int64_t *out_idx)
{
    __shared__ int hist[256];
    __shared__ int sel[4];
    __shared__ int npos;
    __shared__ float sv[TT_TOPK_LARGE_KMAX];
    __shared__ int64_t si[TT_TOPK_LARGE_KMAX];
    const int tid = threadIdx.x;
    const int M = src.len(b);

    // 1. the k-th score key (kv = min(k, valid entries))
    unsigned prefix = 0u, mask = 0u;
    int krem = k, kv = 0, ties = 0;
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = 24 - 8 * pass;
        if (tid < 256)
            hist[tid] = 0;
        __syncthreads();
        for (int m = tid; m < M; m += LSEL_THREADS) {
            float v;
            int64_t i;
            src.load(b, m, v, i);
            const unsigned key = lk_key(v);
            if (i >= 0 && (key & mask) == prefix)
                atomicAdd(&hist[(key >> shift) & 255u], 1);
        }
        __syncthreads();
        if (tid < 64) {
            if (pass == 0) { // the first pass sees every valid entry: fewer than k -> take them all
                int s = 0;
                for (int j = tid; j < 256; j += 64)
                    s += hist[j];
                for (int off = 32; off >= 1; off >>= 1)
                    s += __shfl_xor(s, off);
                if (tid == 0)
                    npos = min(k, s);
            }
        }
        __syncthreads();
        if (pass == 0) {
            kv = npos;
            krem = kv;
            if (kv == 0)
                break; // block-uniform
        }
        if (tid < 64)
            lk_pick_bin(hist, krem, true, sel);
        __syncthreads();
        prefix |= (unsigned)sel[0] << shift;
        mask |= 0xffu << shift;
        krem -= sel[1];
        ties = sel[2];
        __syncthreads();
    }

    // 2. krem of the `ties` entries with the k-th key are taken: the krem lowest indices (radix select on the index)
    int64_t idx_cut = INT64_MAX; // take ties with idx < idx_cut, then copies of idx_cut up to kv
    int need_cut = 0;
    if (kv > 0 && ties > krem) {
        unsigned long long ip = 0ull, im = 0ull;
        int r = krem;
        for (int pass = 0; pass < 8; ++pass) {
            const int shift = 56 - 8 * pass;
            if (tid < 256)
                hist[tid] = 0;
            __syncthreads();
            for (int m = tid; m < M; m += LSEL_THREADS) {
                float v;
                int64_t i;
                src.load(b, m, v, i);
                if (i >= 0 && lk_key(v) == prefix && ((unsigned long long)i & im) == ip)
                    atomicAdd(&hist[((unsigned long long)i >> shift) & 255u], 1);
            }
            __syncthreads();
            if (tid < 64)
                lk_pick_bin(hist, r, false, sel);
            __syncthreads();
            ip |= (unsigned long long)sel[0] << shift;
            im |= 0xffull << shift;
            r -= sel[1];
            __syncthreads();
        }
        idx_cut = (int64_t)ip;
        need_cut = 1;
    }

    // 3. compaction: the strictly better entries first, then copies of the cut (identical pairs) up to kv
    if (tid == 0)
        npos = 0;
    __syncthreads();
    for (int phase = 0; phase <= need_cut && kv > 0; ++phase) {
        for (int m = tid; m < M; m += LSEL_THREADS) {
            float v;
            int64_t i;
            src.load(b, m, v, i);
            if (i < 0)
                continue;
            const unsigned key = lk_key(v);
            const bool take = phase == 0 ? (key > prefix || (key == prefix && i < idx_cut)) : (key == prefix && i == idx_cut);
            if (take) {
                const int slot = atomicAdd(&npos, 1);
                if (slot < kv) {
                    sv[slot] = v;
                    si[slot] = i;
                }
            }
        }
        __syncthreads();
    }

    // 4. bitonic sort of the kv survivors (padding ranks last), then out
    int P2 = 1;
    while (P2 < kv)
        P2 <<= 1;
    for (int t = kv + tid; t < P2; t += LSEL_THREADS) {
        sv[t] = -INFINITY;
        si[t] = INT64_MAX;
    }
    __syncthreads();
    for (int k2 = 2; k2 <= P2; k2 <<= 1) {
        for (int j2 = k2 >> 1; j2 > 0; j2 >>= 1) {
            for (int t = tid; t < P2; t += LSEL_THREADS) {
                const int l = t ^ j2;
                if (l > t) {
                    const bool up = (t & k2) == 0;
                    if (up == ranks_before(sv[l], si[l], sv[t], si[t])) {
                        const float fv = sv[t];
                        const int64_t fi = si[t];
                        sv[t] = sv[l];
                        si[t] = si[l];
                        sv[l] = fv;
                        si[l] = fi;
                    }
                }
            }
            __syncthreads();
        }
    }
    for (int t = tid; t < k; t += LSEL_THREADS) {
        out_val[(size_t)b * k + t] = t < kv ? sv[t] : -INFINITY;
        out_idx[(size_t)b * k + t] = t < kv ? si[t] : -1;
    }
}

__global__ __launch_bounds__(LSEL_THREADS) void lk_merge_kernel(SegSource src, int k, float *out_val, int64_t *out_idx)
{
    lk_select_row(src, blockIdx.x, k, out_val, out_idx);
}

__global__ __launch_bounds__(LSEL_THREADS) void lk_final_kernel(SearchSource src, int k, float *out_val, int64_t *out_idx)
{
    lk_select_row(src, blockIdx.x, k, out_val, out_idx);
}

// flags[t] = 1 when a list of 32-query tile t carries the give-up marker (tt_score_topk_f32's redo, before t_q is taken)
__global__ __launch_bounds__(256) void lk_marker_kernel(const int64_t *__restrict__ pidx, int B, int n_chunks, int *flags)
{
    const int q0 = blockIdx.x * 32;
    bool bad = false;
    for (int e = threadIdx.x; e < 32 * n_chunks; e += 256) {
        const int q = q0 + e / n_chunks;
        if (q < B && pidx[((size_t)q * n_chunks + e % n_chunks) * LK_M] >= (int64_t)TT_TOPK_INVALID_INDEX)
            bad = true;
    }
    bad = __syncthreads_or(bad);
    if (threadIdx.x == 0)
        flags[blockIdx.x] = bad ? 1 : 0;
}

// Tier decision per query: t_q = max(k-th largest entry of the union (-inf when it has fewer than k entries), seed);
// a saturated list -> rescan from t_q.  One block per query: a 4-pass radix select over the union, then the saturation test.
__global__ __launch_bounds__(LSEL_THREADS) void lk_analyze_kernel(const float *__restrict__ pval, const int64_t *__restrict__ pidx,
                                                                  int n_chunks, int k, const float *__restrict__ seed, LkState *st,
                                                                  int *tier)
{
    __shared__ int hist[256];
    __shared__ int sel[4];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int M = n_chunks * LK_M;
    const float *v = pval + (size_t)b * M;
    float t = -INFINITY;
    if (M >= k) { // the k-th largest of all M entries, padding (-inf) included: kth_largest_kernel's value
        unsigned prefix = 0u, mask = 0u;
        int krem = k;
        for (int pass = 0; pass < 4; ++pass) {
            const int shift = 24 - 8 * pass;
            if (tid < 256)
                hist[tid] = 0;
            __syncthreads();
            for (int m = tid; m < M; m += LSEL_THREADS) {
                const unsigned key = order_key(v[m]);
                if ((key & mask) == prefix)
                    atomicAdd(&hist[(key >> shift) & 255u], 1);
            }
            __syncthreads();
            if (tid < 64)
                lk_pick_bin(hist, krem, true, sel);
            __syncthreads();
            prefix |= (unsigned)sel[0] << shift;
            mask |= 0xffu << shift;
            krem -= sel[1];
            __syncthreads();
        }
        t = order_key_to_float(prefix);
    }
    if (seed)
        t = fmaxf(t, seed[b]);
    bool sat = false;
    for (int c = tid; c < n_chunks; c += LSEL_THREADS) {
        const size_t o = ((size_t)b * n_chunks + c) * LK_M;
        if (pidx[o + LK_M - 1] < 0)
            continue; // not full: it holds every document of its chunk above the seed
        float mn = INFINITY;
        for (int e = 0; e < LK_M; ++e)
            mn = fminf(mn, pval[o + e]);
        if (mn >= t)
            sat = true;
    }
    sat = __syncthreads_or(sat);
    if (tid == 0) {
        LkState s;
        s.lo = (unsigned long long)lk_key(t) << 31; // every document scoring >= t
        s.P = 0ull;
        s.above = 0;
        s.cnt = 0;
        s.mode = sat ? LK_COLLECT : LK_DONE;
        s.s = 63;
        s.pad = 0;
        st[b] = s;
        tier[b] = sat ? 1 : 0;
    }
}

// One corpus scan for the queries in COLLECT or HIST mode: 32-query x 128-document tiles, fp32 FMA chains over the features
// in ascending order (the bits of the main pass and of the oracle), thread = 4 queries x 4 documents.
// MASKED: documents whose keep bit is clear are neither collected nor counted (keep: one word per 32 documents).
template <bool BF, bool MASKED>
__global__ __launch_bounds__(256) void lk_scan_kernel(const float *__restrict__ Q, const void *__restrict__ D, int B, int d, int N,
                                                      LkState *st, Cand *buf, int *hist, const unsigned *__restrict__ keep)
{
    __shared__ __attribute__((aligned(16))) float qs[32][32];                // [feature][query]
    __shared__ __attribute__((aligned(16))) float ds[32][LK_SCAN_DOCS + 4];  // [feature][document]
    const int tid = threadIdx.x, qg = tid >> 5, dg = tid & 31;
    const int n_qt = (B + 31) / 32, n_dt = (N + LK_SCAN_DOCS - 1) / LK_SCAN_DOCS;
    for (int qt = 0; qt < n_qt; ++qt) {
        const bool live = tid < 32 && qt * 32 + tid < B && st[qt * 32 + tid].mode != LK_DONE;
        if (!__syncthreads_or(live))
            continue; // block-uniform
        int md[4], sh[4];
        unsigned long long lo[4], P[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int q = qt * 32 + qg * 4 + i;
            md[i] = LK_DONE;
            lo[i] = P[i] = 0ull;
            sh[i] = 0;
            if (q < B) {
                md[i] = st[q].mode;
                lo[i] = st[q].lo;
                P[i] = st[q].P;
                sh[i] = st[q].s;
            }
        }
        for (int dt = blockIdx.x; dt < n_dt; dt += gridDim.x) {
            // documents of this tile: rem of them from row0 on (64-bit: N may come within 65 of INT_MAX)
            const int64_t row0 = (int64_t)dt * LK_SCAN_DOCS;
            const int rem = (int)min((int64_t)LK_SCAN_DOCS, (int64_t)N - row0);
            const float *D32 = (const float *)D + row0 * d;
            const unsigned short *D16 = (const unsigned short *)D + row0 * d;
            float acc[4][4];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    acc[i][j] = 0.0f;
            // the thread's four documents row0 + 4 dg + j share a keep word (row0 is a multiple of 128): their bits, from bit 0
            unsigned kbits = 0xfu;
            if (MASKED && dg * 4 < rem)
                kbits = keep[(row0 + dg * 4) >> 5] >> ((dg * 4) & 31);
            for (int f0 = 0; f0 < d; f0 += 32) {
                __syncthreads();
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int e = tid + 256 * r, qi = e >> 5, fi = e & 31, q = qt * 32 + qi;
                    qs[fi][qi] = q < B ? Q[(size_t)q * d + f0 + fi] : 0.0f;
                }
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int e = tid + 256 * r, di = e >> 5, fi = e & 31;
                    float v = 0.0f;
                    if (di < rem) {
                        if (BF)
                            v = __uint_as_float((unsigned)D16[di * d + f0 + fi] << 16);
                        else
                            v = D32[di * d + f0 + fi];
                    }
                    ds[fi][di] = v;
                }
                __syncthreads();
#pragma unroll 8
                for (int f = 0; f < 32; ++f) {
                    const f32x4 a = *(const f32x4 *)&qs[f][qg * 4];
                    const f32x4 c = *(const f32x4 *)&ds[f][dg * 4];
#pragma unroll
                    for (int i = 0; i < 4; ++i)
#pragma unroll
                        for (int j = 0; j < 4; ++j)
                            acc[i][j] = fmaf(a[i], c[j], acc[i][j]);
                }
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (md[i] == LK_DONE)
                    continue;
                const int q = qt * 32 + qg * 4 + i;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (dg * 4 + j >= rem || (MASKED && !((kbits >> j) & 1u)))
                        continue;
                    const int n = (int)(row0 + dg * 4 + j); // < N

                    const unsigned long long comp = lk_comp(acc[i][j], n);
                    if (comp < lo[i])
                        continue;
                    if (md[i] == LK_COLLECT) {
                        const int slot = atomicAdd(&st[q].cnt, 1);
                        if (slot < LK_CAP) {
                            Cand c;
                            c.v = acc[i][j];
                            c.x = n;
                            buf[(size_t)q * LK_CAP + slot] = c;
                        }
                    } else if ((comp >> sh[i]) == (P[i] >> sh[i])) {
                        const int w = min(11, sh[i]);
                        atomicAdd(&hist[(size_t)q * LK_BINS + ((comp >> (sh[i] - w)) & ((1ull << w) - 1))], 1);
                    }
                }
            }
        }
    }
}

// After a scan: COLLECT that fit -> done; COLLECT that overflowed -> histogram passes; HIST -> fix the next digit, and collect
// as soon as the documents at or above the prefix fit the buffer.
__global__ __launch_bounds__(256) void lk_decide_kernel(LkState *st, int *tier, int *hist, int k)
{
    __shared__ int pre[256];
    __shared__ int sel[3];
    const int b = blockIdx.x, tid = threadIdx.x;
    LkState s = st[b];
    int *h = hist + (size_t)b * LK_BINS;
    if (s.mode == LK_DONE)
        return;
    bool zero = false;
    if (s.mode == LK_COLLECT) {
        if (s.cnt <= LK_CAP) {
            s.mode = LK_DONE;
        } else {
            s.mode = LK_HIST;
            s.P = 0ull;
            s.s = 63;
            s.above = 0;
            zero = true;
        }
    } else {
        const int w = min(11, s.s), nb = 1 << w;
        const long long krem = (long long)k - s.above;
        int c[8], sum = 0;
#pragma unroll
        for (int i = 0; i < 8; ++i) { // thread t: bins nb-1-8t .. nb-8-8t (high bins first)
            const int bin = nb - 1 - (tid * 8 + i);
            c[i] = bin >= 0 ? h[bin] : 0;
            sum += c[i];
        }
        pre[tid] = sum;
        if (tid == 0) {
            sel[0] = -1;
            sel[1] = 0;
            sel[2] = 0;
        }
        __syncthreads();
        if (tid == 0) {
            int run = 0;
            for (int t = 0; t < 256; ++t) {
                const int x = pre[t];
                pre[t] = run;
                run += x;
            }
        }
        __syncthreads();
        long long before = pre[tid];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            if (before < krem && before + c[i] >= krem) {
                sel[0] = nb - 1 - (tid * 8 + i);
                sel[1] = (int)before;
                sel[2] = c[i];
            }
            before += c[i];
        }
        __syncthreads();
        if (sel[0] < 0) { // (cannot happen: k documents score >= t_q) -- collect everything counted
            s.mode = LK_COLLECT;
            s.cnt = 0;
        } else {
            s.P |= (unsigned long long)sel[0] << (s.s - w);
            s.s -= w;
            s.above += sel[1];
            if (s.above + sel[2] <= LK_CAP) {
                s.mode = LK_COLLECT;
                s.lo = s.P > s.lo ? s.P : s.lo;
                s.cnt = 0;
            } else {
                zero = true;
            }
        }
    }
    if (zero)
        for (int i = tid; i < LK_BINS; i += 256)
            h[i] = 0;
    __syncthreads();
    if (tid == 0) {
        if (s.mode == LK_HIST)
            tier[b] = 2;
        st[b] = s;
    }
}

static_assert(LK_M == MERGE_KMAX, "the main pass under a large k keeps lists of the k <= 64 search's longest length");

// Workspace of a large-k search: the k = 64 plan's, then the large-k state.
struct LargePlan {
    bool small; // k <= 64: the call is tt_score_topk_f32 / _bf16's own
    size_t tier_off, st_off, buf_off, hist_off, ws_bytes;
};

// pl: make_plan for lists of min(k, LK_M)
LargePlan make_large_plan(const Plan &pl, int B, int k)
{
    LargePlan lp;
    lp.small = k <= LK_M;
    TTWorkspace ws;
    ws.off = tt_align_up(pl.ws_bytes, 256);
    const size_t rows = tt_align_up((size_t)B, 32);
    lp.tier_off = ws.take(rows * sizeof(int));
    if (lp.small) {
        lp.st_off = lp.buf_off = lp.hist_off = 0;
    } else {
        lp.st_off = ws.take(rows * sizeof(LkState));
        lp.buf_off = ws.take(rows * LK_CAP * sizeof(Cand));
        lp.hist_off = ws.take(rows * LK_BINS * sizeof(int));
    }
    lp.ws_bytes = ws.off;
    return lp;
}

// The workspace queries: false = no call of this shape
bool large_plan_of(int B, int64_t N, int d, int k, int bf16, LargePlan *lp)
{
    if (B <= 0 || N < 0 || k <= 0 || k > TT_TOPK_LARGE_KMAX)
        return false;
    *lp = make_large_plan(make_plan(B, N, k < LK_M ? k : LK_M, d, bf16 != 0), B, k);
    return true;
}

// the give-up redo of tt_score_topk_f32, on the lists themselves: a marker must never reach t_q
int flag_lists(const ExactCall &c, const Plan &pl, int *flags)
{
    hipLaunchKernelGGL(lk_marker_kernel, dim3(pl.main.n_qtiles), dim3(256), 0, c.stream,
                       (const int64_t *)((const char *)c.workspace + pl.pidx_off), c.B, pl.main.n_chunks, flags);
    TT_LAUNCH_CHECK();
    return TT_OK;
}

typedef void (*LkScan)(const float *, const void *, int, int, int, LkState *, Cand *, int *, const unsigned *);
const LkScan lk_scan[2][2] = {{lk_scan_kernel<false, false>, lk_scan_kernel<false, true>}, // [bf16 rows][keep]
                              {lk_scan_kernel<true, false>, lk_scan_kernel<true, true>}};

// The large and masked entries.
int score_topk_large(const ExactCall &c)
{
    Plan pl;
    const int rc = exact_validate(c, TT_TOPK_LARGE_KMAX, &pl);
    if (rc != TT_OK || c.B == 0)
        return rc;
    const LargePlan lp = make_large_plan(pl, c.B, c.k);
    const int B = c.B, k = c.k;
    const hipStream_t st = c.stream;
    char *ws = (char *)c.workspace;
    int *tier = (int *)(ws + lp.tier_off);
    TT_RC_CHECK(tt_zero_async(tier, (size_t)B * sizeof(int), st));
    if (lp.small)
        return score_topk_pred(c, pl, nullptr);
    if (c.N == 0) {
        SegSource src{nullptr, nullptr, 0, 1, 0};
        hipLaunchKernelGGL(lk_merge_kernel, dim3(B), dim3(LSEL_THREADS), 0, st, src, k, c.out_val, c.out_idx);
        TT_LAUNCH_CHECK();
        return TT_OK;
    }
    // tier 0: the k = 64 main pass, seeded with the k-th largest sample maximum
    TT_RC_CHECK(score_partials(c, pl, ExactPass{LK_M, nullptr, nullptr}));
    TT_RC_CHECK(redo_gave_up(c, pl, LK_M, flag_lists, false));
    const float *pval = (const float *)(ws + pl.pval_off);
    const int64_t *pidx = (const int64_t *)(ws + pl.pidx_off);
    const int M = pl.main.n_chunks * LK_M;
    LkState *sts = (LkState *)(ws + lp.st_off);
    Cand *buf = (Cand *)(ws + lp.buf_off);
    int *hist = (int *)(ws + lp.hist_off);
    hipLaunchKernelGGL(lk_analyze_kernel, dim3(B), dim3(LSEL_THREADS), 0, st, pval, pidx, pl.main.n_chunks, k,
                       pl.prepass ? (const float *)(ws + pl.pre_val_off) : (const float *)nullptr, sts, tier);
    TT_LAUNCH_CHECK();
    TT_RC_CHECK(tt_zero_async(hist, (size_t)B * LK_BINS * sizeof(int), st));
    // tiers 1 and 2: a fixed chain of (scan, decide) launches, each a no-op for the queries that are done
    const int n_dt = (int)((c.N + LK_SCAN_DOCS - 1) / LK_SCAN_DOCS);
    const int grid = n_dt < LK_SCAN_BLOCKS ? n_dt : LK_SCAN_BLOCKS;
    for (int r = 0; r < LK_ROUNDS; ++r) {
        hipLaunchKernelGGL(lk_scan[c.bf16][c.keep != nullptr], dim3(grid), dim3(256), 0, st, c.Q, c.D, B, c.d, (int)c.N, sts, buf,
                           hist, c.keep);
        TT_LAUNCH_CHECK();
        hipLaunchKernelGGL(lk_decide_kernel, dim3(B), dim3(256), 0, st, sts, tier, hist, k);
        TT_LAUNCH_CHECK();
    }
    SearchSource src{pval, pidx, M, buf, sts, tier, c.idx_offset};
    hipLaunchKernelGGL(lk_final_kernel, dim3(B), dim3(LSEL_THREADS), 0, st, src, k, c.out_val, c.out_idx);
    TT_LAUNCH_CHECK();
    return TT_OK;
}
} // namespace

size_t score_topk_large_ws_bytes(const Plan &pl, int B, int k)
{
    return make_large_plan(pl, B, k).ws_bytes;
}

TT_EXPORT size_t tt_score_topk_large_workspace_bytes(int B, int64_t N, int d, int k, int bf16)
{
    LargePlan lp;
    return large_plan_of(B, N, d, k, bf16, &lp) ? lp.ws_bytes : 0;
}

TT_EXPORT size_t tt_score_topk_large_tier_offset(int B, int64_t N, int d, int k, int bf16)
{
    LargePlan lp;
    return large_plan_of(B, N, d, k, bf16, &lp) ? lp.tier_off : (size_t)-1;
}

TT_EXPORT int tt_score_topk_large_f32(const float *Q, int B, int d, const float *D, int64_t N, int k, int64_t idx_offset,
                                      float *out_val, int64_t *out_idx, void *workspace, size_t workspace_bytes,
                                      tt_stream_t stream)
{
    return score_topk_large(ExactCall{Q, B, d, D, false, N, k, idx_offset, nullptr, out_val, out_idx, workspace, workspace_bytes,
                                      (hipStream_t)stream, "tt_score_topk_large_f32"});
}

TT_EXPORT int tt_score_topk_large_bf16(const float *Q, int B, int d, const void *D_bf16, int64_t N, int k, int64_t idx_offset,
                                       float *out_val, int64_t *out_idx, void *workspace, size_t workspace_bytes,
                                       tt_stream_t stream)
{
    return score_topk_large(ExactCall{Q, B, d, D_bf16, true, N, k, idx_offset, nullptr, out_val, out_idx, workspace,
                                      workspace_bytes, (hipStream_t)stream, "tt_score_topk_large_bf16"});
}

// ---- K4m: masked exact search (DESIGN.md "K4m") ------------------------------------------------------------------------------
// The large call with a keep-bitmask: the same plan, workspace and launches, on the MASKED instantiations.  keep == NULL is the
// unmasked call itself.
TT_EXPORT size_t tt_score_topk_masked_workspace_bytes(int B, int64_t N, int d, int k, int bf16)
{
    return tt_score_topk_large_workspace_bytes(B, N, d, k, bf16);
}

TT_EXPORT int tt_score_topk_masked_f32(const float *Q, int B, int d, const float *D, int64_t N, const uint32_t *keep, int k,
                                       int64_t idx_offset, float *out_val, int64_t *out_idx, void *workspace,
                                       size_t workspace_bytes, tt_stream_t stream)
{
    return score_topk_large(ExactCall{Q, B, d, D, false, N, k, idx_offset, keep, out_val, out_idx, workspace, workspace_bytes,
                                      (hipStream_t)stream, "tt_score_topk_masked_f32"});
}

TT_EXPORT int tt_score_topk_masked_bf16(const float *Q, int B, int d, const void *D_bf16, int64_t N, const uint32_t *keep, int k,
                                        int64_t idx_offset, float *out_val, int64_t *out_idx, void *workspace,
                                        size_t workspace_bytes, tt_stream_t stream)
{
    return score_topk_large(ExactCall{Q, B, d, D_bf16, true, N, k, idx_offset, keep, out_val, out_idx, workspace,
                                      workspace_bytes, (hipStream_t)stream, "tt_score_topk_masked_bf16"});
}

// ---- Tagged search (DESIGN.md "Tagged search") -------------------------------------------------------------------------------
// The masked call for k <= 64 with a per-query filter: the same plan, workspace and launches, on the TAGGED instantiations of the
// main and sample passes (score_topk.hip).  tags == match_mask == match_value == NULL is the masked call itself.
namespace {
int score_topk_tagged(ExactCall c)
{
    if (c.k > MERGE_KMAX)
        return tt_fail(TT_ERR_UNSUPPORTED, "%s: k=%d > %d (tagged search keeps the k <= 64 lists only)", c.who, c.k, MERGE_KMAX);
    const int given = (c.tags != nullptr) + (c.match_mask != nullptr) + (c.match_value != nullptr);
    if (given != 0 && given != 3)
        return tt_fail(TT_ERR_BAD_SHAPE, "%s: tags, match_mask and match_value must be all NULL or all non-NULL", c.who);
    // (tags: a tile's 128 bytes are read as two 16-word scalar loads)
    if (((uintptr_t)c.tags & 15) || (((uintptr_t)c.match_mask | (uintptr_t)c.match_value) & 3))
        return tt_fail(TT_ERR_BAD_SHAPE, "%s: tags must be 16-byte, match_mask and match_value 4-byte aligned", c.who);
    return score_topk_large(c);
}
} // namespace

TT_EXPORT size_t tt_score_topk_tagged_workspace_bytes(int B, int64_t N, int d, int k, int bf16)
{
    return k > MERGE_KMAX ? 0 : tt_score_topk_large_workspace_bytes(B, N, d, k, bf16);
}

TT_EXPORT int tt_score_topk_tagged_f32(const float *Q, int B, int d, const float *D, int64_t N, const uint32_t *tags,
                                       const uint32_t *match_mask, const uint32_t *match_value, const uint32_t *keep, int k,
                                       int64_t idx_offset, float *out_val, int64_t *out_idx, void *workspace,
                                       size_t workspace_bytes, tt_stream_t stream)
{
    return score_topk_tagged(ExactCall{Q, B, d, D, false, N, k, idx_offset, keep, out_val, out_idx, workspace, workspace_bytes,
                                       (hipStream_t)stream, "tt_score_topk_tagged_f32", false, tags, match_mask, match_value});
}

TT_EXPORT int tt_score_topk_tagged_bf16(const float *Q, int B, int d, const void *D_bf16, int64_t N, const uint32_t *tags,
                                        const uint32_t *match_mask, const uint32_t *match_value, const uint32_t *keep, int k,
                                        int64_t idx_offset, float *out_val, int64_t *out_idx, void *workspace,
                                        size_t workspace_bytes, tt_stream_t stream)
{
    return score_topk_tagged(ExactCall{Q, B, d, D_bf16, true, N, k, idx_offset, keep, out_val, out_idx, workspace, workspace_bytes,
                                       (hipStream_t)stream, "tt_score_topk_tagged_bf16", false, tags, match_mask, match_value});
}

// ---- Biased search (DESIGN.md "Biased search") -------------------------------------------------------------------------------
// The masked call for k <= 64 with a per-document score bias: the same plan, workspace and launches, on the BIASED
// instantiations of the main and sample passes (score_topk.hip).  bias == NULL is the masked call itself.
namespace {
int score_topk_biased(ExactCall c)
{
    if (c.k > MERGE_KMAX)
        return tt_fail(TT_ERR_UNSUPPORTED, "%s: k=%d > %d (biased search keeps the k <= 64 lists only)", c.who, c.k, MERGE_KMAX);
    // (a tile's 128 bytes are read as two 16-word scalar loads)
    if ((uintptr_t)c.bias & 15)
        return tt_fail(TT_ERR_BAD_SHAPE, "%s: bias must be 16-byte aligned", c.who);
    return score_topk_large(c);
}
} // namespace

TT_EXPORT size_t tt_score_topk_biased_workspace_bytes(int B, int64_t N, int d, int k, int bf16)
{
    return k > MERGE_KMAX ? 0 : tt_score_topk_large_workspace_bytes(B, N, d, k, bf16);
}

TT_EXPORT int tt_score_topk_biased_f32(const float *Q, int B, int d, const float *D, int64_t N, const float *bias,
                                       const uint32_t *keep, int k, int64_t idx_offset, float *out_val, int64_t *out_idx,
                                       void *workspace, size_t workspace_bytes, tt_stream_t stream)
{
    return score_topk_biased(ExactCall{Q, B, d, D, false, N, k, idx_offset, keep, out_val, out_idx, workspace, workspace_bytes,
                                       (hipStream_t)stream, "tt_score_topk_biased_f32", false, nullptr, nullptr, nullptr, bias});
}

TT_EXPORT int tt_score_topk_biased_bf16(const float *Q, int B, int d, const void *D_bf16, int64_t N, const float *bias,
                                        const uint32_t *keep, int k, int64_t idx_offset, float *out_val, int64_t *out_idx,
                                        void *workspace, size_t workspace_bytes, tt_stream_t stream)
{
    return score_topk_biased(ExactCall{Q, B, d, D_bf16, true, N, k, idx_offset, keep, out_val, out_idx, workspace, workspace_bytes,
                                       (hipStream_t)stream, "tt_score_topk_biased_bf16", false, nullptr, nullptr, nullptr, bias});
}

// ---- Cursor search (DESIGN.md "Cursor search") -------------------------------------------------------------------------------
// The masked call for k <= 64 restricted, per query, to the documents strictly after a (score, id) cursor in the order (score
// desc, index asc): the same plan, workspace and launches, on the AFTER instantiations of the main and sample passes
// (score_topk.hip).  after_val == after_idx == NULL is the masked call itself.
namespace {
int score_topk_after(ExactCall c)
{
    if (c.k > MERGE_KMAX)
        return tt_fail(TT_ERR_UNSUPPORTED, "%s: k=%d > %d (a larger page is two consecutive calls)", c.who, c.k, MERGE_KMAX);
    if ((c.after_val != nullptr) != (c.after_idx != nullptr))
        return tt_fail(TT_ERR_BAD_SHAPE, "%s: after_val and after_idx must be both NULL or both non-NULL", c.who);
    if (((uintptr_t)c.after_val & 3) || ((uintptr_t)c.after_idx & 7))
        return tt_fail(TT_ERR_BAD_SHAPE, "%s: after_val must be 4-byte and after_idx 8-byte aligned", c.who);
    return score_topk_large(c);
}
} // namespace

TT_EXPORT size_t tt_score_topk_after_workspace_bytes(int B, int64_t N, int d, int k, int bf16)
{
    return k > MERGE_KMAX ? 0 : tt_score_topk_large_workspace_bytes(B, N, d, k, bf16);
}

TT_EXPORT int tt_score_topk_after_f32(const float *Q, int B, int d, const float *D, int64_t N, const float *after_val,
                                      const int64_t *after_idx, const uint32_t *keep, int k, int64_t idx_offset, float *out_val,
                                      int64_t *out_idx, void *workspace, size_t workspace_bytes, tt_stream_t stream)
{
    return score_topk_after(ExactCall{Q, B, d, D, false, N, k, idx_offset, keep, out_val, out_idx, workspace, workspace_bytes,
                                      (hipStream_t)stream, "tt_score_topk_after_f32", false, nullptr, nullptr, nullptr, nullptr,
                                      after_val, after_idx});
}

TT_EXPORT int tt_score_topk_after_bf16(const float *Q, int B, int d, const void *D_bf16, int64_t N, const float *after_val,
                                       const int64_t *after_idx, const uint32_t *keep, int k, int64_t idx_offset, float *out_val,
                                       int64_t *out_idx, void *workspace, size_t workspace_bytes, tt_stream_t stream)
{
    return score_topk_after(ExactCall{Q, B, d, D_bf16, true, N, k, idx_offset, keep, out_val, out_idx, workspace, workspace_bytes,
                                      (hipStream_t)stream, "tt_score_topk_after_bf16", false, nullptr, nullptr, nullptr, nullptr,
                                      after_val, after_idx});
}

// The kernels' local id bound of a cursor (after_words.h), for a caller that wants to see it: host code only.
TT_EXPORT int tt_after_local_bound(int64_t after_idx, int64_t idx_offset, int N)
{
    return after_local_bound(after_idx, idx_offset, N < 0 ? 0 : N);
}

namespace {
// keep word w = the ballots of keep_bool[32 w .. 32 w + 31] != 0 (a wave packs two words); bits at or beyond N are zero
__global__ __launch_bounds__(256) void keep_pack_kernel(const uint8_t *__restrict__ keep_bool, int64_t N, unsigned *__restrict__ keep)
{
    const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const unsigned long long b = __ballot(n < N && keep_bool[n] != 0);
    const int lane = threadIdx.x & 63;
    if ((lane == 0 || lane == 32) && n < N)
        keep[n >> 5] = (unsigned)(b >> lane);
}

// bit ids[i] - idx_offset cleared (vector atomic AND); ids outside [idx_offset, idx_offset + N) are somebody else's rows
__global__ __launch_bounds__(256) void keep_clear_kernel(unsigned *keep, int64_t N, const int64_t *__restrict__ ids, int64_t n_ids,
                                                         int64_t idx_offset)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_ids)
        return;
    const int64_t id = ids[i];
    if (id < idx_offset || id - idx_offset >= N) // (ordered so that the subtraction cannot overflow for any id >= idx_offset)
        return;
    const int64_t n = id - idx_offset;
    atomicAnd(keep + (n >> 5), ~(1u << (n & 31)));
}
} // namespace

TT_EXPORT int tt_keep_mask_pack(const uint8_t *keep_bool, int64_t N, uint32_t *keep, tt_stream_t stream)
{
    if (N < 0 || N > (int64_t)INT_MAX * 256)
        return tt_fail(TT_ERR_BAD_SHAPE, "tt_keep_mask_pack: N=%lld", (long long)N);
    if (N == 0)
        return TT_OK;
    if (!keep_bool || !keep || ((uintptr_t)keep & 3))
        return tt_fail(TT_ERR_BAD_SHAPE, "tt_keep_mask_pack: null pointer, or keep not 4-byte aligned");
    hipLaunchKernelGGL(keep_pack_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, (hipStream_t)stream, keep_bool, N, keep);
    TT_LAUNCH_CHECK();
    return TT_OK;
}

TT_EXPORT int tt_keep_mask_clear_ids(uint32_t *keep, int64_t N, const int64_t *ids, int64_t n_ids, int64_t idx_offset,
                                     tt_stream_t stream)
{
    if (N < 0 || n_ids < 0 || n_ids > (int64_t)INT_MAX * 256)
        return tt_fail(TT_ERR_BAD_SHAPE, "tt_keep_mask_clear_ids: N=%lld n_ids=%lld", (long long)N, (long long)n_ids);
    if (N == 0 || n_ids == 0)
        return TT_OK;
    if (!keep || !ids || ((uintptr_t)keep & 3))
        return tt_fail(TT_ERR_BAD_SHAPE, "tt_keep_mask_clear_ids: null pointer, or keep not 4-byte aligned");
    hipLaunchKernelGGL(keep_clear_kernel, dim3((unsigned)((n_ids + 255) / 256)), dim3(256), 0, (hipStream_t)stream, keep, N, ids,
                       n_ids, idx_offset);
    TT_LAUNCH_CHECK();
    return TT_OK;
}

TT_EXPORT int tt_topk_merge_large(const float *in_val, const int64_t *in_idx, int B, int M, int k, float *out_val,
                                  int64_t *out_idx, tt_stream_t stream)
{
    if (B < 0 || M < 0 || k <= 0)
        return tt_fail(TT_ERR_BAD_SHAPE, "tt_topk_merge_large: B=%d M=%d k=%d", B, M, k);
    if (k > TT_TOPK_LARGE_KMAX)
        return tt_fail(TT_ERR_UNSUPPORTED, "tt_topk_merge_large: k=%d > %d", k, TT_TOPK_LARGE_KMAX);
    if (k <= MERGE_KMAX)
        return tt_topk_merge(in_val, in_idx, B, M, k, out_val, out_idx, stream);
    if (B == 0)
        return TT_OK;
    SegSource src{in_val, in_idx, M, M > 0 ? M : 1, 0};
    hipLaunchKernelGGL(lk_merge_kernel, dim3(B), dim3(LSEL_THREADS), 0, (hipStream_t)stream, src, k, out_val, out_idx);
    TT_LAUNCH_CHECK();
    return TT_OK;
}

TT_EXPORT int tt_topk_merge_shards_large(const void *gathered, int world, size_t rank_stride, size_t idx_byte_offset, int B,
                                         int kp, int k, float *out_val, int64_t *out_idx, tt_stream_t stream)
{
    if (B < 0 || world <= 0 || kp <= 0 || k <= 0)
        return tt_fail(TT_ERR_BAD_SHAPE, "tt_topk_merge_shards_large: world=%d B=%d kp=%d k=%d", world, B, kp, k);
    if (k > TT_TOPK_LARGE_KMAX)
        return tt_fail(TT_ERR_UNSUPPORTED, "tt_topk_merge_shards_large: k=%d > %d", k, TT_TOPK_LARGE_KMAX);
    if (k <= MERGE_KMAX)
        return tt_topk_merge_shards(gathered, world, rank_stride, idx_byte_offset, B, kp, k, out_val, out_idx, stream);
    TT_RC_CHECK(merge_shards_layout_ok(ShardsCall{gathered, world, rank_stride, idx_byte_offset, B, kp, "tt_topk_merge_shards_large"},
                                       out_val, out_idx));
    if (B == 0)
        return TT_OK;
    SegSource src{(const float *)gathered, (const int64_t *)((const char *)gathered + idx_byte_offset), world * kp, kp,
                  rank_stride};
    hipLaunchKernelGGL(lk_merge_kernel, dim3(B), dim3(LSEL_THREADS), 0, (hipStream_t)stream, src, k, out_val, out_idx);
    TT_LAUNCH_CHECK();
    return TT_OK;
}
