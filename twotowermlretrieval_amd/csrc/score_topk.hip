// K4/K5: fused brute-force scoring + top-k, exact fp32 (gfx950).
//
// Replaces torch.matmul(q, D.t()) + torch.topk (backend/evaluators.py:185-186,
// :269-272; backend/trainer.py:62-65) without ever forming the [B,N] matrix.
//
// Design (DESIGN.md section "K4"):
//  * one WAVE is an independent streaming engine for one task =
//    (32-query tile, contiguous range of 32-document tiles).  No block barrier
//    anywhere: the wave that issues an LDS-DMA is the wave that waits for it
//    (counted s_waitcnt vmcnt) and reads it.
//  * the 32 queries live in VGPRs as the B operand of v_mfma_f32_32x32x2_f32
//    (lane l holds Q[l&31][2s + (l>>5)], s = 0..d/2-1); documents are the A
//    operand, so a lane's 16 accumulator registers are 16 documents of ONE
//    query and the running top-k threshold is a lane-local register.
//  * documents stream HBM -> LDS with global_load_lds_dwordx4 in 4 KiB slabs
//    (32 docs x 32 features = one 128-B line per doc), a 4-deep private ring
//    per wave; the 16-B chunks of a row are XOR-swizzled on the SOURCE address
//    so the ds_read_b128 operand reads are bank-conflict free.
//  * scores are bit-for-bit the ascending-index fp32 FMA chain of
//    oracle/tt_oracle.c:o_score_topk (MFMA f32 = k-ordered fmaf chain; lane
//    half h supplies feature 2s+h, so the chain order is 0,1,2,...,d-1).
//  * selection: a score reaches the slow path only if it is >= its query's
//    current k-th best (a lane-local register); the slow path appends (score, doc)
//    to the (wave, query) candidate buffer in the caller's workspace with a
//    fire-and-forget 8-byte store; a nearly full buffer -- and every buffer once
//    at the end -- is rank-compacted by the wave (each lane counts the entries
//    ranking before its own, entries of rank < k are written back sorted, the
//    k-th score becomes the new bound).  Ties: score desc, index asc.  Partial
//    lists go to the workspace; topk_merge_kernel reduces them (also used for the
//    sample-pass maxima and for the cross-shard merge after the RCCL all-gather).
#include "tt_common.h"

#include <limits.h>
#include <math.h>

namespace {

constexpr int TILE_DOCS = 32;
constexpr int SLAB_BYTES = 32 * 128; // 32 docs x 32 f32
constexpr int NSTAGE = 4;            // ring depth (slabs); NSTAGE-1 in flight
#ifndef TT_K4_NT_NSTAGE
#define TT_K4_NT_NSTAGE 4
#endif
constexpr int NSTAGE_NT = TT_K4_NT_NSTAGE; // the one-query-tile build's ring (its waves re-read nothing: more bytes in flight per CU)
constexpr int WPB = 4;               // waves per block
constexpr int DMA_PER_SLAB = 4;      // global_load_lds_dwordx4 per slab per wave
constexpr int PACE_R = 16;            // pacing counter slots per chunk (> pace_lag + 1)
constexpr int PACE_POLLS = 400;       // bound of one wait (~0.3 us per poll)
constexpr int DRAW_POLLS = 1 << 16;   // bound of the wait for a chunk-mate's pool draw (s_sleep 2 = 128 clocks per poll: ~4 ms)
constexpr int DRAW_GAVE_UP = 0x7fffffff;

typedef __attribute__((address_space(3))) void lds_void;
typedef const __attribute__((address_space(1))) void gbl_void;

struct Cand;
struct ScoreParams {
    const float *Q;
    const void *D; // [N][d] f32, or bf16 for the BF instantiations
    int B;
    int N;
    int k;
    int n_qtiles;
    int n_chunks;
    int tiles_per_chunk;
    int n_tiles;
    int n_tasks;
    // tiles [0, static_tiles) are split evenly over the chunks (tiles_per_chunk each); tiles [static_tiles, n_tiles) are a
    // pool of tail_blocks blocks of tail_g tiles per query tile that the waves draw from (tail_ctr[qtile], atomicAdd) once
    // their own range is done: the chip's XCDs do not stream / multiply at one speed (wave end times spread over 10-13 %
    // of the launch with equal shares).  tail_ctr == nullptr: everything static.
    int static_tiles, tail_g, tail_blocks;
    int *tail_ctr;
    // Several query tiles (K4 only): the n_qtiles waves of a chunk sit on one XCD and read the same documents, but nothing
    // keeps them within an L2's reach of each other (32 waves over 160 MB each: 10x the corpus fetched at B = 1024).
    // pace[chunk][PACE_R]: a wave adds 1 to slot b % PACE_R when it has finished its b-th block of pace_g tiles and does
    // not start block b + pace_lag before all n_qtiles waves have (a HINT: the wait is bounded, and a wave that ran into
    // the bound stops waiting for good, so nothing depends on the other waves being resident).  grp_blk[chunk][grp_maxseg]:
    // the pool blocks the chunk's waves take, drawn by whichever of them gets there first (0 = not drawn, -1 = being
    // drawn, else block + 1), so that the pool is walked in step as well.  Both nullptr: every wave for itself.
    int *pace;
    int pace_g, pace_lag;
    int *pace_timeouts; // one word behind the pacing slots: how many waves gave up a pacing wait (the counters are only
                        // coherent among waves that share an XCD's L2: a chunk that straddles XCDs times out once per wave
                        // -- correct results, ~0.15 ms late; tt_score_topk_pace_timeouts_offset lets a bench report it)
    int *grp_blk;
    int grp_maxseg;
    float *pval;   // [n_qtiles*32][n_chunks][k]
    int64_t *pidx; // same shape, global indices (idx_offset applied), -1 = empty
    int64_t idx_offset;
    struct Cand *cand;  // [n_tasks][32][CAP] candidate buffers (workspace)
    const float *thr0;  // optional per-query lower bound of the final k-th score
    int thr0_stride, thr0_off;
    const int *run_if;  // optional device predicate per 32-query tile: tile t is skipped while run_if[t] == 0
    int draw_polls;     // bound of the wait for a chunk-mate's pool draw (DRAW_POLLS; the comparison build can force a give-up)
    const unsigned *keep; // MASKED instantiations: keep-bitmask, one word per 32-document tile (bit n & 31 of word n >> 5 set ->
                          // document n of D may be returned); nullptr in every other launch
};

// The keep word of one tile (MASKED).  It is wave-uniform, so it travels as a scalar load on the lgkmcnt side: the tile loop's
// LDS-DMA ring lives on counted vmcnt waits, and a compiler-visible global load in the loop would make hipcc drain it
// (vmcnt(0)) on every tile.  Issued in front of the tile's last slab of MFMAs, waited for in front of the epilogue: the
// latency sits under that slab's multiply chain.  The wait names the destination, so no consumer is scheduled above it, and
// the tile's accumulators, so that hipcc cannot hoist it above the MFMAs (register-only instructions, which "memory" does not
// order) back to the load.
// (first: the slab's first A operand(s), named so that the slab's MFMA chain stays below the load)
template <class A>
__device__ __forceinline__ void keep_word_issue(const unsigned *word, unsigned &kw, A &first)
{
    asm volatile("s_load_dword %[kw], %[word], 0x0" : [kw] "=s"(kw), "+v"(first) : [word] "s"(word) : "memory");
}

template <class Acc>
__device__ __forceinline__ void keep_word_wait(unsigned &kw, Acc &acc)
{
    asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(kw), "+v"(acc) : : "memory");
}

__device__ __forceinline__ int xcd_remap(int b, int nblk)
{
    // consecutive logical blocks -> blocks that share an XCD (b % 8 equal), bijective.
    if (nblk < 16)
        return b;
    int x = b & 7, q = nblk >> 3, r = nblk & 7;
    return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + (b >> 3);
}

// One candidate: (score, document index relative to D).  8 bytes, one store.
struct __attribute__((aligned(8))) Cand {
    float v;
    int x;
};

__device__ __forceinline__ Cand cand_load_l2(const Cand *p)
{
    // sc1 load: served by L2, never by a stale line in this CU's L1 (the wave re-reads what it wrote)
    unsigned long long u = __hip_atomic_load((const unsigned long long *)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    Cand c;
    c.v = __uint_as_float((unsigned)u);
    c.x = (int)(u >> 32);
    return c;
}

// Fire-and-forget 8-byte candidate store the compiler's waitcnt pass does not see (it still counts in
// vmcnt: the counted waits of the DMA ring only get stricter, and every reader drains vmcnt(0) first).
__device__ __forceinline__ void cand_store_async(Cand *dst, float v, int x)
{
    const unsigned long long bits = ((unsigned long long)(unsigned)x << 32) | (unsigned long long)__float_as_uint(v);
    asm volatile("global_store_dwordx2 %0, %1, off\n\ts_nop 1" ::"v"(dst), "v"(bits) : "memory");
}

// Wave-cooperative compaction of one query's candidate buffer: keeps the k best of its n
// entries (score desc, index asc), SORTED, at the front.  Lane t owns entries t, t+64, ...
// rank(e) = #{entries ranking before e}; ranks are a permutation because (score,index) pairs
// are distinct.  Returns through the references the new count and, when n >= k, the k-th score.
template <int CAP>
__device__ __forceinline__ void compact_query(Cand *base, int n, int k, int lane, int &n_new, float &kth,
                                              bool &have_kth)
{
    constexpr int E = CAP / 64;
    float v[E];
    int x[E], rank[E];
#pragma unroll
    for (int i = 0; i < E; ++i) {
        const int e = lane + 64 * i;
        Cand c;
        c.v = -INFINITY;
        c.x = INT_MAX;
        if (e < n)
            c = cand_load_l2(base + e);
        v[i] = c.v;
        x[i] = c.x;
        rank[i] = 0;
    }
#pragma unroll
    for (int i2 = 0; i2 < E; ++i2) {
        const int lim = min(n - 64 * i2, 64);
        for (int l2 = 0; l2 < lim; ++l2) {
            const float sv = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v[i2]), l2));
            const int sx = __builtin_amdgcn_readlane(x[i2], l2);
#pragma unroll
            for (int i = 0; i < E; ++i)
                rank[i] += (sv > v[i] || (sv == v[i] && sx < x[i])) ? 1 : 0;
        }
    }
    have_kth = n >= k;
    kth = -INFINITY;
#pragma unroll
    for (int i = 0; i < E; ++i) {
        const bool live = lane + 64 * i < n;
        if (live && rank[i] < k) {
            Cand c;
            c.v = v[i];
            c.x = x[i];
            base[rank[i]] = c;
        }
        const unsigned long long bk = __ballot(live && rank[i] == k - 1);
        if (bk)
            kth = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v[i]), __ffsll((long long)bk) - 1));
    }
    n_new = min(n, k);
}

// MAXONLY = true is the sample pass: no candidate buffers, each (wave, query) only tracks the
// maximum score over its documents (one partial entry, index = chunk id).
// NT: the document stream with the nt cache policy (aux = 2): for ONE query tile, when every byte is read once by one wave
// (B = 32 over 10M x 256: 1.884 -> 1.84 ms; with 32 query tiles re-reading each chunk from L2 it costs 20 %: 44.2 -> 52.9 ms)
// BF: the documents are bf16 rows (tt_score_topk_bf16).  A 128-B line of a row then carries 64 features, so a tile is NS/2
// slabs; the same ring, swizzle and reads bring in the raw words and each A operand is widened in a register (bf16 -> fp32
// is exact: the high half of the fp32 word), in the same ascending feature order -- the scores are tt_score_topk_f32's over
// the widened rows, bit for bit.
// MASKED: p.keep decides which documents may be returned (tt_score_topk_masked_f32 / _bf16).  A masked document is scored like
// any other and then left out of every selection: the append pass, and the sample maxima (a bound taken from a document that
// cannot be returned is no lower bound of the masked k-th score).  MASKED = false is the kernel as it always was.
template <int NS, int CAP, bool MAXONLY, bool NT = false, bool BF = false, bool MASKED = false>
__global__ __launch_bounds__(WPB * 64, 2) void score_topk_kernel(ScoreParams p)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    static_assert(!BF || NS % 2 == 0, "bf16 rows: d a multiple of 64");
    constexpr int NST = NT ? NSTAGE_NT : NSTAGE;
    constexpr int WAVE_LDS = NST * SLAB_BYTES;
    constexpr int NSD = BF ? NS / 2 : NS; // 128-B slabs per document row
    constexpr int ROW_BYTES = NSD * 128;
    const int lane = threadIdx.x & 63;
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    char *ring = smem + wid * WAVE_LDS;

    const int task = xcd_remap(blockIdx.x, gridDim.x) * WPB + wid;
    if (task >= p.n_tasks)
        return; // wave-uniform; the kernel has no block-level barrier
    const int qtile = task % p.n_qtiles;
    if (p.run_if && p.run_if[qtile] == 0)
        return;
    const int chunk = task / p.n_qtiles;
    int t0 = chunk * p.tiles_per_chunk; // the wave's own range first, then blocks of the pool
    int t1 = min(t0 + p.tiles_per_chunk, p.static_tiles);
    const int k = p.k;
    const int h = lane >> 5;
    const int j = lane & 31;

    // ---- query operand: lane (j,h) keeps Q[qrow][2s+h] --------------------
    // Staged through the (still idle) ring so the global reads are whole 512-B rows instead of
    // 4-byte strided accesses: coalesced global_load_dwordx4 -> swizzled ds_write_b128 -> ds_read_b128.
    const int qrow = qtile * 32 + j;
    float qreg[NS * 16];
    {
        constexpr int F = NS % 4 == 0 ? 128 : (NS % 2 == 0 ? 64 : 32); // features per pass (32 x F floats <= 16 KiB)
        constexpr int NPASS = NS * 32 / F;
        constexpr int CPR = F / 4;                 // 16-byte chunks per row
        constexpr int SWZ = CPR >= 16 ? 15 : CPR - 1;
#pragma unroll
        for (int pass = 0; pass < NPASS; ++pass) {
#pragma unroll
            for (int i = 0; i < F / 8; ++i) {
                const int idx = i * 64 + lane;
                const int row = idx / CPR, ch = idx % CPR;
                const int gr = qtile * 32 + row;
                f32x4 v = {0, 0, 0, 0};
                if (gr < p.B)
                    v = *(const f32x4 *)(p.Q + (size_t)gr * (NS * 32) + pass * F + ch * 4);
                *(f32x4 *)(ring + row * (F * 4) + ((ch ^ (row & SWZ)) << 4)) = v;
            }
#pragma unroll
            for (int t = 0; t < CPR; ++t) {
                const f32x4 v = *(const f32x4 *)(ring + j * (F * 4) + ((t ^ (j & SWZ)) << 4));
                qreg[pass * (F / 2) + 2 * t] = h ? v.y : v.x;
                qreg[pass * (F / 2) + 2 * t + 1] = h ? v.w : v.z;
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); // reads done before the region is rewritten
        }
    }
    // Selection state of query j, replicated in lanes j and j+32:
    //   thr = a proven lower bound of the query's final k-th score (documents below it are dropped),
    //   cnt = entries in this wave's candidate buffer for the query.
    // thr starts from the caller's bound (k-th score over a sample of the corpus, or -inf).
    float thr = INFINITY; // padded queries never qualify
    if (qrow < p.B)
        thr = (!MAXONLY && p.thr0) ? p.thr0[(size_t)qrow * p.thr0_stride + p.thr0_off] : -INFINITY;
    int cnt = 0;
    float runmax = -INFINITY;
    Cand *const cbase = p.cand + ((size_t)task * 32 + j) * CAP; // this lane's query buffer

    auto compact_where = [&](unsigned long long qmask) { // qmask: bit q set -> compact query q
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // candidate stores have reached L2
        while (qmask) {
            const int q = __ffsll((long long)qmask) - 1;
            qmask &= qmask - 1;
            const int n = __builtin_amdgcn_readlane(cnt, q);
            int n_new;
            float kth;
            bool have;
            compact_query<CAP>(p.cand + ((size_t)task * 32 + q) * CAP, n, k, lane, n_new, kth, have);
            if (j == q) {
                cnt = n_new;
                if (have)
                    thr = kth; // >= old thr: every entry was admitted under a bound <= it
            }
        }
    };

    // ---- pacing (see ScoreParams::pace) ------------------------------------
    constexpr bool PACED = !MAXONLY && !NT; // (NT is the one-query-tile build)
    int *const pace = (PACED && p.pace) ? p.pace + (size_t)chunk * PACE_R : nullptr;
    bool waits = pace != nullptr; // false once a wait ran into its bound
    int gb = 0;                   // blocks of pace_g tiles this wave has finished
    int in_blk = 0;               // tiles of the current block done
    int seg = 0;                  // pool blocks this wave has taken
    bool gave_up = false;         // a shared pool draw timed out (wave-uniform)
    auto pace_gate = [&](int b) { // all n_qtiles waves of the chunk have finished their block b?
        const int need = p.n_qtiles * (b / PACE_R + 1);
        const int *slot = pace + (b % PACE_R);
        for (int polls = 0;; ++polls) {
            int v;
            // scalar load past the scalar cache: its own counter (lgkmcnt), so the LDS-DMA ring stays in flight
            asm volatile("s_load_dword %0, %1, 0x0 glc\n\ts_waitcnt lgkmcnt(0)" : "=s"(v) : "s"(slot) : "memory");
            if (v >= need)
                return;
            if (polls == PACE_POLLS) {
                waits = false;
                if (lane == 0)
                    atomicAdd(p.pace_timeouts, 1);
                return;
            }
            __builtin_amdgcn_s_sleep(8);
        }
    };

    // ---- DMA state -------------------------------------------------------
    // DMA instruction jj moves docs 8jj..8jj+7 of the tile: lane -> (doc 8jj + lane>>3,
    // physical 16-B chunk lane&7).  Logical chunk = physical ^ ((doc>>1)&7) (source swizzle).
    const char *Dbytes = (const char *)p.D;
    int dma_tile = t0, dma_s = 0;
    const char *rowp[DMA_PER_SLAB];
    auto set_rows = [&](int tile) {
#pragma unroll
        for (int jj = 0; jj < DMA_PER_SLAB; ++jj) {
            int di = 8 * jj + (lane >> 3);
            int doc = min(tile * TILE_DOCS + di, p.N - 1);
            int chunk16 = (lane & 7) ^ ((di >> 1) & 7);
            rowp[jj] = Dbytes + (size_t)doc * ROW_BYTES + chunk16 * 16;
        }
    };
    auto dma_issue = [&](int stage) {
        char *dst = ring + stage * SLAB_BYTES;
#pragma unroll
        for (int jj = 0; jj < DMA_PER_SLAB; ++jj)
            __builtin_amdgcn_global_load_lds((gbl_void *)(rowp[jj] + dma_s * 128),
                                             (lds_void *)(dst + jj * 1024), 16, 0, NT ? 2 : 0);
        if (++dma_s == NSD) {
            dma_s = 0;
            dma_tile = min(dma_tile + 1, t1 - 1); // past the end: harmless re-read
            set_rows(dma_tile);
        }
    };

    for (;;) { // segments: the own range, then pool blocks
    if (t0 < t1) {
        set_rows(t0);
#pragma unroll
        for (int g = 0; g < NST - 1; ++g)
            dma_issue(g);

        // read address: lane (i=j, h) wants logical chunk c of row i
        const int rd_swz = (j >> 1) & 7;
        const char *rd_row = ring + j * 128;
        int stage = 0;

        for (int tile = t0; tile < t1; ++tile) {
            if (PACED && waits && in_blk == 0 && gb >= p.pace_lag)
                pace_gate(gb - p.pace_lag);
            f32x16 acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
            unsigned kw = 0xffffffffu; // the tile's keep word (MASKED)
#pragma unroll
            for (int s = 0; s < NSD; ++s) {
                // slab (tile,s) has landed once at most (NST-2) younger slabs are pending
                // (candidate stores also count in vmcnt: they only make this wait stricter)
                asm volatile("s_waitcnt vmcnt(%0)" ::"n"(DMA_PER_SLAB * (NST - 2)) : "memory");
                const char *buf = rd_row + stage * SLAB_BYTES;
                f32x4 frag[8];
#pragma unroll
                for (int c = 0; c < 8; ++c)
                    frag[c] = *(const f32x4 *)(buf + ((c ^ rd_swz) << 4));
                // the ring slot consumed one step ago is free once its reads have returned
#ifndef TT_K4_NO_LGKM0
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#endif
                // (MASKED: right behind the asm wait above, which already ends a scheduling region -- a statement further
                //  down would pin dma_issue's address arithmetic in front of it instead of between the MFMAs)
                if (MASKED && s == NSD - 1)
                    keep_word_issue(p.keep + tile, kw, frag[0]);
                dma_issue((stage + NST - 1) % NST);
                if (BF) {
                    // chunk c holds features 8c..8c+7 of the slab; word w = features (8c+2w, 8c+2w+1) in its (low, high)
                    // half = feature pair 4c+w, of which lane half h supplies feature 8c+2w+h
                    const int sh = h ? 0 : 16;
#pragma unroll
                    for (int c = 0; c < 8; ++c) {
#pragma unroll
                        for (int w = 0; w < 4; ++w) {
                            const unsigned u = __float_as_uint(frag[c][w]);
                            const float a = __uint_as_float((u << sh) & 0xffff0000u);
                            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, qreg[32 * s + 4 * c + w], acc, 0, 0, 0);
                        }
                    }
                } else {
#pragma unroll
                    for (int c = 0; c < 8; ++c) {
                        float a0 = h ? frag[c].y : frag[c].x;
                        float a1 = h ? frag[c].w : frag[c].z;
                        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, qreg[16 * s + 2 * c], acc, 0, 0, 0);
                        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, qreg[16 * s + 2 * c + 1], acc, 0, 0, 0);
                    }
                }
                stage = (stage + 1) % NST;
            }

            // ---- epilogue: acc[r] = score(doc tile*32 + (r&3)+8(r>>2)+4h, query j) ----
            const int tile_base = tile * TILE_DOCS;
            const bool partial = tile_base + TILE_DOCS > p.N;
            // MASKED: bit (r & 3) + 8 (r >> 2) of kwh = the keep bit of the lane's document r (bits at or beyond N: the
            // doc < p.N test stays)
            unsigned kwh = 0xffffffffu;
            if (MASKED) {
                keep_word_wait(kw, acc);
                kwh = kw >> (4 * h);
            }
            auto kept = [&](int r) { return !MASKED || ((kwh >> ((r & 3) + 8 * (r >> 2))) & 1u) != 0u; };
            if (MAXONLY) {
                float m = -INFINITY;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int doc = tile_base + (r & 3) + 8 * (r >> 2) + 4 * h;
                    m = fmaxf(m, ((!partial || doc < p.N) && kept(r)) ? acc[r] : -INFINITY);
                }
                runmax = fmaxf(runmax, m);
                continue;
            }
            float m = acc[0];
#pragma unroll
            for (int r = 1; r < 16; ++r)
                m = fmaxf(m, acc[r]);
            // (MASKED: m may come from a masked document -- that only costs the slow path a look; a tile with nothing kept
            //  skips it)
            if ((!MASKED || kw != 0u) && __ballot(m >= thr) != 0ull) {
                // Append pass.  The store is inline asm on purpose: a compiler-visible global store
                // (or the compaction's loads) inside this loop makes hipcc emit s_waitcnt vmcnt(0) at
                // every join, which drains the LDS-DMA ring on each tile that has a candidate.
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int doc = tile_base + (r & 3) + 8 * (r >> 2) + 4 * h;
                    const bool c = (!partial || doc < p.N) && kept(r) && acc[r] >= thr;
                    const unsigned long long mask = __ballot(c);
                    if (mask == 0ull)
                        continue;
                    const int c_lo = (int)((mask >> j) & 1ull), c_hi = (int)((mask >> (j + 32)) & 1ull);
                    if (c)
                        cand_store_async(cbase + cnt + (h ? c_lo : 0), acc[r], doc);
                    cnt += c_lo + c_hi;
                }
                // one tile adds at most 32 entries per query: compact while there is still room for that
                const unsigned long long full = __ballot(cnt > CAP - 34) & 0xffffffffull;
                if (full)
                    compact_where(full);
            }
            if (PACED && pace && (++in_blk == p.pace_g || tile == t1 - 1)) {
                // block done (counted whether or not this wave still waits for the others: they may wait for it)
                if (lane == 0)
                    asm volatile("global_atomic_add %0, %1, off" ::"v"(pace + (gb % PACE_R)), "v"(1) : "memory");
                ++gb;
                in_blk = 0;
            }
        }
    }
    if (MAXONLY || !p.tail_ctr)
        break;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // the over-prefetch of the segment's end has landed: the ring is free
    int blk = 0;
    if (PACED && p.grp_blk) {
        // the chunk's waves take the same pool blocks in the same order: the first to get here draws for all of them
        if (seg >= p.grp_maxseg)
            break;
        if (lane == 0) {
            int *slot = p.grp_blk + (size_t)chunk * p.grp_maxseg + seg;
            int v = __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            bool drew = false;
            if (v == 0) {
                int expected = 0;
                if (__hip_atomic_compare_exchange_strong(slot, &expected, -1, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                         __HIP_MEMORY_SCOPE_AGENT)) {
                    v = atomicAdd(p.tail_ctr, 1) + 1;
                    __hip_atomic_store(slot, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    drew = true;
                } else {
                    v = expected;
                }
            }
            // the drawing wave is between its two atomics (it waits for nobody: ~2 us).  Bounded like every other cross-wave
            // wait of the library: DRAW_POLLS sleeps (~4 ms) and the wave gives up -- its partial lists then say so (below), and
            // tt_score_topk_f32 redoes the wave's query tile on the static split, which waits for nobody
            if (p.draw_polls < 0 && !drew) // (comparison build, TT_DRAW_POLLS=-1: every wave that did not draw itself gives up)
                v = -1;
            for (int polls = 0; v < 0 && polls < p.draw_polls; ++polls) {
                __builtin_amdgcn_s_sleep(2);
                v = __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            blk = v < 0 ? DRAW_GAVE_UP : v - 1;
        }
        ++seg;
    } else if (lane == 0) {
        blk = atomicAdd(p.tail_ctr + qtile, 1);
    }
    blk = __builtin_amdgcn_readfirstlane(blk);
    if (blk == DRAW_GAVE_UP)
        gave_up = true;
    if (blk >= p.tail_blocks)
        break;
    t0 = p.static_tiles + blk * p.tail_g;
    t1 = min(t0 + p.tail_g, p.n_tiles);
    dma_tile = t0;
    dma_s = 0;
    }
    // LDS-DMA still in flight would land after the wave has ended: drain it (and the stores).
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

    if (MAXONLY) {
        runmax = fmaxf(runmax, __shfl_xor(runmax, 32));
        if (h == 0 && qrow < p.B) {
            const size_t o = (size_t)qrow * p.n_chunks + chunk;
            p.pval[o] = runmax;
            p.pidx[o] = t0 < t1 ? (int64_t)chunk : -1;
        }
        return;
    }

    // ---- final compaction + partial lists out ---------------------------------
    {
        const unsigned long long over = __ballot(cnt > k) & 0xffffffffull;
        if (over)
            compact_where(over);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    // 32*k output slots, lanes take them round-robin so the candidate loads overlap.  The trip count is wave-uniform: the
    // __shfl reads query q's count from lane q, and a lane that has left the loop would return 0 there (ds_bpermute)
    const int rows_live = min(32, p.B - qtile * 32);
    for (int it0 = 0; it0 < rows_live * k; it0 += 64) {
        const int it = it0 + lane;
        const int q = min(it / k, rows_live - 1), t = it - q * k;
        const int n = __shfl(cnt, q);
        if (it >= rows_live * k)
            continue;
        const size_t o = ((size_t)(qtile * 32 + q) * p.n_chunks + chunk) * k + t;
        Cand c;
        c.v = -INFINITY;
        c.x = -1;
        if (t < n)
            c = cand_load_l2(p.cand + ((size_t)task * 32 + q) * CAP + t);
        // a wave that gave up a pool draw has not seen every document: its lists carry (+inf, TT_TOPK_INVALID_INDEX + t),
        // which the merge ranks first -- tt_score_topk_f32 looks for them in the merged lists and redoes those query tiles
        // (redo_flag_kernel below); a caller of the partials entry point sees them as they are
        p.pval[o] = gave_up ? INFINITY : c.v;
        p.pidx[o] = gave_up ? (int64_t)TT_TOPK_INVALID_INDEX + t : (t < n ? p.idx_offset + c.x : -1);
    }
}

// ---------------------------------------------------------------------------
// K4w: the same kernel for wide embeddings, 256 < d <= 512 (HIDDEN_DIM up to 512 is what the encoder supports).
// 32 queries x 512 features do not fit a wave's registers as 32x32x2 B operands, so a task is a 16-QUERY tile on
// v_mfma_f32_16x16x4_f32: lane (n = l&15, kq = l>>4) keeps Q[n][4s+kq], s < d/4 (128 VGPRs at d = 512) and its
// 8 accumulator registers are 8 documents of query n (two 16-document sub-tiles x rows 4kq..4kq+3).  A chain of
// 16x16x4 MFMAs with k ascending is bit-identical to the sequential fmaf chain, like the 32x32x2 form
// (tools/experiments/mfma16_order.hip), so the oracle parity carries over.  Ring, DMA, thresholds, candidate
// buffers, compaction, partial lists and merge are K4's; the launch is bound by HBM streaming (d * 4 bytes per doc).
// ---------------------------------------------------------------------------
template <int NS, int CAP, bool MAXONLY, bool NT = false, bool MASKED = false>
__global__ __launch_bounds__(WPB * 64, 2) void score_topk16_kernel(ScoreParams p)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int WAVE_LDS = NSTAGE * SLAB_BYTES;
    constexpr int ROW_BYTES = NS * 128;
    const int lane = threadIdx.x & 63;
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    char *ring = smem + wid * WAVE_LDS;

    const int task = xcd_remap(blockIdx.x, gridDim.x) * WPB + wid;
    if (task >= p.n_tasks)
        return; // wave-uniform; the kernel has no block-level barrier
    const int qtile = task % p.n_qtiles; // 16 queries
    if (p.run_if && p.run_if[qtile >> 1] == 0)
        return;
    const int chunk = task / p.n_qtiles;
    int t0 = chunk * p.tiles_per_chunk; // the wave's own range first, then blocks of the pool
    int t1 = min(t0 + p.tiles_per_chunk, p.static_tiles);
    const int k = p.k;
    const int n = lane & 15, kq = lane >> 4;

    const int qrow = qtile * 16 + n;
    float qreg[NS * 8];
    {
        const float *qp = p.Q + (size_t)min(qrow, p.B - 1) * (NS * 32) + kq;
#pragma unroll
        for (int s = 0; s < NS * 8; ++s)
            qreg[s] = qrow < p.B ? qp[4 * s] : 0.0f;
    }
    float thr = INFINITY; // padded queries never qualify
    if (qrow < p.B)
        thr = (!MAXONLY && p.thr0) ? p.thr0[(size_t)qrow * p.thr0_stride + p.thr0_off] : -INFINITY;
    int cnt = 0; // the same value in the four lanes of a query
    float runmax = -INFINITY;
    Cand *const cbase = p.cand + ((size_t)task * 16 + n) * CAP;

    auto compact_where = [&](unsigned qmask) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        while (qmask) {
            const int q = __ffs((int)qmask) - 1;
            qmask &= qmask - 1;
            const int nn = __builtin_amdgcn_readlane(cnt, q);
            int n_new;
            float kth;
            bool have;
            compact_query<CAP>(p.cand + ((size_t)task * 16 + q) * CAP, nn, k, lane, n_new, kth, have);
            if (n == q) {
                cnt = n_new;
                if (have)
                    thr = kth;
            }
        }
    };

    // ---- DMA: K4's (slab = 32 docs x 32 features; instruction jj moves docs 8jj..8jj+7; lane -> (doc 8jj +
    //      lane>>3, physical 16-B chunk lane&7); logical chunk = physical ^ ((doc>>1)&7)) ----
    const char *Dbytes = (const char *)p.D;
    int dma_tile = t0, dma_s = 0;
    const char *rowp[DMA_PER_SLAB];
    auto set_rows = [&](int tile) {
#pragma unroll
        for (int jj = 0; jj < DMA_PER_SLAB; ++jj) {
            int di = 8 * jj + (lane >> 3);
            int doc = min(tile * TILE_DOCS + di, p.N - 1);
            int chunk16 = (lane & 7) ^ ((di >> 1) & 7);
            rowp[jj] = Dbytes + (size_t)doc * ROW_BYTES + chunk16 * 16;
        }
    };
    auto dma_issue = [&](int stage) {
        char *dst = ring + stage * SLAB_BYTES;
#pragma unroll
        for (int jj = 0; jj < DMA_PER_SLAB; ++jj)
            __builtin_amdgcn_global_load_lds((gbl_void *)(rowp[jj] + dma_s * 128),
                                             (lds_void *)(dst + jj * 1024), 16, 0, NT ? 2 : 0);
        if (++dma_s == NS) {
            dma_s = 0;
            dma_tile = min(dma_tile + 1, t1 - 1); // past the end: harmless re-read
            set_rows(dma_tile);
        }
    };

    for (;;) { // segments: the own range, then pool blocks
    if (t0 < t1) {
        set_rows(t0);
#pragma unroll
        for (int gi = 0; gi < NSTAGE - 1; ++gi)
            dma_issue(gi);
        // A element (sub-tile u, k-step t of the slab): row 16u + n, logical chunk t, float kq of the chunk
        const char *rd[2];
        int rsw[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int r = 16 * u + n;
            rd[u] = ring + r * 128 + 4 * kq;
            rsw[u] = (r >> 1) & 7;
        }
        int stage = 0;
        for (int tile = t0; tile < t1; ++tile) {
            f32x4 acc[2] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
            unsigned kw = 0xffffffffu; // the tile's keep word (MASKED: see score_topk_kernel)
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                asm volatile("s_waitcnt vmcnt(%0)" ::"n"(DMA_PER_SLAB * (NSTAGE - 2)) : "memory");
                float a[2][8];
#pragma unroll
                for (int t = 0; t < 8; ++t)
#pragma unroll
                    for (int u = 0; u < 2; ++u)
                        a[u][t] = *(const float *)(rd[u] + stage * SLAB_BYTES + ((t ^ rsw[u]) << 4));
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                if (MASKED && s == NS - 1) {
                    float a00[2] = {a[0][0], a[1][0]}; // (both chains' first operands)
                    keep_word_issue(p.keep + tile, kw, a00);
                    a[0][0] = a00[0];
                    a[1][0] = a00[1];
                }
                dma_issue((stage + NSTAGE - 1) % NSTAGE);
#pragma unroll
                for (int t = 0; t < 8; ++t) {
                    acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[0][t], qreg[8 * s + t], acc[0], 0, 0, 0);
                    acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[1][t], qreg[8 * s + t], acc[1], 0, 0, 0);
                }
                stage = (stage + 1) % NSTAGE;
            }
            // ---- epilogue: acc[u][r] = score(doc tile*32 + 16u + 4kq + r, query n) ----
            const int tile_base = tile * TILE_DOCS;
            const bool partial = tile_base + TILE_DOCS > p.N;
            unsigned kwh = 0xffffffffu; // MASKED: bit 16u + r = the keep bit of the lane's document (u, r)
            if (MASKED) {
                keep_word_wait(kw, acc[1]);
                kwh = kw >> (4 * kq);
            }
            auto kept = [&](int u, int r) { return !MASKED || ((kwh >> (16 * u + r)) & 1u) != 0u; };
            float m = -INFINITY; // over the documents that may be returned
#pragma unroll
            for (int u = 0; u < 2; ++u)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    m = fmaxf(m, ((!partial || tile_base + 16 * u + 4 * kq + r < p.N) && kept(u, r)) ? acc[u][r] : -INFINITY);
            if (MAXONLY) {
                runmax = fmaxf(runmax, m);
                continue;
            }
            if (__ballot(m >= thr) != 0ull) {
#pragma unroll
                for (int u = 0; u < 2; ++u)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int doc = tile_base + 16 * u + 4 * kq + r;
                        const bool c = (!partial || doc < p.N) && kept(u, r) && acc[u][r] >= thr;
                        const unsigned long long mask = __ballot(c);
                        if (mask == 0ull)
                            continue;
                        // the four lanes of query n sit at n, n+16, n+32, n+48: slots in kq order
                        const int b0 = (int)((mask >> n) & 1ull), b1 = (int)((mask >> (n + 16)) & 1ull);
                        const int b2 = (int)((mask >> (n + 32)) & 1ull), b3 = (int)((mask >> (n + 48)) & 1ull);
                        const int before = (kq > 0 ? b0 : 0) + (kq > 1 ? b1 : 0) + (kq > 2 ? b2 : 0);
                        if (c)
                            cand_store_async(cbase + cnt + before, acc[u][r], doc);
                        cnt += b0 + b1 + b2 + b3;
                    }
                // one tile adds at most 32 entries per query: compact while there is still room for that
                const unsigned long long full = __ballot(cnt > CAP - 34) & 0xffffull;
                if (full)
                    compact_where((unsigned)full);
            }
        }
    }
    if (MAXONLY || !p.tail_ctr)
        break;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // the over-prefetch of the segment's end has landed: the ring is free
    int blk = 0;
    if (lane == 0)
        blk = atomicAdd(p.tail_ctr + qtile, 1);
    blk = __builtin_amdgcn_readfirstlane(blk);
    if (blk >= p.tail_blocks)
        break;
    t0 = p.static_tiles + blk * p.tail_g;
    t1 = min(t0 + p.tail_g, p.n_tiles);
    dma_tile = t0;
    dma_s = 0;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

    if (MAXONLY) {
        runmax = fmaxf(runmax, __shfl_xor(runmax, 16));
        runmax = fmaxf(runmax, __shfl_xor(runmax, 32));
        if (kq == 0 && qrow < p.B) {
            const size_t o = (size_t)qrow * p.n_chunks + chunk;
            p.pval[o] = runmax;
            p.pidx[o] = t0 < t1 ? (int64_t)chunk : -1;
        }
        return;
    }
    {
        const unsigned long long over = __ballot(cnt > k) & 0xffffull;
        if (over)
            compact_where((unsigned)over);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    const int rows_live = min(16, p.B - qtile * 16);
    for (int it0 = 0; it0 < rows_live * k; it0 += 64) { // wave-uniform trip count: see score_topk_kernel's output loop
        const int it = it0 + lane;
        const int q = min(it / k, rows_live - 1), t = it - q * k;
        const int nn = __shfl(cnt, q);
        if (it >= rows_live * k)
            continue;
        const size_t o = ((size_t)(qtile * 16 + q) * p.n_chunks + chunk) * k + t;
        Cand c;
        c.v = -INFINITY;
        c.x = -1;
        if (t < nn)
            c = cand_load_l2(p.cand + ((size_t)task * 16 + q) * CAP + t);
        p.pval[o] = c.v;
        p.pidx[o] = t < nn ? p.idx_offset + c.x : -1;
    }
}

// ---------------------------------------------------------------------------
// K5: top-k of M unordered candidates per query, (score desc, index asc).
// One block per query.  The candidates are scanned ONCE: valid entries (idx >= 0; most
// partial-list slots are padding) are packed into an LDS pool; whenever the pool could overflow
// it is reduced to its k best.  The final reduction emits the sorted top-k.  A reduction is k
// rounds of block-wide arg-best over the pool, each round picking the best entry that ranks
// strictly after the previous pick.
// ---------------------------------------------------------------------------
constexpr int MERGE_THREADS = 256;
constexpr int MERGE_POOL = 6144;                 // LDS pool entries (12 B each)
constexpr int MERGE_SEG = MERGE_THREADS * 16;    // candidates scanned between overflow checks
constexpr int MERGE_KMAX = 64;

__device__ __forceinline__ bool ranks_before(float sa, int64_t ia, float sb, int64_t ib)
{
    return sa > sb || (sa == sb && ia < ib);
}

// Block-wide: the best pool entry ranking strictly after (pv,pi).  Returns bi == INT64_MAX if none.
__device__ __forceinline__ void pool_next_best(const float *pool_v, const int64_t *pool_i, int n, float pv,
                                               int64_t pi, float *red_v, int64_t *red_i, float &bv, int64_t &bi)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    bv = -INFINITY;
    bi = INT64_MAX;
    for (int m = tid; m < n; m += MERGE_THREADS) {
        const float cv = pool_v[m];
        const int64_t ci = pool_i[m];
        if (!ranks_before(pv, pi, cv, ci))
            continue;
        if (bi == INT64_MAX || ranks_before(cv, ci, bv, bi)) {
            bv = cv;
            bi = ci;
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const float ov = __shfl_xor(bv, off);
        const int64_t oi = __shfl_xor(bi, off);
        if (oi != INT64_MAX && (bi == INT64_MAX || ranks_before(ov, oi, bv, bi))) {
            bv = ov;
            bi = oi;
        }
    }
    if (lane == 0) {
        red_v[wave] = bv;
        red_i[wave] = bi;
    }
    __syncthreads();
    bv = red_v[0];
    bi = red_i[0];
#pragma unroll
    for (int w = 1; w < MERGE_THREADS / 64; ++w) {
        const float ov = red_v[w];
        const int64_t oi = red_i[w];
        if (oi != INT64_MAX && (bi == INT64_MAX || ranks_before(ov, oi, bv, bi))) {
            bv = ov;
            bi = oi;
        }
    }
    __syncthreads();
}

// Candidate m of row b lives in segment m / seg_len at [b][m % seg_len]; segment s starts seg_stride BYTES
// after segment s-1 (one segment of length M = a plain [B,M] matrix; `world` segments of length k' = the
// all-gathered per-shard lists of ShardedIndex, read in place).
__global__ __launch_bounds__(MERGE_THREADS) void topk_merge_kernel(const float *__restrict__ in_val,
                                                                   const int64_t *__restrict__ in_idx,
                                                                   int M, int k, float *out_val,
                                                                   int64_t *out_idx, const int *run_if,
                                                                   int seg_len, size_t seg_stride)
{
    if (run_if && run_if[blockIdx.x >> 5] == 0)
        return;
    __shared__ float pool_v[MERGE_POOL];
    __shared__ int64_t pool_i[MERGE_POOL];
    __shared__ float top_v[MERGE_KMAX];
    __shared__ int64_t top_i[MERGE_KMAX];
    __shared__ float red_v[MERGE_THREADS / 64];
    __shared__ int64_t red_i[MERGE_THREADS / 64];
    __shared__ int pool_n;
    const int b = blockIdx.x, tid = threadIdx.x;
    auto v_at = [&](int m) -> float {
        const int sg = m / seg_len, wi = m - sg * seg_len;
        return ((const float *)((const char *)in_val + (size_t)sg * seg_stride))[(size_t)b * seg_len + wi];
    };
    auto ix_at = [&](int m) -> int64_t {
        const int sg = m / seg_len, wi = m - sg * seg_len;
        return ((const int64_t *)((const char *)in_idx + (size_t)sg * seg_stride))[(size_t)b * seg_len + wi];
    };
    if (tid == 0)
        pool_n = 0;
    __syncthreads();

    // reduce the pool to its k best (sorted) in place; returns the new size
    auto reduce_pool = [&]() {
        const int n = pool_n;
        float pv = INFINITY;
        int64_t pi = -1;
        int kept = 0;
        for (int r = 0; r < k; ++r) {
            float bv;
            int64_t bi;
            pool_next_best(pool_v, pool_i, n, pv, pi, red_v, red_i, bv, bi);
            if (bi == INT64_MAX)
                break;
            if (tid == 0) {
                top_v[r] = bv;
                top_i[r] = bi;
            }
            pv = bv;
            pi = bi;
            kept = r + 1;
        }
        __syncthreads();
        if (tid < kept) {
            pool_v[tid] = top_v[tid];
            pool_i[tid] = top_i[tid];
        }
        if (tid == 0)
            pool_n = kept;
        __syncthreads();
        return kept;
    };

    for (int base = 0; base < M; base += MERGE_SEG) {
        if (pool_n + MERGE_SEG > MERGE_POOL) // block-uniform (pool_n read after a barrier)
            reduce_pool();
        const int end = min(base + MERGE_SEG, M);
        int64_t ci[MERGE_SEG / MERGE_THREADS];
#pragma unroll
        for (int u = 0; u < MERGE_SEG / MERGE_THREADS; ++u) { // all index loads in flight together
            const int m = base + tid + u * MERGE_THREADS;
            ci[u] = m < end ? ix_at(m) : -1;
        }
#pragma unroll
        for (int u = 0; u < MERGE_SEG / MERGE_THREADS; ++u) {
            if (ci[u] >= 0) {
                const int slot = atomicAdd(&pool_n, 1);
                pool_v[slot] = v_at(base + tid + u * MERGE_THREADS);
                pool_i[slot] = ci[u];
            }
        }
        __syncthreads();
    }
    const int kept = reduce_pool();
    if (tid < k) {
        out_val[(size_t)b * k + tid] = tid < kept ? pool_v[tid] : -INFINITY;
        out_idx[(size_t)b * k + tid] = tid < kept ? pool_i[tid] : -1;
    }
}

// ---------------------------------------------------------------------------
// k-th largest of M values per row (threshold seeding): 4-pass radix select on the order-preserving
// integer image of the floats; one block per row, cost independent of k.  -inf when M < k.
// ---------------------------------------------------------------------------
__device__ __forceinline__ unsigned order_key(float f)
{
    const unsigned b = __float_as_uint(f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

__device__ __forceinline__ float order_key_to_float(unsigned key)
{
    return __uint_as_float((key & 0x80000000u) ? (key & 0x7fffffffu) : ~key);
}

// top_out (nullable): [rows][k], receives the row's k largest values, UNORDERED (the values above the k-th in arrival
// order, then copies of the k-th; -inf padding when M < k) -- what a shard contributes to the union seed of a sharded
// search (tt_score_topk_screened_seed_list_f32).
__global__ __launch_bounds__(256) void kth_largest_kernel(const float *__restrict__ vals, int M, int k,
                                                          float *__restrict__ out, const int *run_if,
                                                          float *__restrict__ top_out)
{
    if (run_if && run_if[blockIdx.x >> 5] == 0)
        return;
    __shared__ int hist[256];
    __shared__ int sel[2];
    __shared__ int wpos;
    const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const float *v = vals + (size_t)row * M;
    if (M < k) {
        if (tid == 0 && out)
            out[row] = -INFINITY;
        if (top_out)
            for (int i = tid; i < k; i += 256)
                top_out[(size_t)row * k + i] = i < M ? v[i] : -INFINITY;
        return;
    }
    unsigned prefix = 0u, mask = 0u;
    int k_rem = k;
    // up to 256 x KTH_REG values (every seeding pass of the searches) are read ONCE into registers; the four passes then
    // run on those (four passes of dependent global loads were 16 us per search, three quarters of this kernel)
    constexpr int KTH_REG = 16;
    const bool in_regs = M <= 256 * KTH_REG;
    unsigned keys[KTH_REG];
    if (in_regs) {
#pragma unroll
        for (int i = 0; i < KTH_REG; ++i) {
            const int m = tid + 256 * i;
            keys[i] = m < M ? order_key(v[m]) : 0u; // (key 0 = below every float: never selected while M >= k)
        }
    }
#pragma unroll 1
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = 24 - 8 * pass;
        hist[tid] = 0;
        __syncthreads();
        if (in_regs) {
#pragma unroll
            for (int i = 0; i < KTH_REG; ++i)
                if (tid + 256 * i < M && (keys[i] & mask) == prefix)
                    atomicAdd(&hist[(keys[i] >> shift) & 255u], 1);
        } else {
            for (int m = tid; m < M; m += 256) {
                const unsigned key = order_key(v[m]);
                if ((key & mask) == prefix)
                    atomicAdd(&hist[(key >> shift) & 255u], 1);
            }
        }
        __syncthreads();
        if (tid < 64) { // one wave: suffix sums over the 256 bins (4 bins per lane, high bins first)
            int c[4], s = 0;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                c[i] = hist[255 - (lane * 4 + i)];
                s += c[i];
            }
            int incl = s; // inclusive scan over lanes
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const int y = __shfl_up(incl, off);
                if (lane >= off)
                    incl += y;
            }
            int above = incl - s; // entries in strictly higher bins than this lane's first
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (above < k_rem && above + c[i] >= k_rem) {
                    sel[0] = 255 - (lane * 4 + i);
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
    const float kth = order_key_to_float(prefix);
    if (tid == 0 && out)
        out[row] = kth;
    if (top_out) {
        // k - k_rem values are strictly above the k-th (k_rem = the k-th's rank among its equals): they go first, in
        // arrival order; the remaining k_rem slots are copies of the k-th
        if (tid == 0)
            wpos = 0;
        __syncthreads();
        float *dst = top_out + (size_t)row * k;
        if (in_regs) {
#pragma unroll
            for (int i = 0; i < KTH_REG; ++i)
                if (tid + 256 * i < M && keys[i] > prefix)
                    dst[atomicAdd(&wpos, 1)] = order_key_to_float(keys[i]);
        } else {
            for (int m = tid; m < M; m += 256)
                if (order_key(v[m]) > prefix)
                    dst[atomicAdd(&wpos, 1)] = v[m];
        }
        for (int i = k - k_rem + tid; i < k; i += 256)
            dst[i] = kth;
    }
}

// ---------------------------------------------------------------------------
// Rank of a designated document (BatchEvaluator, evaluators.py:58-65).
// One block per query; scores are the same ascending-index FMA chain, one lane per document (the chain is
// sequential by definition).  A wave takes 64 documents at a time and stages them 32 features at a time through LDS:
// the global reads are whole 128-byte row segments (8 lanes x 16 B per row), the chain reads its own row from a
// 33-float-stride image (conflict-free).
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void score_rank_kernel(const float *__restrict__ Q,
                                                         const float *__restrict__ D, int N, int d,
                                                         const int64_t *__restrict__ target,
                                                         int64_t *rank)
{
    __shared__ float qs[512];
    __shared__ float stage[4][64 * 33];
    __shared__ int cnt[4];
    const int b = blockIdx.x, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int tg = (int)target[b];
    for (int x = threadIdx.x; x < d; x += 256)
        qs[x] = Q[(size_t)b * d + x];
    __syncthreads();
    float st = 0.0f;
    {
        const float *row = D + (size_t)tg * d;
        for (int x = 0; x < d; ++x)
            st = fmaf(qs[x], row[x], st);
    }
    float *img = stage[wv];
    int c = 0;
    for (int n0 = wv * 64; n0 < N; n0 += 256) { // wave-uniform trip count
        float acc = 0.0f;
        for (int x0 = 0; x0 < d; x0 += 32) {
#pragma unroll
            for (int i = 0; i < 8; ++i) { // rows 8 i + lane / 8, 16-byte chunk lane % 8
                const int r = 8 * i + (lane >> 3), n = min(n0 + r, N - 1);
                f32x4 v = {0, 0, 0, 0};
                if (x0 + 4 * (lane & 7) < d) // d is a multiple of 4, not necessarily of 32
                    v = *(const f32x4 *)(D + (size_t)n * d + x0 + 4 * (lane & 7));
                float *dst = img + r * 33 + 4 * (lane & 7);
                dst[0] = v.x;
                dst[1] = v.y;
                dst[2] = v.z;
                dst[3] = v.w;
            }
            __builtin_amdgcn_wave_barrier();
            const float *mine = img + lane * 33;
            const int xe = min(32, d - x0);
            for (int x = 0; x < xe; ++x)
                acc = fmaf(qs[x0 + x], mine[x], acc);
            __builtin_amdgcn_wave_barrier();
        }
        const int n = n0 + lane;
        c += (n < N) && (n != tg) && (acc > st || (acc == st && n < tg));
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1)
        c += __shfl_xor(c, off);
    if (lane == 0)
        cnt[wv] = c;
    __syncthreads();
    if (threadIdx.x == 0)
        rank[b] = 1 + (int64_t)cnt[0] + cnt[1] + cnt[2] + cnt[3];
}

// All scores of a query: S[b][n] = the ascending-index FMA chain of <Q[b], D[n]> (the scores score_topk selects from),
// for the callers that blend the dense score of EVERY document with another signal (backend/simple_hybrid.py:53-56).
// grid (ceil(N / 256), B); a wave takes 64 documents, staged 32 features at a time through LDS like score_rank_kernel.
__global__ __launch_bounds__(256) void score_all_kernel(const float *__restrict__ Q, const float *__restrict__ D, int N,
                                                        int d, float *__restrict__ S)
{
    __shared__ float qs[512];
    __shared__ float stage[4][64 * 33];
    const int b = blockIdx.y, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int x = threadIdx.x; x < d; x += 256)
        qs[x] = Q[(size_t)b * d + x];
    __syncthreads();
    float *img = stage[wv];
    const int n0 = blockIdx.x * 256 + wv * 64;
    if (n0 >= N)
        return; // wave-uniform; no block barrier below
    float acc = 0.0f;
    for (int x0 = 0; x0 < d; x0 += 32) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int r = 8 * i + (lane >> 3), n = min(n0 + r, N - 1);
            f32x4 v = {0, 0, 0, 0};
            if (x0 + 4 * (lane & 7) < d)
                v = *(const f32x4 *)(D + (size_t)n * d + x0 + 4 * (lane & 7));
            float *dst = img + r * 33 + 4 * (lane & 7);
            dst[0] = v.x;
            dst[1] = v.y;
            dst[2] = v.z;
            dst[3] = v.w;
        }
        __builtin_amdgcn_wave_barrier();
        const float *mine = img + lane * 33;
        const int xe = min(32, d - x0);
        for (int x = 0; x < xe; ++x)
            acc = fmaf(qs[x0 + x], mine[x], acc);
        __builtin_amdgcn_wave_barrier();
    }
    if (n0 + lane < N)
        S[(size_t)b * N + n0 + lane] = acc;
}

// One launch of score_topk_kernel over docs [0,N): how the work is cut and where its
// partial lists live inside the workspace.
struct Pass {
    int n_qtiles, n_tiles, n_chunks, tiles_per_chunk, n_tasks;
    int tail_own, static_tiles, tail_g, tail_blocks; // with the pool on: tail_own tiles per chunk are static (see ScoreParams)
    int64_t N;
};

struct Plan {
    int cap;       // candidate-buffer entries per (wave, query): 64 (k <= 16) or 128
    size_t smem;   // dynamic LDS per block
    Pass main, pre;
    bool prepass;  // sample pass first: its k-th scores seed the main pass's thresholds
    // workspace layout (byte offsets)
    size_t cand_off, pval_off, pidx_off, pre_val_off, pre_idx_off, tailctr_off, ws_bytes;
    // three or more query tiles on the 32-query kernel: pacing counters and the chunks' pool draws behind the pool counter(s)
    bool paced;
    int pace_g, pace_lag;
    int grp_maxseg;
    size_t pace_off, grp_off, ctr_bytes; // ctr_bytes: pool counter(s) + pacing + draws, zeroed together before the main pass
    size_t redo_off; // one int per query tile: a wave of the tile gave up a pool draw -> the static-split pass redoes the tile
};

bool tt_score_pacing() // TT_SCORE_PACE=0: every wave for itself (measurement)
{
    return TT_AB_SWITCH(TT_SCORE_PACE, 1) != 0;
}

Pass make_pass(int B, int64_t N, int slots, int qt, bool tail = false)
{
    Pass ps;
    ps.N = N;
    ps.n_qtiles = (B + qt - 1) / qt; // qt queries per task: 32, or 16 for wide embeddings (d > 256)
    ps.n_tiles = (int)((N + TILE_DOCS - 1) / TILE_DOCS);
    const TTChunks c = tt_chunks(ps.n_tiles, (slots + ps.n_qtiles - 1) / ps.n_qtiles, INT_MAX);
    ps.tiles_per_chunk = c.tiles_per_chunk;
    ps.n_chunks = c.n_chunks;
    ps.n_tasks = ps.n_qtiles * ps.n_chunks;
    // pool = the last 1/TT_SCORE_TAIL_DIV of every chunk's share (0: everything static) in blocks of a quarter of it,
    // 4..64 tiles (a block costs one refill of the wave's ring, ~2 us)
    const TTTailSplit t = tt_tail_split(ps.tiles_per_chunk, ps.n_chunks, ps.n_tiles, tail ? TT_AB_SWITCH(TT_SCORE_TAIL_DIV, 8) : 0,
                                        8, 4, 64);
    ps.tail_own = t.own;
    ps.static_tiles = t.static_tiles;
    ps.tail_g = t.tail_g;
    ps.tail_blocks = t.tail_blocks;
    return ps;
}

// Prepass policy.  A wave's private list costs ~k(1+ln(n/k)) candidate appends per query for the
// n documents it sees, so cutting the corpus over ~2048 waves multiplies the selection work.  When
// chunks are short, first take the exact top-k of a 1/256 sample: its k-th score is a valid lower
// bound of the final k-th score, and with it the main pass admits only ~256k candidates per query
// in total.  Long chunks (large B) do not need it.
constexpr int64_t PREPASS_MIN_N = 262144;
constexpr int PREPASS_MAX_CHUNK_DOCS = 65536;
constexpr int64_t PREPASS_MIN_SAMPLE = 16384;

// bf16: bf16 document rows (tt_score_topk_bf16), which run on 32-query tiles at every batch size; for B > 16 the
// workspace layout is the fp32 one (only the pacing block length, a kernel argument, depends on the row bytes)
Plan make_plan(int B, int64_t N, int k, int d, bool bf16 = false)
{
    Plan pl;
    const int qt = (!bf16 && (d > 256 || B <= 16)) ? 16 : 32; // 16-query tiles: wide embeddings, and batches that fit one such tile
    pl.cap = k <= 16 ? 64 : 128;
    pl.smem = (size_t)WPB * NSTAGE * SLAB_BYTES;
    const int slots = tt_device_cus() * 8;
    pl.main = make_pass(B, N, slots, qt, true);
    pl.prepass = N >= PREPASS_MIN_N && (int64_t)pl.main.tiles_per_chunk * TILE_DOCS < PREPASS_MAX_CHUNK_DOCS;
    int max_tasks = pl.main.n_tasks;
    if (pl.prepass) {
        int64_t ns = N / 256;
        ns = ns < PREPASS_MIN_SAMPLE ? PREPASS_MIN_SAMPLE : ns;
        ns = (ns + TILE_DOCS - 1) / TILE_DOCS * TILE_DOCS;
        pl.pre = make_pass(B, ns, slots, qt);
        max_tasks = pl.pre.n_tasks > max_tasks ? pl.pre.n_tasks : max_tasks;
    } else {
        pl.pre = make_pass(B, 0, slots, qt);
    }
    const size_t rows = (size_t)pl.main.n_qtiles * qt;
    size_t max_chunks = pl.main.n_chunks;
    if (pl.prepass && (size_t)pl.pre.n_chunks > max_chunks)
        max_chunks = pl.pre.n_chunks;
    TTWorkspace ws;
    pl.cand_off = ws.take((size_t)max_tasks * qt * pl.cap * 8);
    pl.pval_off = ws.take(rows * max_chunks * k * sizeof(float));
    pl.pidx_off = ws.take(rows * max_chunks * k * sizeof(int64_t));
    pl.pre_val_off = ws.take(rows * k * sizeof(float));
    pl.pre_idx_off = ws.take(rows * k * sizeof(int64_t));
    pl.tailctr_off = ws.take((size_t)pl.main.n_qtiles * sizeof(int));
    // (32-query tiles only: the redo pass in tt_score_topk_f32_pred keeps one flag per 32 queries)
    pl.paced = qt == 32 && pl.main.n_qtiles >= 3; // (two query tiles: +0.7 % with it, 1.7x fetched either way)
    {
        // the chunks of one XCD (an eighth of them) share its 4 MiB L2: a chunk's waves must stay within its part of
        // ~3 MiB of each other, i.e. (pace_lag + 1) * pace_g tiles
        const int env_g = TT_AB_SWITCH(TT_SCORE_PACE_G, 0);
        const int env_lag = TT_AB_SWITCH(TT_SCORE_PACE_LAG, 0);
        const int64_t per_xcd = (pl.main.n_chunks + 7) / 8;
        const int64_t window = (3 << 20) / (per_xcd * TILE_DOCS * d * (bf16 ? 2 : 4)); // tiles
        pl.pace_lag = env_lag > 0 ? env_lag : 2;
        int g = (int)(window / (pl.pace_lag + 1));
        pl.pace_g = env_g > 0 ? env_g : (g < 1 ? 1 : (g > 8 ? 8 : g));
        if (pl.pace_lag > PACE_R - 2)
            pl.pace_lag = PACE_R - 2;
    }
    pl.grp_maxseg = 0;
    pl.pace_off = pl.grp_off = ws.off;
    if (pl.paced) {
        ws.take(((size_t)pl.main.n_chunks * PACE_R + 1) * sizeof(int)); // + the time-out count
        pl.grp_off = ws.off;
        if (pl.main.tail_blocks > 0) {
            // a chunk's waves may take up to 4x their even share of the pool (>= 16 blocks); n_chunks * grp_maxseg >=
            // tail_blocks, so every block is drawn by a chunk that still may
            const int even = (pl.main.tail_blocks + pl.main.n_chunks - 1) / pl.main.n_chunks;
            pl.grp_maxseg = 4 * even > 16 ? 4 * even : 16;
            ws.take((size_t)pl.main.n_chunks * pl.grp_maxseg * sizeof(int));
        }
    }
    pl.ctr_bytes = ws.off - pl.tailctr_off;
    pl.redo_off = ws.take((size_t)pl.main.n_qtiles * sizeof(int));
    pl.ws_bytes = ws.off;
    return pl;
}

constexpr bool score_dim_ok(int d, bool bf16 = false)
{
    if (bf16)
        return d == 64 || d == 128 || d == 192 || d == 256;
    return d == 32 || d == 64 || d == 96 || d == 128 || d == 192 || d == 256 || d == 320 || d == 384 || d == 448 || d == 512;
}

// The kernel families, for launch_ns: score_topk_kernel (32-query tiles) over fp32 and over bf16 rows, and
// score_topk16_kernel (16-query tiles).
struct Score32 {
    template <int NS, int CAP, bool MAXONLY, bool NT, bool MASKED>
    static const void *fn() { return (const void *)score_topk_kernel<NS, CAP, MAXONLY, NT, false, MASKED>; }
    static constexpr size_t smem_nt = (size_t)WPB * NSTAGE_NT * SLAB_BYTES; // the NT form's own ring depth
};
struct Score32Bf16 {
    template <int NS, int CAP, bool MAXONLY, bool NT, bool MASKED>
    static const void *fn() { return (const void *)score_topk_kernel<NS, CAP, MAXONLY, NT, true, MASKED>; }
    static constexpr size_t smem_nt = Score32::smem_nt;
};
struct Score16 {
    template <int NS, int CAP, bool MAXONLY, bool NT, bool MASKED>
    static const void *fn() { return (const void *)score_topk16_kernel<NS, CAP, MAXONLY, NT, MASKED>; }
    static constexpr size_t smem_nt = (size_t)WPB * NSTAGE * SLAB_BYTES;
};

template <class K, int NS, bool MASKED>
int launch_ns_m(const ScoreParams &sp, const Plan &pl, hipStream_t st, bool maxonly)
{
    const void *fn;
    size_t smem = pl.smem;
    if (maxonly) {
        fn = K::template fn<NS, 64, true, false, MASKED>();
    } else if (NS == 8 && sp.n_qtiles == 1) { // (d = 256 only: the instantiations are not free)
        fn = pl.cap == 64 ? K::template fn<8, 64, false, true, MASKED>() : K::template fn<8, 128, false, true, MASKED>();
        smem = K::smem_nt;
    } else {
        fn = pl.cap == 64 ? K::template fn<NS, 64, false, false, MASKED>() : K::template fn<NS, 128, false, false, MASKED>();
    }
    TT_HIP_CHECK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
    ScoreParams args = sp;
    void *argv[] = {&args};
    TT_HIP_CHECK(hipLaunchKernel(fn, dim3((sp.n_tasks + WPB - 1) / WPB), dim3(WPB * 64), argv, smem, st));
    return TT_OK;
}

// sp.keep set: the MASKED instantiation of the same kernel
template <class K, int NS>
int launch_ns(const ScoreParams &sp, const Plan &pl, hipStream_t st, bool maxonly)
{
    return sp.keep ? launch_ns_m<K, NS, true>(sp, pl, st, maxonly) : launch_ns_m<K, NS, false>(sp, pl, st, maxonly);
}

int launch_score(int d, const ScoreParams &sp, const Plan &pl, hipStream_t st, bool maxonly, bool bf16)
{
    if (bf16) { // (score_dim_ok: 64 <= d <= 256, 32-query tiles at every B)
        switch (d) {
        case 64: return launch_ns<Score32Bf16, 2>(sp, pl, st, maxonly);
        case 128: return launch_ns<Score32Bf16, 4>(sp, pl, st, maxonly);
        case 192: return launch_ns<Score32Bf16, 6>(sp, pl, st, maxonly);
        default: return launch_ns<Score32Bf16, 8>(sp, pl, st, maxonly);
        }
    }
    if (d <= 256 && sp.B <= 16) { // half the MFMA work of a 32-query tile: the launch stays on the HBM roofline
        switch (d) {
        case 32: return launch_ns<Score16, 1>(sp, pl, st, maxonly);
        case 64: return launch_ns<Score16, 2>(sp, pl, st, maxonly);
        case 96: return launch_ns<Score16, 3>(sp, pl, st, maxonly);
        case 128: return launch_ns<Score16, 4>(sp, pl, st, maxonly);
        case 192: return launch_ns<Score16, 6>(sp, pl, st, maxonly);
        default: return launch_ns<Score16, 8>(sp, pl, st, maxonly);
        }
    }
    switch (d) {
    case 320: return launch_ns<Score16, 10>(sp, pl, st, maxonly);
    case 384: return launch_ns<Score16, 12>(sp, pl, st, maxonly);
    case 448: return launch_ns<Score16, 14>(sp, pl, st, maxonly);
    case 512: return launch_ns<Score16, 16>(sp, pl, st, maxonly);
    case 32: return launch_ns<Score32, 1>(sp, pl, st, maxonly);
    case 64: return launch_ns<Score32, 2>(sp, pl, st, maxonly);
    case 96: return launch_ns<Score32, 3>(sp, pl, st, maxonly);
    case 128: return launch_ns<Score32, 4>(sp, pl, st, maxonly);
    case 192: return launch_ns<Score32, 6>(sp, pl, st, maxonly);
    default: return launch_ns<Score32, 8>(sp, pl, st, maxonly);
    }
}

ScoreParams pass_params(const Pass &ps, const float *Q, int B, const void *D, int k, int64_t idx_offset, char *ws,
                        const Plan &pl)
{
    ScoreParams sp;
    sp.Q = Q;
    sp.D = D;
    sp.B = B;
    sp.N = (int)ps.N;
    sp.k = k;
    sp.n_qtiles = ps.n_qtiles;
    sp.n_chunks = ps.n_chunks;
    sp.tiles_per_chunk = ps.tiles_per_chunk;
    sp.n_tiles = ps.n_tiles;
    sp.n_tasks = ps.n_tasks;
    sp.static_tiles = ps.n_tiles; // (the caller turns the pool on for the main pass)
    sp.tail_g = 1;
    sp.tail_blocks = 0;
    sp.tail_ctr = nullptr;
    sp.pace = nullptr;
    sp.pace_timeouts = nullptr;
    sp.pace_g = sp.pace_lag = 1;
    sp.grp_blk = nullptr;
    sp.grp_maxseg = 0;
    sp.pval = (float *)(ws + pl.pval_off);
    sp.pidx = (int64_t *)(ws + pl.pidx_off);
    sp.idx_offset = idx_offset;
    sp.cand = (Cand *)(ws + pl.cand_off);
    sp.thr0 = nullptr;
    sp.thr0_stride = 0;
    sp.thr0_off = 0;
    sp.run_if = nullptr;
    sp.draw_polls = TT_AB_SWITCH(TT_DRAW_POLLS, DRAW_POLLS);
    sp.keep = nullptr;
    return sp;
}

// The supported widths, for error messages.
const char *score_dims(bool bf16)
{
    return bf16 ? "64, 128, 192, 256" : "32, 64, 96, 128, 192, 256, 320, 384, 448, 512";
}

// D: fp32 rows, or bf16 rows when bf16 is set.
// k_seed (0 = k): the rank whose sample score seeds the main pass -- the FINAL k of a large-k search, whose main pass keeps
// lists of k = 64 (tt_score_topk_large_f32: a seed for the 64th score would drop documents ranked 65..k_seed)
int score_partials(const float *Q, int B, int d, const void *D, bool bf16, int64_t N, int k, int64_t idx_offset,
                   void *workspace, size_t workspace_bytes, hipStream_t st, Plan *plan_out, const char *who,
                   const int *run_if = nullptr, void *const *prof_events = nullptr, int k_seed = 0,
                   const unsigned *keep = nullptr)
{
    if (B <= 0 || N <= 0 || k <= 0)
        return tt_fail(TT_ERR_BAD_SHAPE, "%s: B=%d N=%lld k=%d", who, B, (long long)N, k);
    if (!score_dim_ok(d, bf16))
        return tt_fail(TT_ERR_UNSUPPORTED, "%s: d=%d (supported: %s)", who, d, score_dims(bf16));
    if (k > 64)
        return tt_fail(TT_ERR_UNSUPPORTED, "%s: k=%d > 64", who, k);
    if (N >= (int64_t)INT_MAX - 64)
        return tt_fail(TT_ERR_UNSUPPORTED, "%s: N=%lld >= 2^31-64; shard the corpus", who, (long long)N);
    if (!Q || !D)
        return tt_fail(TT_ERR_BAD_SHAPE, "%s: null pointer", who);
    const Plan pl = make_plan(B, N, k, d, bf16);
    if (!workspace || workspace_bytes < pl.ws_bytes)
        return tt_fail(TT_ERR_WORKSPACE, "%s: workspace %zu < %zu bytes", who, workspace_bytes, pl.ws_bytes);
    if (((uintptr_t)D & 15) || ((uintptr_t)Q & 3) || ((uintptr_t)workspace & 255))
        return tt_fail(TT_ERR_BAD_SHAPE, "%s: D must be 16-byte and the workspace 256-byte aligned", who);
    char *ws = (char *)workspace;
    *plan_out = pl;
    const float *thr0 = nullptr;
    // (the predicated form -- the screened search's on-device fallback, a no-op unless a flag is raised -- skips
    //  the sample pass: it only seeds thresholds, and two fewer empty launches sit behind every screened search)
    if (pl.prepass && !run_if) {
        // sample pass over D[0:ns): per-(wave,query) maxima, then their k-th largest per query.
        // k distinct documents score at least that much, so it bounds the final k-th score from below.
        // (keep: the maxima are over the kept documents of the sample -- the first words of the mask -- and a chunk with none
        //  contributes -inf: only documents that may be returned vouch for the bound)
        ScoreParams pp = pass_params(pl.pre, Q, B, D, k, 0, ws, pl);
        pp.run_if = run_if;
        pp.keep = keep;
        int rc = launch_score(d, pp, pl, st, true, bf16);
        if (rc != TT_OK)
            return rc;
        hipLaunchKernelGGL(kth_largest_kernel, dim3(B), dim3(256), 0, st, (const float *)pp.pval, pl.pre.n_chunks,
                           k_seed > 0 ? k_seed : k, (float *)(ws + pl.pre_val_off), run_if, (float *)nullptr);
        TT_LAUNCH_CHECK();
        thr0 = (const float *)(ws + pl.pre_val_off);
    }
    ScoreParams sp = pass_params(pl.main, Q, B, D, k, idx_offset, ws, pl);
    sp.thr0 = thr0;
    sp.thr0_stride = 1;
    sp.thr0_off = 0;
    sp.run_if = run_if;
    sp.keep = keep;
    if (pl.main.tail_blocks > 0 && !run_if) {
        // (the predicated form keeps the static split: its launches sit behind every screened search as no-ops, and a
        //  counter reset would be one more)
        sp.tiles_per_chunk = pl.main.tail_own;
        sp.static_tiles = pl.main.static_tiles;
        sp.tail_g = pl.main.tail_g;
        sp.tail_blocks = pl.main.tail_blocks;
        sp.tail_ctr = (int *)(ws + pl.tailctr_off);
    }
    if (pl.paced && !run_if && tt_score_pacing()) {
        sp.pace = (int *)(ws + pl.pace_off);
        sp.pace_timeouts = sp.pace + (size_t)pl.main.n_chunks * PACE_R;
        sp.pace_g = pl.pace_g;
        sp.pace_lag = pl.pace_lag;
        if (sp.tail_ctr) {
            sp.grp_blk = (int *)(ws + pl.grp_off);
            sp.grp_maxseg = pl.grp_maxseg;
        }
    }
    if (sp.tail_ctr || sp.pace)
        TT_RC_CHECK(tt_zero_async(ws + pl.tailctr_off, pl.ctr_bytes, st));
    if (prof_events)
        TT_HIP_CHECK(hipEventRecord((hipEvent_t)prof_events[0], st));
    const int rc = launch_score(d, sp, pl, st, false, bf16);
    if (prof_events && rc == TT_OK)
        TT_HIP_CHECK(hipEventRecord((hipEvent_t)prof_events[1], st));
    return rc;
}

} // namespace

// Byte offset, in the workspace of a finished tt_score_topk(_partials)_f32 call of this shape, of an int32 that counts the waves
// whose pacing wait ran into its bound (0 when the launch was not paced): (size_t)-1 if the shape is never paced.
TT_EXPORT size_t tt_score_topk_pace_timeouts_offset(int B, int64_t N, int d, int k)
{
    if (B <= 0 || N <= 0 || k <= 0)
        return (size_t)-1;
    const Plan pl = make_plan(B, N, k, d);
    return pl.paced ? pl.pace_off + (size_t)pl.main.n_chunks * PACE_R * sizeof(int) : (size_t)-1;
}

// Diagnostic: byte offset of the per-query-tile flags (int32 each) that say which tiles the last tt_score_topk_f32 call of this
// shape did again because a wave had given up a pool draw; (size_t)-1 = the shape never draws from a shared pool.
TT_EXPORT size_t tt_score_topk_redo_flags_offset(int B, int64_t N, int d, int k)
{
    if (B <= 0 || N <= 0 || k <= 0)
        return (size_t)-1;
    const Plan pl = make_plan(B, N, k, d);
    return (pl.paced && pl.main.tail_blocks > 0) ? pl.redo_off : (size_t)-1;
}

TT_EXPORT size_t tt_score_topk_workspace_bytes(int B, int64_t N, int d, int k)
{
    if (B <= 0 || N < 0 || k <= 0)
        return 0;
    return make_plan(B, N, k, d).ws_bytes;
}

TT_EXPORT size_t tt_score_topk_bf16_workspace_bytes(int B, int64_t N, int d, int k)
{
    if (B <= 0 || N < 0 || k <= 0)
        return 0;
    return make_plan(B, N, k, d, true).ws_bytes;
}

TT_EXPORT int tt_score_topk_partials_f32(const float *Q, int B, int d, const float *D, int64_t N, int k,
                                         int64_t idx_offset, void *workspace, size_t workspace_bytes,
                                         const float **part_val, const int64_t **part_idx, int *part_m,
                                         void *const *prof_events, tt_stream_t stream)
{
    Plan pl;
    int rc = score_partials(Q, B, d, D, false, N, k, idx_offset, workspace, workspace_bytes, (hipStream_t)stream, &pl,
                            "tt_score_topk_partials_f32", nullptr, prof_events);
    if (rc != TT_OK)
        return rc;
    if (part_val)
        *part_val = (const float *)((const char *)workspace + pl.pval_off);
    if (part_idx)
        *part_idx = (const int64_t *)((const char *)workspace + pl.pidx_off);
    if (part_m)
        *part_m = pl.main.n_chunks * k;
    return TT_OK;
}

namespace {
// flags[t] = 1 when a query of 32-query tile t came out of the merge with the give-up marker in its first place
__global__ __launch_bounds__(64) void redo_flag_kernel(const int64_t *__restrict__ out_idx, int B, int k, int *__restrict__ flags)
{
    const int q = blockIdx.x * 32 + threadIdx.x;
    const bool bad = threadIdx.x < 32 && q < B && out_idx[(size_t)q * k] >= (int64_t)TT_TOPK_INVALID_INDEX;
    const unsigned long long any = __ballot(bad);
    if (threadIdx.x == 0)
        flags[blockIdx.x] = any != 0ull;
}
} // namespace

// Exact path over fp32 (bf16 = false) or bf16 rows, optionally predicated on a device flag (the screened path's fallback).
namespace {
int score_topk_pred(const float *Q, int B, int d, const void *D, bool bf16, int64_t N, int k, int64_t idx_offset,
                    float *out_val, int64_t *out_idx, void *workspace, size_t workspace_bytes, const int *run_if,
                    hipStream_t st, const char *who, const unsigned *keep = nullptr)
{
    if (B < 0 || N < 0 || k <= 0)
        return tt_fail(TT_ERR_BAD_SHAPE, "%s: B=%d N=%lld k=%d", who, B, (long long)N, k);
    if (B == 0)
        return TT_OK;
    if (!score_dim_ok(d, bf16))
        return tt_fail(TT_ERR_UNSUPPORTED, "%s: d=%d (supported: %s)", who, d, score_dims(bf16));
    if (k > 64)
        return tt_fail(TT_ERR_UNSUPPORTED, "%s: k=%d > 64", who, k);
    if (!out_val || !out_idx)
        return tt_fail(TT_ERR_BAD_SHAPE, "%s: null output pointer", who);
    if (N == 0) { // merge over zero candidates writes the (-inf,-1) tail
        hipLaunchKernelGGL(topk_merge_kernel, dim3(B), dim3(MERGE_THREADS), 0, st, (const float *)nullptr,
                           (const int64_t *)nullptr, 0, k, out_val, out_idx, (const int *)nullptr, 1, (size_t)0);
        TT_LAUNCH_CHECK();
        return TT_OK;
    }
    Plan pl;
    int rc = score_partials(Q, B, d, D, bf16, N, k, idx_offset, workspace, workspace_bytes, st, &pl, who, run_if, nullptr, 0, keep);
    if (rc != TT_OK)
        return rc;
    const char *ws = (const char *)workspace;
    hipLaunchKernelGGL(topk_merge_kernel, dim3(B), dim3(MERGE_THREADS), 0, st, (const float *)(ws + pl.pval_off),
                       (const int64_t *)(ws + pl.pidx_off), pl.main.n_chunks * k, k, out_val, out_idx, run_if,
                       pl.main.n_chunks * k, (size_t)0);
    TT_LAUNCH_CHECK();
    if (!run_if && pl.paced && pl.main.tail_blocks > 0 && tt_score_pacing()) {
        // The one wait of this path that cannot be skipped without losing documents is a wave's wait for a chunk-mate's pool
        // draw; a wave whose budget ran out marked its lists (+inf, TT_TOPK_INVALID_INDEX + t).  Nothing downstream reads that
        // marker, so it is dealt with HERE, on the device: the query tiles whose merged list starts with it are done again on
        // the static split (the predicated form: no pool, no pacing, nobody to wait for) -- three small launches that find
        // nothing to do in every run observed so far (~10 us behind a search of >= 4 ms).
        // (only paced plans get here, and make_plan paces 32-query tiles only: one flag per 32 queries)
        int *redo = (int *)((char *)workspace + pl.redo_off);
        hipLaunchKernelGGL(redo_flag_kernel, dim3(pl.main.n_qtiles), dim3(64), 0, st, (const int64_t *)out_idx, B, k, redo);
        TT_LAUNCH_CHECK();
        return score_topk_pred(Q, B, d, D, bf16, N, k, idx_offset, out_val, out_idx, workspace, workspace_bytes, redo, st,
                               who, keep);
    }
    return TT_OK;
}
} // namespace

// The predicated forms, for the screened path's fallback (csrc/screen.hip).
int tt_score_topk_f32_pred(const float *Q, int B, int d, const float *D, int64_t N, int k, int64_t idx_offset,
                           float *out_val, int64_t *out_idx, void *workspace, size_t workspace_bytes,
                           const int *run_if, hipStream_t st)
{
    return score_topk_pred(Q, B, d, D, false, N, k, idx_offset, out_val, out_idx, workspace, workspace_bytes, run_if, st,
                           "tt_score_topk_f32");
}

int tt_score_topk_bf16_pred(const float *Q, int B, int d, const void *D, int64_t N, int k, int64_t idx_offset,
                            float *out_val, int64_t *out_idx, void *workspace, size_t workspace_bytes,
                            const int *run_if, hipStream_t st)
{
    return score_topk_pred(Q, B, d, D, true, N, k, idx_offset, out_val, out_idx, workspace, workspace_bytes, run_if, st,
                           "tt_score_topk_bf16");
}

TT_EXPORT int tt_score_topk_f32(const float *Q, int B, int d, const float *D, int64_t N, int k,
                                int64_t idx_offset, float *out_val, int64_t *out_idx, void *workspace,
                                size_t workspace_bytes, tt_stream_t stream)
{
    return tt_score_topk_f32_pred(Q, B, d, D, N, k, idx_offset, out_val, out_idx, workspace, workspace_bytes, nullptr,
                                  (hipStream_t)stream);
}

TT_EXPORT int tt_score_topk_bf16(const float *Q, int B, int d, const void *D_bf16, int64_t N, int k,
                                 int64_t idx_offset, float *out_val, int64_t *out_idx, void *workspace,
                                 size_t workspace_bytes, tt_stream_t stream)
{
    return tt_score_topk_bf16_pred(Q, B, d, D_bf16, N, k, idx_offset, out_val, out_idx, workspace, workspace_bytes,
                                   nullptr, (hipStream_t)stream);
}

// k-th largest of each row of vals [B][M] -> out [B] (internal: threshold seeding of both search paths)
int tt_kth_largest(const float *vals, int B, int M, int k, float *out, hipStream_t st)
{
    hipLaunchKernelGGL(kth_largest_kernel, dim3(B), dim3(256), 0, st, vals, M, k, out, (const int *)nullptr, (float *)nullptr);
    TT_LAUNCH_CHECK();
    return TT_OK;
}

// the k largest of each row of vals [B][M] -> list [B][k], unordered (-inf padding when M < k)
int tt_k_largest_list(const float *vals, int B, int M, int k, float *list, hipStream_t st)
{
    hipLaunchKernelGGL(kth_largest_kernel, dim3(B), dim3(256), 0, st, vals, M, k, (float *)nullptr, (const int *)nullptr, list);
    TT_LAUNCH_CHECK();
    return TT_OK;
}

namespace {
// Union seed of a row-sharded search: lists [world][B][ks] (every shard's ks largest sample maxima per query, as the
// all-gather left them) -> seed[q] = the kth-th largest of the world * ks values of query q.  Those are approximate scores
// of world * ks DISTINCT documents (one per 32-document sample tile, the shards' rows are disjoint), so kth documents of the
// whole corpus score at least seed[q]: a valid lower bound of the global kth-th best approximate score, and a much
// tighter one than any single shard's kth-th sample maximum.  (ks < kth on wide jobs: 16 ranks x k = 64 would be 1024 values;
// every rank then lists its 32 largest and the 64th of the 512 is taken -- still 64 distinct documents above the seed.)
// One wave per query, rank by counting (world * ks <= 512).
__global__ __launch_bounds__(64) void seed_union_kernel(const float *__restrict__ lists, int world, int B, int ks, int kth,
                                                        float *__restrict__ seed)
{
    const int q = blockIdx.x, lane = threadIdx.x;
    const int M = world * ks;
    __shared__ float v[512];
    for (int i = lane; i < M; i += 64)
        v[i] = lists[((size_t)(i / ks) * B + q) * ks + (i % ks)];
    __syncthreads();
    for (int i = lane; i < M; i += 64) {
        const float x = v[i];
        int before = 0; // entries ranking before entry i in (value desc, position asc) order
        for (int j = 0; j < M; ++j)
            before += (v[j] > x) || (v[j] == x && j < i);
        if (before == kth - 1)
            seed[q] = x; // exactly one entry has this rank (NaNs do not occur: the lists hold MFMA sums of finite inputs)
    }
}
} // namespace

TT_EXPORT int tt_seed_union_f32(const float *lists, int world, int B, int list_len, int kth, float *seed, tt_stream_t stream)
{
    if (!lists || !seed || world < 1 || B <= 0 || list_len < 1 || (int64_t)world * list_len > 512 || kth < 1 ||
        kth > world * list_len)
        return tt_fail(TT_ERR_BAD_SHAPE, "tt_seed_union_f32: world=%d B=%d list_len=%d kth=%d (kth <= world * list_len <= 512)",
                       world, B, list_len, kth);
    hipLaunchKernelGGL(seed_union_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, lists, world, B, list_len, kth, seed);
    TT_LAUNCH_CHECK();
    return TT_OK;
}

TT_EXPORT int tt_topk_merge(const float *in_val, const int64_t *in_idx, int B, int M, int k, float *out_val,
                            int64_t *out_idx, tt_stream_t stream)
{
    if (B < 0 || M < 0 || k <= 0)
        return tt_fail(TT_ERR_BAD_SHAPE, "tt_topk_merge: B=%d M=%d k=%d", B, M, k);
    if (k > MERGE_KMAX)
        return tt_fail(TT_ERR_UNSUPPORTED, "tt_topk_merge: k=%d > %d", k, MERGE_KMAX);
    if (B == 0)
        return TT_OK;
    hipLaunchKernelGGL(topk_merge_kernel, dim3(B), dim3(MERGE_THREADS), 0, (hipStream_t)stream, in_val, in_idx, M,
                       k, out_val, out_idx, (const int *)nullptr, M > 0 ? M : 1, (size_t)0);
    TT_LAUNCH_CHECK();
    return TT_OK;
}

TT_EXPORT int tt_topk_merge_shards(const void *gathered, int world, size_t rank_stride, size_t idx_byte_offset, int B,
                                   int kp, int k, float *out_val, int64_t *out_idx, tt_stream_t stream)
{
    if (B < 0 || world <= 0 || kp <= 0 || k <= 0)
        return tt_fail(TT_ERR_BAD_SHAPE, "tt_topk_merge_shards: world=%d B=%d kp=%d k=%d", world, B, kp, k);
    if (k > MERGE_KMAX)
        return tt_fail(TT_ERR_UNSUPPORTED, "tt_topk_merge_shards: k=%d > %d", k, MERGE_KMAX);
    if ((int64_t)world * kp > INT_MAX)
        return tt_fail(TT_ERR_UNSUPPORTED, "tt_topk_merge_shards: world*kp too large");
    if (!gathered || !out_val || !out_idx || ((uintptr_t)gathered & 7) || (rank_stride & 7) || (idx_byte_offset & 7) ||
        idx_byte_offset < (size_t)B * kp * sizeof(float) || rank_stride < idx_byte_offset + (size_t)B * kp * sizeof(int64_t))
        return tt_fail(TT_ERR_BAD_SHAPE, "tt_topk_merge_shards: layout (stride %zu, idx offset %zu) does not hold [B,kp] f32 + i64, 8-byte aligned",
                       rank_stride, idx_byte_offset);
    if (B == 0)
        return TT_OK;
    hipLaunchKernelGGL(topk_merge_kernel, dim3(B), dim3(MERGE_THREADS), 0, (hipStream_t)stream, (const float *)gathered,
                       (const int64_t *)((const char *)gathered + idx_byte_offset), world * kp, k, out_val, out_idx,
                       (const int *)nullptr, kp, rank_stride);
    TT_LAUNCH_CHECK();
    return TT_OK;
}

TT_EXPORT int tt_score_all_f32(const float *Q, int B, int d, const float *D, int64_t N, float *S, tt_stream_t stream)
{
    if (B < 0 || N <= 0 || d <= 0 || (d & 3))
        return tt_fail(TT_ERR_BAD_SHAPE, "tt_score_all_f32: B=%d N=%lld d=%d", B, (long long)N, d);
    if (N >= INT_MAX || d > 512 || B > 65535)
        return tt_fail(TT_ERR_UNSUPPORTED, "tt_score_all_f32: N, d (<= 512) or B (<= 65535) too large");
    if (B == 0)
        return TT_OK;
    if (!Q || !D || !S)
        return tt_fail(TT_ERR_BAD_SHAPE, "tt_score_all_f32: null pointer");
    hipLaunchKernelGGL(score_all_kernel, dim3((unsigned)((N + 255) / 256), B), dim3(256), 0, (hipStream_t)stream, Q, D, (int)N, d, S);
    TT_LAUNCH_CHECK();
    return TT_OK;
}

TT_EXPORT int tt_score_rank_f32(const float *Q, int B, int d, const float *D, int64_t N, const int64_t *target,
                                int64_t *rank, tt_stream_t stream)
{
    if (B < 0 || N <= 0 || d <= 0 || (d & 3))
        return tt_fail(TT_ERR_BAD_SHAPE, "tt_score_rank_f32: B=%d N=%lld d=%d", B, (long long)N, d);
    if (N >= INT_MAX)
        return tt_fail(TT_ERR_UNSUPPORTED, "tt_score_rank_f32: N too large");
    if (d > 512)
        return tt_fail(TT_ERR_UNSUPPORTED, "tt_score_rank_f32: d=%d > 512", d);
    if (B == 0)
        return TT_OK;
    hipLaunchKernelGGL(score_rank_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, Q, D, (int)N, d, target, rank);
    TT_LAUNCH_CHECK();
    return TT_OK;
}

// ===========================================================================
// K4L: exact top-k for 64 < k <= TT_TOPK_LARGE_KMAX (DESIGN.md "Large k").
//
// Tier 0  the main pass above, unchanged, with per-(wave, query) lists of m = 64 (seeded with the k-th -- not the 64th --
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

// Workspace of a large-k search: the k = 64 plan's, then the large-k state.
struct LargePlan {
    Plan pl;
    bool small; // k <= 64: the call is tt_score_topk_f32 / _bf16's own
    size_t tier_off, st_off, buf_off, hist_off, ws_bytes;
};

LargePlan make_large_plan(int B, int64_t N, int d, int k, bool bf16)
{
    LargePlan lp;
    lp.small = k <= LK_M;
    lp.pl = make_plan(B, N, lp.small ? k : LK_M, d, bf16);
    TTWorkspace ws;
    ws.off = tt_align_up(lp.pl.ws_bytes, 256);
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

int score_topk_large(const float *Q, int B, int d, const void *D, bool bf16, int64_t N, int k, int64_t idx_offset,
                     float *out_val, int64_t *out_idx, void *workspace, size_t workspace_bytes, hipStream_t st, const char *who,
                     const unsigned *keep = nullptr)
{
    if (B < 0 || N < 0 || k <= 0)
        return tt_fail(TT_ERR_BAD_SHAPE, "%s: B=%d N=%lld k=%d", who, B, (long long)N, k);
    if (!score_dim_ok(d, bf16))
        return tt_fail(TT_ERR_UNSUPPORTED, "%s: d=%d (supported: %s)", who, d, score_dims(bf16));
    if (k > TT_TOPK_LARGE_KMAX)
        return tt_fail(TT_ERR_UNSUPPORTED, "%s: k=%d > %d", who, k, TT_TOPK_LARGE_KMAX);
    if (N >= (int64_t)INT_MAX - 64)
        return tt_fail(TT_ERR_UNSUPPORTED, "%s: N=%lld >= 2^31-64; shard the corpus", who, (long long)N);
    if ((uintptr_t)keep & 3)
        return tt_fail(TT_ERR_BAD_SHAPE, "%s: keep must be 4-byte aligned", who);
    if (B == 0)
        return TT_OK;
    if (!Q || !D || !out_val || !out_idx)
        return tt_fail(TT_ERR_BAD_SHAPE, "%s: null pointer", who);
    const LargePlan lp = make_large_plan(B, N, d, k, bf16);
    if (!workspace || workspace_bytes < lp.ws_bytes)
        return tt_fail(TT_ERR_WORKSPACE, "%s: workspace %zu < %zu bytes", who, workspace_bytes, lp.ws_bytes);
    if (((uintptr_t)D & 15) || ((uintptr_t)Q & 3) || ((uintptr_t)workspace & 255))
        return tt_fail(TT_ERR_BAD_SHAPE, "%s: D must be 16-byte and the workspace 256-byte aligned", who);
    char *ws = (char *)workspace;
    int *tier = (int *)(ws + lp.tier_off);
    TT_RC_CHECK(tt_zero_async(tier, (size_t)B * sizeof(int), st));
    if (lp.small)
        return score_topk_pred(Q, B, d, D, bf16, N, k, idx_offset, out_val, out_idx, workspace, workspace_bytes, nullptr, st, who,
                               keep);
    if (N == 0) {
        SegSource src{nullptr, nullptr, 0, 1, 0};
        hipLaunchKernelGGL(lk_merge_kernel, dim3(B), dim3(LSEL_THREADS), 0, st, src, k, out_val, out_idx);
        TT_LAUNCH_CHECK();
        return TT_OK;
    }
    // tier 0: the k = 64 main pass, seeded with the k-th largest sample maximum
    Plan pl;
    TT_RC_CHECK(score_partials(Q, B, d, D, bf16, N, LK_M, idx_offset, workspace, workspace_bytes, st, &pl, who, nullptr,
                               nullptr, k, keep));
    const float *pval = (const float *)(ws + pl.pval_off);
    const int64_t *pidx = (const int64_t *)(ws + pl.pidx_off);
    const int M = pl.main.n_chunks * LK_M;
    if (pl.paced && pl.main.tail_blocks > 0 && tt_score_pacing()) {
        // the give-up redo of tt_score_topk_f32, on the lists themselves: a marker must never reach t_q
        int *redo = (int *)(ws + pl.redo_off);
        hipLaunchKernelGGL(lk_marker_kernel, dim3(pl.main.n_qtiles), dim3(256), 0, st, pidx, B, pl.main.n_chunks, redo);
        TT_LAUNCH_CHECK();
        TT_RC_CHECK(score_partials(Q, B, d, D, bf16, N, LK_M, idx_offset, workspace, workspace_bytes, st, &pl, who, redo, nullptr,
                                   0, keep));
    }
    LkState *sts = (LkState *)(ws + lp.st_off);
    Cand *buf = (Cand *)(ws + lp.buf_off);
    int *hist = (int *)(ws + lp.hist_off);
    hipLaunchKernelGGL(lk_analyze_kernel, dim3(B), dim3(LSEL_THREADS), 0, st, pval, pidx, pl.main.n_chunks, k,
                       pl.prepass ? (const float *)(ws + pl.pre_val_off) : (const float *)nullptr, sts, tier);
    TT_LAUNCH_CHECK();
    TT_RC_CHECK(tt_zero_async(hist, (size_t)B * LK_BINS * sizeof(int), st));
    // tiers 1 and 2: a fixed chain of (scan, decide) launches, each a no-op for the queries that are done
    const int n_dt = (int)((N + LK_SCAN_DOCS - 1) / LK_SCAN_DOCS);
    const int grid = n_dt < LK_SCAN_BLOCKS ? n_dt : LK_SCAN_BLOCKS;
    for (int r = 0; r < LK_ROUNDS; ++r) {
        if (keep && bf16)
            hipLaunchKernelGGL((lk_scan_kernel<true, true>), dim3(grid), dim3(256), 0, st, Q, D, B, d, (int)N, sts, buf, hist, keep);
        else if (keep)
            hipLaunchKernelGGL((lk_scan_kernel<false, true>), dim3(grid), dim3(256), 0, st, Q, D, B, d, (int)N, sts, buf, hist, keep);
        else if (bf16)
            hipLaunchKernelGGL((lk_scan_kernel<true, false>), dim3(grid), dim3(256), 0, st, Q, D, B, d, (int)N, sts, buf, hist, keep);
        else
            hipLaunchKernelGGL((lk_scan_kernel<false, false>), dim3(grid), dim3(256), 0, st, Q, D, B, d, (int)N, sts, buf, hist, keep);
        TT_LAUNCH_CHECK();
        hipLaunchKernelGGL(lk_decide_kernel, dim3(B), dim3(256), 0, st, sts, tier, hist, k);
        TT_LAUNCH_CHECK();
    }
    SearchSource src{pval, pidx, M, buf, sts, tier, idx_offset};
    hipLaunchKernelGGL(lk_final_kernel, dim3(B), dim3(LSEL_THREADS), 0, st, src, k, out_val, out_idx);
    TT_LAUNCH_CHECK();
    return TT_OK;
}
} // namespace

TT_EXPORT size_t tt_score_topk_large_workspace_bytes(int B, int64_t N, int d, int k, int bf16)
{
    if (B <= 0 || N < 0 || k <= 0 || k > TT_TOPK_LARGE_KMAX)
        return 0;
    return make_large_plan(B, N, d, k, bf16 != 0).ws_bytes;
}

TT_EXPORT size_t tt_score_topk_large_tier_offset(int B, int64_t N, int d, int k, int bf16)
{
    if (B <= 0 || N < 0 || k <= 0 || k > TT_TOPK_LARGE_KMAX)
        return (size_t)-1;
    return make_large_plan(B, N, d, k, bf16 != 0).tier_off;
}

TT_EXPORT int tt_score_topk_large_f32(const float *Q, int B, int d, const float *D, int64_t N, int k, int64_t idx_offset,
                                      float *out_val, int64_t *out_idx, void *workspace, size_t workspace_bytes,
                                      tt_stream_t stream)
{
    return score_topk_large(Q, B, d, D, false, N, k, idx_offset, out_val, out_idx, workspace, workspace_bytes,
                            (hipStream_t)stream, "tt_score_topk_large_f32");
}

TT_EXPORT int tt_score_topk_large_bf16(const float *Q, int B, int d, const void *D_bf16, int64_t N, int k, int64_t idx_offset,
                                       float *out_val, int64_t *out_idx, void *workspace, size_t workspace_bytes,
                                       tt_stream_t stream)
{
    return score_topk_large(Q, B, d, D_bf16, true, N, k, idx_offset, out_val, out_idx, workspace, workspace_bytes,
                            (hipStream_t)stream, "tt_score_topk_large_bf16");
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
    return score_topk_large(Q, B, d, D, false, N, k, idx_offset, out_val, out_idx, workspace, workspace_bytes,
                            (hipStream_t)stream, "tt_score_topk_masked_f32", keep);
}

TT_EXPORT int tt_score_topk_masked_bf16(const float *Q, int B, int d, const void *D_bf16, int64_t N, const uint32_t *keep, int k,
                                        int64_t idx_offset, float *out_val, int64_t *out_idx, void *workspace,
                                        size_t workspace_bytes, tt_stream_t stream)
{
    return score_topk_large(Q, B, d, D_bf16, true, N, k, idx_offset, out_val, out_idx, workspace, workspace_bytes,
                            (hipStream_t)stream, "tt_score_topk_masked_bf16", keep);
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
    if ((int64_t)world * kp > INT_MAX)
        return tt_fail(TT_ERR_UNSUPPORTED, "tt_topk_merge_shards_large: world*kp too large");
    if (!gathered || !out_val || !out_idx || ((uintptr_t)gathered & 7) || (rank_stride & 7) || (idx_byte_offset & 7) ||
        idx_byte_offset < (size_t)B * kp * sizeof(float) || rank_stride < idx_byte_offset + (size_t)B * kp * sizeof(int64_t))
        return tt_fail(TT_ERR_BAD_SHAPE, "tt_topk_merge_shards_large: layout (stride %zu, idx offset %zu) does not hold [B,kp] f32 + i64, 8-byte aligned",
                       rank_stride, idx_byte_offset);
    if (B == 0)
        return TT_OK;
    SegSource src{(const float *)gathered, (const int64_t *)((const char *)gathered + idx_byte_offset), world * kp, kp,
                  rank_stride};
    hipLaunchKernelGGL(lk_merge_kernel, dim3(B), dim3(LSEL_THREADS), 0, (hipStream_t)stream, src, k, out_val, out_idx);
    TT_LAUNCH_CHECK();
    return TT_OK;
}
