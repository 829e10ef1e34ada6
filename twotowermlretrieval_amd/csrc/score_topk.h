// Host side of the exact search (K4, score_topk.hip) as its other translation units see it: score_topk_large.hip (K4L / K4m)
// builds on the main pass, screen.hip falls back to the predicated search and borrows the threshold selections.
// Host declarations only: every kernel lives in exactly one .hip file.
#pragma once
#include "tt_common.h"

constexpr int MERGE_KMAX = 64; // k of topk_merge_kernel, and with it of every k <= 64 entry point and of the main pass's lists

namespace { // (internal like every type a kernel of these files takes: the kernels' names carry the namespace)
// One candidate: (score, document index relative to D).  8 bytes, one store.
struct __attribute__((aligned(8))) Cand {
    float v;
    int x;
};
} // namespace

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

// k: the length of the per-(wave, query) lists.  bf16: bf16 document rows, which run on 32-query tiles at every batch size; for
// B > 16 the workspace layout is the fp32 one (only the pacing block length, a kernel argument, depends on the row bytes)
Plan make_plan(int B, int64_t N, int k, int d, bool bf16);

// One exact search as a public entry point received it.
struct ExactCall {
    const float *Q;
    int B, d;
    const void *D; // [N][d] fp32 rows, or bf16 rows when bf16 is set
    bool bf16;
    int64_t N;
    int k;
    int64_t idx_offset;
    const unsigned *keep; // keep-bitmask (K4m), or nullptr
    float *out_val;
    int64_t *out_idx;
    void *workspace;
    size_t workspace_bytes;
    hipStream_t stream;
    const char *who;       // the entry point's name, for messages
    bool partials = false; // tt_score_topk_partials_f32: the caller takes the lists, so there are no outputs and no empty call
    // tagged search (tt_score_topk_tagged_f32 / _bf16): one tag per document, padded to whole 32-document tiles, and one
    // (mask, value) pair per query; all three set, or all three nullptr
    const unsigned *tags = nullptr;
    const unsigned *match_mask = nullptr;
    const unsigned *match_value = nullptr;
    // biased search (tt_score_topk_biased_f32 / _bf16): one float per document, padded to whole 32-document tiles, or nullptr
    const float *bias = nullptr;
    // cursor search (tt_score_topk_after_f32 / _bf16): one (score, GLOBAL id) cursor per query; both set, or both nullptr
    const float *after_val = nullptr;
    const int64_t *after_idx = nullptr;
};

// What varies between the main passes of one call.  (The sample pass always seeds for the call's k.)
struct ExactPass {
    int list_k;               // entries per (wave, query) list: the call's k, or 64 under a large k
    const int *run_if;        // device flag per 32-query tile (tile t runs while run_if[t] != 0: static split, no sample pass), or nullptr
    void *const *prof_events; // two events recorded around the main launch, or nullptr
};

// The argument checks of every public exact search, once per call; what lies below trusts them.  kmax: the entry's k cap
// (MERGE_KMAX, or TT_TOPK_LARGE_KMAX for the large and masked entries).  TT_OK with c.B == 0, or c.N == 0 under
// kmax == MERGE_KMAX: nothing to score and *pl is not set; TT_OK otherwise: *pl is the plan of the main pass, lists of min(k, 64).
int exact_validate(const ExactCall &c, int kmax, Plan *pl);

// Sample pass (when the plan has one and the pass is not predicated) and main pass: partial lists at pl.pval_off / pl.pidx_off.
int score_partials(const ExactCall &c, const Plan &pl, const ExactPass &ps);

// A validated k <= 64 search: lists, merge, give-up redo.  run_if: the predicated form (the screened path's fallback).
int score_topk_pred(const ExactCall &c, const Plan &pl, const int *run_if);

// The give-up redo.  The one wait of the main pass that cannot be skipped without losing documents is a wave's wait for a
// chunk-mate's pool draw; a wave whose budget ran out marked its lists (+inf, TT_TOPK_INVALID_INDEX + t).  Nothing downstream
// reads that marker, so it is dealt with on the device: `flag` raises pl.redo_off's flag of every 32-query tile that carries
// one, and those tiles are scored again on the static split (the predicated form: no pool, no pacing, nobody to wait for),
// then merged again when `merge` is set -- small launches that find nothing to do in every run observed so far (~10 us behind
// a search of >= 4 ms).  A no-op for plans whose waves never wait for a draw.
// (only paced plans draw in step, and make_plan paces 32-query tiles only: one flag per 32 queries)
typedef int (*FlagGaveUp)(const ExactCall &c, const Plan &pl, int *flags);
int redo_gave_up(const ExactCall &c, const Plan &pl, int list_k, FlagGaveUp flag, bool merge);

// score_topk_large.hip: the workspace of a large or masked call whose main pass runs under pl.
size_t score_topk_large_ws_bytes(const Plan &pl, int B, int k);

// A whole k <= 64 search, checks included: both public entries, and under run_if (one device flag per 32-query tile, see
// ExactPass) the screened path's fallback, which names the public entry it stands for in c.who (screen.hip).  The workspace
// is the unmasked search's (tt_score_topk_workspace_bytes / _bf16_workspace_bytes) with or without c.keep.
int exact_small(const ExactCall &c, const int *run_if);

// range.hip: count[b] (+)= the sum of part[b][0, n_chunks), the counting pass's per-(query, chunk) integers; n_chunks = 0 writes zeros
int tt_count_finish(const int64_t *part, int B, int n_chunks, int64_t *count, int accumulate, hipStream_t st);

// k-th largest of each row of vals [B][M] -> out [B] (threshold seeding of both search paths)
int tt_kth_largest(const float *vals, int B, int M, int k, float *out, hipStream_t st);
// the k largest of each row of vals [B][M] -> list [B][k], unordered (-inf padding when M < k)
int tt_k_largest_list(const float *vals, int B, int M, int k, float *list, hipStream_t st);

// One [world] x ([B,kp] f32 + [B,kp] i64) gather as tt_topk_merge_shards(_large) received it.
struct ShardsCall {
    const void *gathered;
    int world;
    size_t rank_stride, idx_byte_offset;
    int B, kp;
    const char *who;
};
// world * kp fits an int and every rank's block holds its two arrays, 8-byte aligned
int merge_shards_layout_ok(const ShardsCall &s, const float *out_val, const int64_t *out_idx);
