// Shared host/device helpers for libtt.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/tt.h"

#define TT_EXPORT extern "C" __attribute__((visibility("default")))

int tt_fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));

#define TT_HIP_CHECK(expr)                                                                   \
    do {                                                                                     \
        hipError_t e_ = (expr);                                                              \
        if (e_ != hipSuccess)                                                                \
            return tt_fail(TT_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), \
                           __FILE__, __LINE__);                                              \
    } while (0)

#define TT_LAUNCH_CHECK() TT_HIP_CHECK(hipGetLastError())

#define TT_RC_CHECK(expr)       \
    do {                        \
        const int rc_ = (expr); \
        if (rc_ != TT_OK)       \
            return rc_;         \
    } while (0)

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

static inline size_t tt_align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// Compute units of the current device; 256 (MI355X) when the query fails, so that workspace-size queries work without a device.
int tt_device_cus();

// Host-side planning pieces shared by the search planners (score_topk.hip with score_topk_large.hip, screen.hip); each planner keeps its own policy.
// n_tiles tiles in chunks of whole tiles: about `want` chunks, at most max_chunks, at least one (one empty chunk for no tiles).
struct TTChunks {
    int tiles_per_chunk, n_chunks;
};
static inline TTChunks tt_chunks(int n_tiles, int want, int max_chunks)
{
    if (n_tiles <= 0)
        return {1, 1};
    want = want > max_chunks ? max_chunks : want;
    want = want > n_tiles ? n_tiles : want;
    want = want < 1 ? 1 : want;
    const int per = (n_tiles + want - 1) / want;
    return {per, (n_tiles + per - 1) / per};
}

// Tail pool of a chunked pass: the last 1/div of every chunk's share (div <= 0: none) is drawn from a shared pool in blocks of
// a quarter of that share, clamped to [g_lo, g_hi] tiles; only when the share is at least min_share tiles.  A chunk keeps
// `own` tiles; tiles [0, static_tiles) are cut statically, the rest are tail_blocks blocks of tail_g tiles.
struct TTTailSplit {
    int own, static_tiles, tail_g, tail_blocks;
};
static inline TTTailSplit tt_tail_split(int tiles_per_chunk, int n_chunks, int n_tiles, int div, int min_share, int g_lo,
                                        int g_hi)
{
    const int share = div > 0 ? tiles_per_chunk / div : 0;
    if (share < min_share)
        return {tiles_per_chunk, n_tiles, 1, 0};
    const int own = tiles_per_chunk - share;
    int g = share / 4;
    g = g < g_lo ? g_lo : (g > g_hi ? g_hi : g);
    const int static_tiles = (int64_t)own * n_chunks < n_tiles ? own * n_chunks : n_tiles;
    return {own, static_tiles, g, (n_tiles - static_tiles + g - 1) / g};
}

// Workspace layout: take(bytes) returns the next buffer's offset and moves on by bytes rounded up to 256.
struct TTWorkspace {
    size_t off = 0;
    size_t take(size_t bytes)
    {
        const size_t at = off;
        off = tt_align_up(off + bytes, 256);
        return at;
    }
};

// Zero `bytes` bytes (multiple of 4, 4-byte aligned) at p with a KERNEL.  Never hipMemsetAsync on a path a caller may
// capture into a HIP graph: on ROCm 7.2 a captured memset node of a larger graph fills with garbage from the second
// replay on (a repeating 16-byte pattern that looks like two kernel-argument pointers: the node's pattern staging is
// recycled) -- observed in torch.cuda.graph captures of the encoder forward and of a screened search
// (tools/experiments/encoder_graph_flags.py; small stand-alone graphs do not show it: memset_graph.hip).
int tt_zero_async(void *p, size_t bytes, hipStream_t st);
int tt_zero3_async(void *p0, size_t b0, void *p1, size_t b1, void *p2, size_t b2, hipStream_t st);

// MUTATION SWITCH, never set in the product build (tools/mutation_guard.py builds the variants): a bit mask of f16-split
// kernels whose `lo` products (hi*lo and lo*hi) are compiled out, which turns "fp32-grade" into plain fp16 (2^-11 per
// product).  The parity tests' tolerances must be tight enough to FAIL on every one of them.
//   1 = K2 gru_seq16 (forward recurrence)   2 = K7 gru_bwd16 (backward recurrence)
//   4 = K1 gemm_rows16 (input projection)   8 = sgemm16 (input gradients, tiled K1, tiled weight gradients)
//  16 = wgrad16 (the weight gradients dW_ih / dW_hh of the training step)
#ifndef TT_MUTATE_DROP_LO
#define TT_MUTATE_DROP_LO 0
#endif

// A/B SWITCHES.  The product library reads NO environment variable on any call path: every switch below is the compile-time
// constant `dflt` there.  A comparison build (-DTT_AB: tools/build_variant.py ab -> ab/libtt_ab.so, loaded by the tests that
// pin a product kernel against the kernel it replaced, and by tools/experiments) reads the variable of the same name at EVERY
// call, so that one process can run both forms; the superseded kernels themselves are compiled only into that build.
#ifdef TT_AB
#include <stdlib.h>
static inline int tt_ab_env(const char *name, int dflt)
{
    const char *e = getenv(name);
    return e ? atoi(e) : dflt;
}
#define TT_AB_SWITCH(name, dflt) tt_ab_env(#name, (dflt))
#else
#define TT_AB_SWITCH(name, dflt) (dflt)
#endif

#define TT_WAVE 64

// The order-preserving integer image of a float (radix selections: score_topk.hip, score_topk_large.hip) and its inverse.
static __device__ __forceinline__ unsigned order_key(float f)
{
    const unsigned b = __float_as_uint(f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

static __device__ __forceinline__ float order_key_to_float(unsigned key)
{
    return __uint_as_float((key & 0x80000000u) ? (key & 0x7fffffffu) : ~key);
}

// The order of every top-k list: score descending, index ascending.
static __device__ __forceinline__ bool ranks_before(float sa, int64_t ia, float sb, int64_t ib)
{
    return sa > sb || (sa == sb && ia < ib);
}
