// The biases of one 32-document tile, as the BIASED instantiations of the exact search kernels read and apply them
// (score_topk.hip: biased search, DESIGN.md "Biased search").  Device code only.
#pragma once
#include "tag_words.h"

// A tile's 32 biases are 128 contiguous bytes and wave-uniform, like its 32 tags: they take the tags' route (tag_words.h, and
// keep_word.h for why a compiler-visible vector load in the tile loop is out of the question) -- two 16-word scalar loads on the
// lgkmcnt side, issued with the keep word's load under the tile's last slab of MFMAs and waited for in front of the epilogue.
// They land in 32 SGPRs as raw words.
struct BiasWords {
    TagWords w; // lo: documents 0..15 of the tile, hi: 16..31
};

template <class A>
__device__ __forceinline__ void bias_words_issue(const float *tile_bias, BiasWords &b, A &first)
{
    tag_words_issue((const unsigned *)tile_bias, b.w, first);
}

template <class Acc>
__device__ __forceinline__ void bias_words_wait(BiasWords &b, unsigned &kw, Acc &acc)
{
    tag_words_wait(b.w, kw, acc);
}

// word of tile row `row` (a compile-time constant at every use: the register is named, never indexed)
__device__ __forceinline__ unsigned bias_word(const BiasWords &b, int row)
{
    return row < 16 ? b.w.lo[row] : b.w.hi[row - 16];
}

// Which row an accumulator element belongs to depends on the lane -- its half in the 32-query kernel, its quarter in the
// 16-query one -- while the biases sit in SGPRs, which every lane sees alike.  The pick is made with the execution mask: one
// v_mov of the first candidate by all lanes, then one v_mov per further candidate by the lanes it belongs to.  A lane half or
// quarter is a fixed range of lanes (the kernels' h = lane >> 5, kq = lane >> 4), so the masks are constants ANDed with the
// mask the wave came with, which is put back at the end.  That is 2 v_mov (4 in the 16-query kernel) and the add per element.
// What hipcc makes of the same pick written in C++ is no alternative: as a select between two elements of one vector it
// becomes ONE extract at a lane-dependent index, lowered to a chain of 15 compares and v_cndmask per element; with the words
// made opaque one by one, a branch pair with saved and restored masks per element.
// out[i] = (lane >= 32) ? row0 + 4 + i : row0 + i, i < 4 -- the 32-query kernel's elements r = 4 g .. 4 g + 3 with row0 = 8 g
__device__ __forceinline__ void bias_pick_half(const BiasWords &b, int row0, float (&out)[4])
{
    unsigned save;
    asm("v_mov_b32 %[o0], %[a0]\n\tv_mov_b32 %[o1], %[a1]\n\tv_mov_b32 %[o2], %[a2]\n\tv_mov_b32 %[o3], %[a3]\n\t"
        "s_mov_b32 %[save], exec_lo\n\t"
        "s_mov_b32 exec_lo, 0\n\t"
        "v_mov_b32 %[o0], %[b0]\n\tv_mov_b32 %[o1], %[b1]\n\tv_mov_b32 %[o2], %[b2]\n\tv_mov_b32 %[o3], %[b3]\n\t"
        "s_mov_b32 exec_lo, %[save]"
        : [o0] "=&v"(out[0]), [o1] "=&v"(out[1]), [o2] "=&v"(out[2]), [o3] "=&v"(out[3]), [save] "=&s"(save)
        : [a0] "s"(bias_word(b, row0)), [a1] "s"(bias_word(b, row0 + 1)), [a2] "s"(bias_word(b, row0 + 2)),
          [a3] "s"(bias_word(b, row0 + 3)), [b0] "s"(bias_word(b, row0 + 4)), [b1] "s"(bias_word(b, row0 + 5)),
          [b2] "s"(bias_word(b, row0 + 6)), [b3] "s"(bias_word(b, row0 + 7)));
}

// out[i] = row0 + 4 (lane >> 4) + i, i < 4 -- the 16-query kernel's elements (u, 0..3) with row0 = 16 u
__device__ __forceinline__ void bias_pick_quarter(const BiasWords &b, int row0, float (&out)[4])
{
    unsigned lo, hi;
    asm("v_mov_b32 %[o0], %[a0]\n\tv_mov_b32 %[o1], %[a1]\n\tv_mov_b32 %[o2], %[a2]\n\tv_mov_b32 %[o3], %[a3]\n\t"
        "s_mov_b32 %[lo], exec_lo\n\t"
        "s_mov_b32 %[hi], exec_hi\n\t"
        "s_and_b32 exec_lo, %[lo], 0xffff0000\n\t" // lanes 16..31
        "s_mov_b32 exec_hi, 0\n\t"
        "v_mov_b32 %[o0], %[b0]\n\tv_mov_b32 %[o1], %[b1]\n\tv_mov_b32 %[o2], %[b2]\n\tv_mov_b32 %[o3], %[b3]\n\t"
        "s_mov_b32 exec_lo, 0\n\t" // lanes 32..63
        "s_mov_b32 exec_hi, %[hi]\n\t"
        "v_mov_b32 %[o0], %[c0]\n\tv_mov_b32 %[o1], %[c1]\n\tv_mov_b32 %[o2], %[c2]\n\tv_mov_b32 %[o3], %[c3]\n\t"
        "s_and_b32 exec_hi, %[hi], 0xffff0000\n\t" // lanes 48..63
        "v_mov_b32 %[o0], %[d0]\n\tv_mov_b32 %[o1], %[d1]\n\tv_mov_b32 %[o2], %[d2]\n\tv_mov_b32 %[o3], %[d3]\n\t"
        "s_mov_b32 exec_lo, %[lo]\n\t"
        "s_mov_b32 exec_hi, %[hi]"
        : [o0] "=&v"(out[0]), [o1] "=&v"(out[1]), [o2] "=&v"(out[2]), [o3] "=&v"(out[3]), [lo] "=&s"(lo), [hi] "=&s"(hi)
        : [a0] "s"(bias_word(b, row0)), [a1] "s"(bias_word(b, row0 + 1)), [a2] "s"(bias_word(b, row0 + 2)),
          [a3] "s"(bias_word(b, row0 + 3)), [b0] "s"(bias_word(b, row0 + 4)), [b1] "s"(bias_word(b, row0 + 5)),
          [b2] "s"(bias_word(b, row0 + 6)), [b3] "s"(bias_word(b, row0 + 7)), [c0] "s"(bias_word(b, row0 + 8)),
          [c1] "s"(bias_word(b, row0 + 9)), [c2] "s"(bias_word(b, row0 + 10)), [c3] "s"(bias_word(b, row0 + 11)),
          [d0] "s"(bias_word(b, row0 + 12)), [d1] "s"(bias_word(b, row0 + 13)), [d2] "s"(bias_word(b, row0 + 14)),
          [d3] "s"(bias_word(b, row0 + 15))
        : "scc");
}

// The biased score: fl32(s + bias), ONE fp32 add (round to nearest even) behind the finished multiply chain -- not a non-zero
// initial accumulator and not an fma, which round differently (and the former would make the score depend on the MFMA's
// internal order).
__device__ __forceinline__ float bias_add(float s, float bias)
{
    return s + bias;
}
