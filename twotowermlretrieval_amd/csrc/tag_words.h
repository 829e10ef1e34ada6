// The tags of one 32-document tile, as the TAGGED instantiations of the exact search kernels read them (score_topk.hip: tagged
// search, DESIGN.md "Tagged search").  Device code only.
#pragma once

// A tile's 32 tags are 128 contiguous bytes and wave-uniform, so they travel like the keep word (keep_word.h, which says why a
// compiler-visible vector load in the tile loop is out of the question): two 16-word scalar loads on the lgkmcnt side, issued
// under the tile's last slab of MFMAs and waited for in front of the epilogue.  They land in 32 SGPRs; a VALU instruction of
// gfx9 reads one SGPR, which is exactly what one document's test needs (tag_match_word).
typedef unsigned tag_u32x16 __attribute__((ext_vector_type(16)));

struct TagWords {
    tag_u32x16 lo, hi; // tags of documents 0..15 and 16..31 of the tile
};

// (first: the first A operand(s) of the MFMAs that follow, named so that their chain stays below the loads; the destinations
//  are early-clobber: the second load still needs the address pair)
template <class A>
__device__ __forceinline__ void tag_words_issue(const unsigned *tile_tags, TagWords &t, A &first)
{
    asm volatile("s_load_dwordx16 %[lo], %[tags], 0x0\n\ts_load_dwordx16 %[hi], %[tags], 0x40"
                 : [lo] "=&s"(t.lo), [hi] "=&s"(t.hi), "+v"(first)
                 : [tags] "s"(tile_tags)
                 : "memory");
}

// The wait names the destinations (tags and the keep word that was issued with them), so no consumer is scheduled above it,
// and the tile's accumulators, so that hipcc cannot hoist it above the MFMAs.  Scalar loads return out of order: lgkmcnt(0).
template <class Acc>
__device__ __forceinline__ void tag_words_wait(TagWords &t, unsigned &kw, Acc &acc)
{
    asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(t.lo), "+s"(t.hi), "+s"(kw), "+v"(acc) : : "memory");
}

// The eligibility word of ONE query over the tile: bit i set iff (tag[i] & match_mask) == match_value.  mm / mv are the
// lane's query's pair (VGPRs), every tag is an SGPR operand: per document one v_and (SGPR tag, VGPR mask), one v_cmp_eq against
// the VGPR value and the fold of the bit into the word.  Every lane forms the whole word of its query: the lanes that share a
// query (two in the 32-query kernel, four in the 16-query one) own different documents of the tile, but which of a tile's
// SGPRs a lane would need then depends on the lane, and selecting it costs what computing the other half does.
__device__ __forceinline__ unsigned tag_match_word(const TagWords &t, unsigned mm, unsigned mv)
{
    // Folded as w = 2 w + bit from document 31 down, not as 32 masks (1 << i) OR-ed together: hipcc parks the masks that are no
    // inline constants in VGPRs, which the d = 256 instantiations do not have.  What it emits for this form is, per two
    // documents, 2 v_and, 2 v_cmp_eq, 2 v_cndmask (0 / 1, 0 / 2), a v_or3 and a v_lshlrev: 4 vector instructions per document
    // (DESIGN.md "Tagged search" has the issue-slot accounting).
    unsigned w = 0u;
#pragma unroll
    for (int i = 15; i >= 0; --i)
        w = w + w + (((t.hi[i] & mm) == mv) ? 1u : 0u);
#pragma unroll
    for (int i = 15; i >= 0; --i)
        w = w + w + (((t.lo[i] & mm) == mv) ? 1u : 0u);
    return w;
}
