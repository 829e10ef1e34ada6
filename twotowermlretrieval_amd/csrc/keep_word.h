// The keep word of one 32-document tile, as the MASKED instantiations of the search kernels read it (score_topk.hip: K4m;
// screen.hip: the masked screen).  Device code only.
#pragma once

// The word is wave-uniform, so it travels as a scalar load on the lgkmcnt side: the tile loops' LDS-DMA rings live on counted
// vmcnt waits, and a compiler-visible global load in the loop would make hipcc drain them (vmcnt(0)) on every tile.  Issued
// under the tile's MFMAs, waited for in front of the epilogue: the latency sits under the multiply chain.  The wait names the
// destination, so no consumer is scheduled above it, and the tile's accumulators, so that hipcc cannot hoist it above the
// MFMAs (register-only instructions, which "memory" does not order) back to the load.
// (first: the first A operand(s) of the MFMAs that follow, named so that their chain stays below the load)
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
