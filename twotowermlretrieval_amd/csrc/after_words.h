// The cursor of one query, as the AFTER instantiations of the exact search kernels read and apply it (score_topk.hip: cursor
// search, DESIGN.md "Cursor search").  Plain integer and float code, host and device.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define TT_AFTER_FN __host__ __device__ __forceinline__
#else
#define TT_AFTER_FN inline
#endif

// The cursor's id is GLOBAL and any int64; the epilogue compares 32-bit local ids (documents 0 .. N - 1 of the call's D).  The
// local bound is clamp(after_idx - idx_offset, -1, N) as if in exact integers: an id below the shard's first (other shards,
// INT64_MIN) lies before every local document (-1: a tie at the cursor's score is eligible everywhere), one at or beyond its
// end (INT64_MAX) behind every one (N: no tie is).  The difference itself can leave int64 (INT64_MAX - (-5)), so it is never
// formed signed: below idx_offset is decided by the comparison, and from there on the unsigned difference is exact.
TT_AFTER_FN int after_local_bound(int64_t after_idx, int64_t idx_offset, int N)
{
    if (after_idx < idx_offset)
        return -1;
    const uint64_t diff = (uint64_t)after_idx - (uint64_t)idx_offset;
    return diff > (uint64_t)N ? N : (int)diff;
}

// Document doc (local id) with score s lies strictly after the cursor (a, cl) in the order (score desc, index asc).  IEEE
// comparisons: a NaN cursor score makes nothing eligible (a padded query's cursor), a NaN score is never eligible, -0.0 == +0.0.
TT_AFTER_FN bool after_eligible(float s, int doc, float a, int cl)
{
    return s < a || (s == a && doc > cl);
}
