"""Reference semantics of tagged search in numpy (no GPU, no product code).

Document n is eligible for query b iff (tags[n] & match_mask[b]) == match_value[b] -- all three read as UNSIGNED 32-bit words --
and, when a keep mask is given, keep[n].  A document's score does not depend on the other documents, so the expected result of
query b is the untouched CPU oracle's score_topk over that query's eligible rows with the indices mapped back, ties included
(what tests/test_masked_gpu.expected does for one mask shared by the batch)."""
import numpy as np


def as_u32(x, n=None):
    """x (an int, or an int32 / uint32 / int64 array holding 32-bit patterns) as a uint32 array; an int is broadcast to n."""
    if np.isscalar(x):
        return np.full(n, int(x) & 0xFFFFFFFF, dtype=np.uint32)
    x = np.asarray(x)
    if x.dtype == np.int32:
        return x.view(np.uint32)
    return (x.astype(np.int64) & 0xFFFFFFFF).astype(np.uint32)


def eligibility(tags, match_mask, match_value, keep=None, B=None):
    """bool [B, N]: row b is query b's eligible documents.  keep: optional bool [N] ANDed into every row."""
    tags = as_u32(tags)
    if B is None:
        B = len(match_mask) if not np.isscalar(match_mask) else len(match_value)
    mm, mv = as_u32(match_mask, B), as_u32(match_value, B)
    elig = (tags[None, :] & mm[:, None]) == mv[:, None]
    if keep is not None:
        elig &= np.asarray(keep, dtype=bool)[None, :]
    return elig


def expected(oracle, Qn, Dn, elig, k, rows, idx_offset=0):
    """(values f32 [len(rows), k], indices int64 [len(rows), k]) of the queries `rows`: the oracle over each query's own
    eligible rows of Dn, indices mapped back and offset, tail (-inf, -1)."""
    vals = np.full((len(rows), k), -np.inf, dtype=np.float32)
    idx = np.full((len(rows), k), -1, dtype=np.int64)
    for out, b in enumerate(rows):
        kept = np.flatnonzero(elig[b])
        if len(kept) == 0:
            continue
        v, i = oracle.score_topk(np.ascontiguousarray(Qn[b:b + 1]), np.ascontiguousarray(Dn[kept]), k)
        vals[out] = v[0]
        idx[out] = np.where(i[0] >= 0, kept[np.maximum(i[0], 0)] + idx_offset, -1)
    return vals, idx


def distinct_filters(match_mask, match_value, B):
    """[(mask, value, rows)]: the distinct (mask, value) pairs of a batch and the queries that carry each."""
    mm, mv = as_u32(match_mask, B), as_u32(match_value, B)
    groups = {}
    for b in range(B):
        groups.setdefault((int(mm[b]), int(mv[b])), []).append(b)
    return [(m, v, np.array(r)) for (m, v), r in groups.items()]
