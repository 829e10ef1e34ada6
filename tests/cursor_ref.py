"""Reference semantics of cursor search in numpy (no GPU, no product code).

The library's total order is (score desc, index asc).  Document n (global id g = n + idx_offset) with score s lies strictly
AFTER the cursor (a, i) iff  s < a  or  (s == a and g > i)  -- IEEE comparisons, so a NaN cursor score makes nothing eligible --
and a cursor search returns the first k eligible (and kept) documents in that order, tail (-inf, -1).  Scores come from the
untouched CPU oracle's score_all (float32, the kernels' chain); the order is a stable descending sort."""
import numpy as np

I64_MAX, I64_MIN = 2 ** 63 - 1, -(2 ** 63)
NEG_INF = np.float32(-np.inf)


def local_bound(after_idx, idx_offset, N):
    """clamp(after_idx - idx_offset, -1, N) in exact (Python) integers: what the kernels compare a document's position with."""
    return max(-1, min(int(N), int(after_idx) - int(idx_offset)))


def eligibility(S, after_val, after_idx, idx_offset=0, keep=None):
    """bool [B,N] from scores S f32 [B,N] and the cursors (after_val [B] f32, after_idx [B] int64, global ids)."""
    S = np.asarray(S, dtype=np.float32)
    a = np.broadcast_to(np.asarray(after_val, dtype=np.float32), S.shape[:1])[:, None]
    i = np.broadcast_to(np.asarray(after_idx, dtype=np.int64), S.shape[:1])[:, None]
    g = (np.arange(S.shape[1], dtype=np.int64) + np.int64(idx_offset))[None, :]      # (N + idx_offset stays far inside int64)
    with np.errstate(invalid="ignore"):
        elig = (S < a) | ((S == a) & (g > i))
    if keep is not None:
        elig = elig & np.asarray(keep, dtype=bool)[None, :]
    return elig


def first_k(S, elig, k, idx_offset=0):
    """(vals f32 [B,k], ids int64 [B,k]): per row the first k eligible documents of the stable descending sort."""
    B = S.shape[0]
    vals = np.full((B, k), NEG_INF, dtype=np.float32)
    ids = np.full((B, k), -1, dtype=np.int64)
    for b in range(B):
        cols = np.flatnonzero(elig[b])
        order = cols[np.argsort(-S[b, cols], kind="stable")][:k]                     # (cols ascend: stable = index asc)
        vals[b, :len(order)] = S[b, order]
        ids[b, :len(order)] = order + idx_offset
    return vals, ids


def search_after(S, after_val, after_idx, k, idx_offset=0, keep=None):
    return first_k(S, eligibility(S, after_val, after_idx, idx_offset, keep), k, idx_offset)


def expected(oracle, Qn, Dn, after_val, after_idx, k, rows, idx_offset=0, keep=None):
    """The cursor search of the queries `rows` of Qn over Dn (cursors given for ALL queries of Qn): the oracle's scores, the
    rule, the sort."""
    rows = np.asarray(rows)
    N = Dn.shape[0]
    S = oracle.score_all(np.ascontiguousarray(Qn[rows]), Dn) if N else np.zeros((len(rows), 0), dtype=np.float32)
    a = np.broadcast_to(np.asarray(after_val, dtype=np.float32), Qn.shape[:1])[rows]
    i = np.broadcast_to(np.asarray(after_idx, dtype=np.int64), Qn.shape[:1])[rows]
    return search_after(S, a, i, k, idx_offset, keep)


def walk(s_row, a, i, k, idx_offset=0):
    """The literal reading for one query: lay the whole row out in the total order, skip entries until the first one that is
    past the cursor, take k from there."""
    order = np.argsort(-s_row, kind="stable")
    vals, ids, started = [], [], False
    for n in order:
        s, g = s_row[n], int(n) + idx_offset
        if not started:
            started = bool(s < a) or bool(s == a and g > i)
        if started and len(ids) < k:
            vals.append(s)
            ids.append(g)
    pad = k - len(ids)
    return np.array(vals + [NEG_INF] * pad, dtype=np.float32), np.array(ids + [-1] * pad, dtype=np.int64)


def pages_until_tail(s_row, k, idx_offset=0, limit=100_000):
    """All pages of one query concatenated, each page's cursor the previous page's last entry, until a page ends in the tail."""
    S = np.asarray(s_row, dtype=np.float32)[None, :]
    a, i = np.float32(np.inf), -1
    vals, ids = [], []
    for _ in range(limit):
        v, x = search_after(S, [a], [i], k, idx_offset)
        vals.append(v[0])
        ids.append(x[0])
        a, i = v[0, -1], int(x[0, -1])
        if i == -1:
            break
    return np.concatenate(vals), np.concatenate(ids)


def ceiling(pos_scores, pos_ids, margin=0.0, ratio=None):
    """mine_hard_negatives' ceiling in numpy: min over the valid positives (id >= 0 and a score above -inf), minus margin or
    times ratio, in float32; +inf without a valid positive."""
    s = np.where((pos_ids >= 0) & (pos_scores > NEG_INF), pos_scores, np.float32(np.inf)).astype(np.float32)
    m = s.min(axis=1) if s.shape[1] else np.full(s.shape[0], np.inf, dtype=np.float32)
    return (m * np.float32(ratio) if ratio is not None else m - np.float32(margin)).astype(np.float32)


def mine(S, pos_ids, k, margin=0.0, ratio=None, idx_offset=0):
    """mine_hard_negatives over dense scores S [B,N]: the k best documents with score <= ceiling that are no positive."""
    B, N = S.shape
    local = pos_ids - idx_offset
    ok = (pos_ids >= 0) & (local >= 0) & (local < N)
    ps = np.where(ok, np.take_along_axis(S, np.clip(local, 0, max(N - 1, 0)), 1), NEG_INF).astype(np.float32)
    c = ceiling(ps, pos_ids, margin, ratio)
    elig = S <= c[:, None]
    for b in range(B):
        elig[b, local[b][ok[b]]] = False
    return first_k(S, elig, k, idx_offset), c
