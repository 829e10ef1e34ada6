"""Fused lists (DESIGN.md "Fused lists", include/tt.h at tt_topk_fuse_rank_f32) in numpy: the reference of tests/test_fuse_*.py.
`walk` is the literal rule -- a Python dict per row, float32 adds in list order; `vectorised` the same by array operations.
Every step is a separately rounded float32 operation, so everything the tests compare is compared for equality."""
import numpy as np

NEG_INF = np.float32(-np.inf)


def rrf_table(L, M, c=60.0, weights=None):
    """w_l / (c + m + 1) in float64, rounded once: float32 [L,M]."""
    w = np.ones(L) if weights is None else np.asarray(weights, np.float64)
    return (w[:, None] / (np.float64(c) + np.arange(1, M + 1, dtype=np.float64))[None, :]).astype(np.float32)


def terms(vals, weight):
    """The score form's terms: fl32(weight[l] * vals[b][l][m]), float32 [B,L,M] (padding gives inf or NaN, never read)."""
    with np.errstate(invalid="ignore"):
        return (np.asarray(weight, np.float32)[None, :, None] * np.asarray(vals, np.float32)).astype(np.float32)


def walk_row(idx, term, missing, k):
    """One row: idx int64 [L,M], term float32 [L,M] (the term of every entry), missing float32 [L] ->
    (out_val [k], out_idx [k], out_pos [k,L])."""
    L, M = idx.shape
    pos = {}                                              # id -> [column of its live entry per list, -1 = absent]
    for l in range(L):
        for m in range(M):
            i = int(idx[l, m])
            if i < 0:
                continue
            p = pos.setdefault(i, [-1] * L)
            if p[l] < 0:                                  # the first occurrence in a list counts
                p[l] = m
    fused = {}
    for i, p in pos.items():
        acc = np.float32(0.0)
        for l in range(L):
            acc = np.float32(acc + (term[l, p[l]] if p[l] >= 0 else missing[l]))
        fused[i] = acc
    order = sorted(pos, key=lambda i: (-float(fused[i]), i))[:k]
    ov, oi, op = np.full(k, NEG_INF, np.float32), np.full(k, -1, np.int64), np.full((k, L), -1, np.int32)
    for r, i in enumerate(order):
        ov[r], oi[r], op[r] = fused[i], i, pos[i]
    return ov, oi, op


def walk(idx, term, missing, k):
    """The batch form: idx [B,L,M], term [B,L,M] or [L,M] (a rank table) -> (out_val [B,k], out_idx [B,k], out_pos [B,k,L])."""
    idx, term, missing = np.asarray(idx, np.int64), np.asarray(term, np.float32), np.asarray(missing, np.float32)
    rows = [walk_row(idx[b], term if term.ndim == 2 else term[b], missing, k) for b in range(len(idx))]
    return tuple(np.stack([r[j] for r in rows]) for j in range(3))


def vectorised_row(idx, term, missing, k):
    """The same by arrays: the ids of the union, a [U,L] matrix of first columns, a float32 add per list, one lexsort."""
    L, M = idx.shape
    ids = np.unique(idx[idx >= 0])
    U = len(ids)
    pos = np.full((U, L), -1, np.int32)
    for l in range(L):
        live = idx[l] >= 0
        first_ids, first_col = np.unique(idx[l][live], return_index=True)      # (the first index of every distinct value)
        pos[np.searchsorted(ids, first_ids), l] = np.flatnonzero(live)[first_col]
    acc = np.zeros(U, np.float32)
    for l in range(L):
        t = np.where(pos[:, l] >= 0, term[l][np.maximum(pos[:, l], 0)], missing[l]).astype(np.float32)
        acc = (acc + t).astype(np.float32)
    order = np.lexsort((ids, -acc.astype(np.float64)))[:k]
    ov, oi, op = np.full(k, NEG_INF, np.float32), np.full(k, -1, np.int64), np.full((k, L), -1, np.int32)
    n = len(order)
    ov[:n], oi[:n], op[:n] = acc[order], ids[order], pos[order]
    return ov, oi, op


def vectorised(idx, term, missing, k):
    idx, term, missing = np.asarray(idx, np.int64), np.asarray(term, np.float32), np.asarray(missing, np.float32)
    rows = [vectorised_row(idx[b], term if term.ndim == 2 else term[b], missing, k) for b in range(len(idx))]
    return tuple(np.stack([r[j] for r in rows]) for j in range(3))


def fuse_rank(idx, table, missing, k):
    """tt_topk_fuse_rank_f32 as the contract states it."""
    return vectorised(idx, table, missing, k)


def fuse_score(vals, idx, weight, missing, k):
    """tt_topk_fuse_score_f32 as the contract states it."""
    return vectorised(idx, terms(vals, weight), missing, k)


def pack(lists, need_vals=True):
    """Lists [(vals [B,M_l], idx [B,M_l])] as one ([B,L,M], [B,L,M]) pair padded with (-inf, -1), as fuse_topk packs them."""
    B, L, M = len(lists[0][1]), len(lists), max(i.shape[1] for _, i in lists)
    vals, idx = np.full((B, L, M), NEG_INF, np.float32), np.full((B, L, M), -1, np.int64)
    for l, (v, i) in enumerate(lists):
        idx[:, l, :i.shape[1]] = i
        if need_vals and v is not None:
            vals[:, l, :i.shape[1]] = v
    return vals, idx


# ---- rows for the tests ------------------------------------------------------------------------------------------------------

BIG = 1 << 62


def _list(rs, pool, n_valid, M):
    """One list: n_valid distinct ids of pool in random order, then padding."""
    out = np.full(M, -1, np.int64)
    out[:n_valid] = rs.choice(pool, n_valid, replace=False)
    return out


def row_patterns(rs, B, L, M):
    """name -> idx int64 [B,L,M]: the overlap patterns of the contract."""
    E = L * M
    out = {}
    out["disjoint"] = np.stack([rs.permutation(E).reshape(L, M) + 5 for _ in range(B)])
    one = np.stack([rs.permutation(3 * M)[:M] for _ in range(B)])
    out["identical"] = np.repeat(one[:, None, :], L, axis=1)
    out["half_overlap"] = np.stack([np.stack([_list(rs, max(2 * M, 2), M, M) for _ in range(L)]) for _ in range(B)])
    pad = out["half_overlap"].copy()
    pad[:, rs.randint(L)] = -1
    out["one_list_padding"] = pad
    ragged = np.full((B, L, M), -1, np.int64)
    for b in range(B):
        for l in range(L):
            n = (0, 1, M)[(b + l) % 3] if (b + l) % 4 else rs.randint(0, M + 1)
            ragged[b, l] = _list(rs, max(2 * M, 2), min(n, M), M)
    out["ragged"] = ragged
    dup = out["half_overlap"].copy()
    if M >= 2:
        for b in range(B):
            for l in range(L):
                src, dst = sorted(rs.choice(M, 2, replace=False))
                dup[b, l, dst] = dup[b, l, src]                   # a duplicate id inside a list: the first occurrence counts
    out["duplicate"] = dup
    big = out["half_overlap"].copy()
    big = np.where(big % 3 == 0, BIG - big, big)              # ids at 2^62 next to small ones, 0 among them
    out["big_ids"] = big
    return {k: np.ascontiguousarray(v, np.int64) for k, v in out.items()}


def values_for(rs, idx, negative=True):
    """Scores for the score form: descending inside a list like a search's, negative ones included, -inf on padding."""
    B, L, M = idx.shape
    v = rs.standard_normal((B, L, M)).astype(np.float32) * 3
    if not negative:
        v = np.abs(v)
    v = -np.sort(-v, axis=-1)
    return np.where(idx >= 0, v, NEG_INF).astype(np.float32)
