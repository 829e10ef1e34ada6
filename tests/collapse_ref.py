"""Collapsed search (DESIGN.md "Collapsed search", include/tt.h at tt_topk_collapse_table) in numpy: the reference of
tests/test_collapse_*.py.  The rule is the literal walk of the contract; no arithmetic is done on scores, so everything the
tests compare is compared for equality."""
import numpy as np

NEG_INF = np.float32(-np.inf)


def walk(idx, gids, m):
    """Positions kept, in order, of one sorted row: idx int64 [M] (< 0 = padding, dropped), gids int64 [M] (negative =
    ungrouped).  An entry is kept if it is ungrouped or fewer than m entries of its group were kept before it."""
    kept_of = {}
    out = []
    for p in range(len(idx)):
        if idx[p] < 0:
            continue
        g = int(gids[p])
        if g >= 0:
            if kept_of.get(g, 0) >= m:
                continue
            kept_of[g] = kept_of.get(g, 0) + 1
        out.append(p)
    return out


def parallel(idx, gids, m):
    """The same positions by the form every entry decides alone: ungrouped, or fewer than m EARLIER ENTRIES OF THE ROW carry
    its group id (padding carries none)."""
    idx, gids = np.asarray(idx), np.asarray(gids)
    g = np.where(idx >= 0, gids, -1)
    return [p for p in range(len(idx)) if idx[p] >= 0 and (g[p] < 0 or int((g[:p] == g[p]).sum()) < m)]


def table_gids(idx, groups, off=0):
    """The group ids of entries idx by the table: groups[idx - off] inside [off, off + N), -1 (ungrouped) elsewhere."""
    idx = np.asarray(idx, np.int64)
    n = len(groups)
    out = np.full(idx.shape, -1, np.int64)
    ok = (idx >= off) & (idx >= 0)
    ok[ok] = (idx[ok] - off) < n          # (idx >= off here: the difference neither wraps nor goes negative)
    out[ok] = np.asarray(groups, np.int64)[idx[ok] - off]
    return out


def collapse_row(vals, idx, gids, k, m):
    """(out_val [k], out_idx [k], out_gid [k], (kept, complete)) of one row, as the C entries define them."""
    vals, idx, gids = np.asarray(vals, np.float32), np.asarray(idx, np.int64), np.asarray(gids, np.int64)
    picks = walk(idx, gids, m)
    kept = min(k, len(picks))
    ov, oi, og = np.full(k, NEG_INF, np.float32), np.full(k, -1, np.int64), np.full(k, -1, np.int64)
    sel = picks[:kept]
    ov[:kept], oi[:kept], og[:kept] = vals[sel], idx[sel], gids[sel]
    return ov, oi, og, (kept, int(kept == k or idx[-1] < 0))


def collapse(vals, idx, gids, k, m):
    """The batch form: [B,M] inputs -> (out_val [B,k], out_idx [B,k], out_gid [B,k], info int32 [B,2])."""
    rows = [collapse_row(vals[b], idx[b], gids[b], k, m) for b in range(len(vals))]
    return (np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows]), np.stack([r[2] for r in rows]),
            np.array([r[3] for r in rows], np.int32).reshape(len(rows), 2))


def sorted_row(scores, eligible=None, off=0):
    """(vals, idx) of ALL eligible rows of one query's scores [N] in (score desc, index asc) order, ids numbered from off."""
    n = np.arange(len(scores)) if eligible is None else np.flatnonzero(eligible)
    order = n[np.lexsort((n, -scores[n].astype(np.float64)))]
    return scores[order].astype(np.float32), order.astype(np.int64) + off


def search(scores, groups, k, m, eligible=None, off=0):
    """The contract applied to whole score rows: scores f32 [B,N] (oracle.score_all), groups int64 [N], eligible bool [N] or
    [B,N] or None -> (out_val, out_idx, out_gid) [B,k]: the walk over every eligible row, cut at k."""
    out = []
    for b in range(len(scores)):
        el = eligible if eligible is None or np.ndim(eligible) == 1 else eligible[b]
        v, i = sorted_row(scores[b], el, off)
        out.append(collapse_row(v, i, np.asarray(groups, np.int64)[i - off], k, m)[:3])
    return tuple(np.stack([o[j] for o in out]) for j in range(3))


def planted(n=4096, d=64, dups=1100, seed=81):
    """(D [n,d], Q [3,d], groups [n], where [dups]): unit rows; for query 0, `dups` near-duplicates of one passage -- one page,
    group 5 -- own the head of the list; the other rows are pages of four."""
    rs = np.random.RandomState(seed)
    D = rs.standard_normal((n, d)).astype(np.float32)
    D /= np.linalg.norm(D, axis=1, keepdims=True)
    Q = rs.standard_normal((3, d)).astype(np.float32)
    Q /= np.linalg.norm(Q, axis=1, keepdims=True)
    where = rs.permutation(n)[:dups]
    noise = rs.standard_normal((dups, d)).astype(np.float32)
    rows = Q[0] + np.float32(0.05) * noise / np.linalg.norm(noise, axis=1, keepdims=True)
    D[where] = rows / np.linalg.norm(rows, axis=1, keepdims=True)
    g = (np.arange(n, dtype=np.int64) // 4) + 10
    g[where] = 5
    return np.ascontiguousarray(D, np.float32), np.ascontiguousarray(Q, np.float32), g, where
