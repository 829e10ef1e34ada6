"""The diversified selection (include/tt.h at tt_mmr_select_f32) in numpy float32: the reference of tests/test_mmr_*.py.

The similarity is the oracle's: G = oracle.score_all(X, X) over the candidates' rows -- the fp32 fmaf chain over the feature
index ascending, the project's defined score applied to two documents.  Everything else is three float32 operations per
candidate and step, each rounded on its own (numpy float32 arithmetic does not fuse), and an argmax with ties to the lower
position."""
import numpy as np

NEG_INF = np.float32(-np.inf)


def valid_mask(vals, idx, off=0, n=None):
    """Candidates that may be selected: a finite relevance, an id >= 0 and (corpus form: n given) off <= id < off + n."""
    idx = np.asarray(idx)
    ok = np.isfinite(vals) & (idx >= 0)
    if n is not None:
        # (the difference in unsigned arithmetic: exact for every id >= max(off, 0), no overflow at the int64 edge)
        ok &= (idx >= off) & (idx.astype(np.uint64) - np.uint64(off % 2 ** 64) < np.uint64(n))
    return ok


def gram(oracle, X):
    """G [C,C] of rows X [C,d] (float32; bf16 rows widened exactly first)."""
    X = np.ascontiguousarray(X, dtype=np.float32)
    if X.shape[0] == 0:
        return np.zeros((0, 0), np.float32)
    return oracle.score_all(X, X)


def greedy(rel, ok, G, k, lam):
    """Positions picked, in order (at most k, fewer when the valid candidates run out)."""
    lam = np.float32(lam)
    mu = np.float32(1.0) - lam
    rel = np.asarray(rel, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        a = (lam * rel).astype(np.float32)
    left = np.array(ok, dtype=bool).copy()
    pen = np.full(len(rel), NEG_INF, np.float32)
    picks = []
    for t in range(k):
        if not left.any():
            break
        if t == 0:
            m = a
        else:
            with np.errstate(invalid="ignore", over="ignore"):
                m = (a - (mu * pen).astype(np.float32)).astype(np.float32)
        cand = np.flatnonzero(left)
        best = cand[np.argmax(m[cand])]   # (the first maximum: ties keep the lower position)
        picks.append(int(best))
        left[best] = False
        pen = np.maximum(pen, G[best]).astype(np.float32)   # G[best] == G[:, best] bit for bit
    return picks


def outputs(vals, idx, picks, k):
    """(out_val [k], out_idx [k], out_pos [k]) of one query: the picks' relevance, id and position, tail (-inf, -1, -1)."""
    ov, oi, op = np.full(k, NEG_INF, np.float32), np.full(k, -1, np.int64), np.full(k, -1, np.int32)
    n = len(picks)
    ov[:n], oi[:n], op[:n] = np.asarray(vals, np.float32)[picks], np.asarray(idx, np.int64)[picks], picks
    return ov, oi, op


def candidate_rows(D, idx, ok, off=0):
    """X [C,d]: row idx - off of D where the candidate is valid, zeros elsewhere (an invalid candidate is never selected)."""
    X = np.zeros((len(idx), D.shape[1]), np.float32)
    for c in np.flatnonzero(ok):
        X[c] = D[int(idx[c]) - off]
    return X


def select(oracle, vals, idx, D, k, lam, off=0):
    """The corpus form over a batch: vals f32 [B,C], idx int64 [B,C], D f32 [N,d] -> (out_val, out_idx, out_pos) [B,k]."""
    vals, idx = np.asarray(vals, np.float32), np.asarray(idx, np.int64)
    ok = valid_mask(vals, idx, off, D.shape[0])
    out = [outputs(vals[b], idx[b], greedy(vals[b], ok[b], gram(oracle, candidate_rows(D, idx[b], ok[b], off)), k, lam), k)
           for b in range(len(vals))]
    return tuple(np.stack([o[j] for o in out]) if out else np.zeros((0, k), t) for j, t in enumerate((np.float32, np.int64, np.int32)))


def planted_cluster(seed, n=20_000, d=256, nq=8, dups=40, cos=0.9):
    """(D [n,d], Q [nq,d], cluster [nq,dups] row numbers): unit rows; for query b a row with cosine `cos` to it and dups - 1
    near-duplicates of that row (noise of norm 1e-3 * (j + 1) on duplicate j, renormalised), planted at random rows."""
    rs = np.random.RandomState(seed)
    D = rs.standard_normal((n, d)).astype(np.float32)
    D /= np.linalg.norm(D, axis=1, keepdims=True)
    Q = rs.standard_normal((nq, d)).astype(np.float32)
    Q /= np.linalg.norm(Q, axis=1, keepdims=True)
    where = rs.permutation(n)[:nq * dups].reshape(nq, dups)
    for b in range(nq):
        u = rs.standard_normal(d)
        u -= (u @ Q[b].astype(np.float64)) * Q[b]
        u /= np.linalg.norm(u)
        base = cos * Q[b] + np.sqrt(1.0 - cos * cos) * u
        for j in range(dups):
            e = rs.standard_normal(d)
            row = base + 1e-3 * (j + 1) * e / np.linalg.norm(e)
            D[where[b, j]] = (row / np.linalg.norm(row)).astype(np.float32)
    return D, Q, where
