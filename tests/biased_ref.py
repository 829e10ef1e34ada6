"""Reference semantics of biased search in numpy (no GPU, no product code).

Document n's score for query b is fl32(s[b, n] + bias[n]): s is the CPU oracle's score_all -- the fp32 fmaf chain over the
feature index ascending from 0 -- and the addition is one float32 add, round to nearest even (numpy's).  The result is the
(score desc, index asc) selection of the kept documents, tail (-inf, -1).  With a bias of zeros this is oracle.score_topk bit
for bit (tests/test_biased_cpu.py checks it), so nothing new is needed under oracle/."""
import numpy as np


def expected(oracle, Qn, Dn, bias, k, rows, keep=None, idx_offset=0):
    """(values f32 [len(rows), k], indices int64 [len(rows), k]) of the queries `rows` of Qn over the documents Dn [N, d]
    (float32) under bias f32 [N] (longer: the first N count) and keep (optional bool [N])."""
    N = Dn.shape[0]
    rows = np.asarray(rows)
    bias = np.asarray(bias, dtype=np.float32)[:N]
    vals = np.full((len(rows), k), -np.inf, dtype=np.float32)
    idx = np.full((len(rows), k), -1, dtype=np.int64)
    if N == 0 or len(rows) == 0:
        return vals, idx
    S = oracle.score_all(np.ascontiguousarray(Qn[rows]), np.ascontiguousarray(Dn))
    Sb = (S + bias[None, :]).astype(np.float32)
    kept = np.arange(N) if keep is None else np.flatnonzero(np.asarray(keep, dtype=bool))
    for out in range(len(rows)):
        s = Sb[out, kept]
        order = np.lexsort((kept, -s))[:k]
        vals[out, :len(order)] = s[order]
        idx[out, :len(order)] = kept[order] + idx_offset
    return vals, idx


def bias_patterns(N, seed):
    """name -> float32 [N]: the bias patterns every grid case runs."""
    rs = np.random.RandomState(seed)
    n = np.arange(N, dtype=np.int64)
    out = {}
    out["zero"] = np.zeros(N, dtype=np.float32)
    out["constant"] = np.full(N, 0.25, dtype=np.float32)
    out["random"] = (rs.standard_normal(N) * 0.05).astype(np.float32)       # the scale of the scores' spread
    # every document of a 32-document tile has a bias of its own: a wrong row <-> register or lane-half mapping shows
    out["lane_map"] = (((7 * n) % 32).astype(np.float32) * np.float32(2.0 ** -5)).astype(np.float32)
    out["alt_tiles"] = np.where((n // 32) % 2 == 1, 1.0, -1.0).astype(np.float32)
    sp = np.zeros(N, dtype=np.float32)                                      # the last (partial) tile's last real row and row 0
    sp[0] = 100.0
    sp[N - 1] = 100.0
    out["spikes"] = sp
    # s + (-1e30) is -1e30 exactly: all but ~1 % of the rows tie at -1e30, across tiles and chunks
    ab = np.full(N, -1e30, dtype=np.float32)
    ab[rs.rand(N) < 0.01] = 0.0
    out["absorbing"] = ab
    out["ramp"] = (-(n.astype(np.float64)) * 1e-3).astype(np.float32)
    return out
