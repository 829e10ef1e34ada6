"""Fused lists on the GPU: the two kernel entries (tt_topk_fuse_rank_f32 / _score_f32 through fuse_topk and through the C ABI),
HybridIndex on every dense layout, and fused_search.

The expected value is the contract itself (fuse_ref: a dict per row, float32 adds in list order), applied to the rows handed to
the kernel.  Every step of the rule is one rounded float32 operation, so values, indices and positions are compared bit for
bit."""
import ctypes

import numpy as np
import pytest
import torch

import fuse_ref
import lexical_ref
import synth
from poison import PATTERNS, pattern_id, poisoned_empty

pytestmark = pytest.mark.gpu

SHAPES = ((1, 1), (1, 63), (1, 64), (1, 65), (1, 255), (1, 256), (1, 257), (1, 1024), (2, 32), (2, 128), (2, 512), (3, 85),
          (3, 341), (8, 8), (8, 128))


@pytest.fixture(scope="module")
def tt():
    import twotowermlretrieval_amd as m
    from twotowermlretrieval_amd import _lib
    _lib.lib()
    assert torch.cuda.is_available()
    return m


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()


def host(ts):
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in ts)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(got, want, what=""):
    """got: device tensors; want: numpy arrays; equal in shape, dtype and every bit."""
    for n, (g, w) in enumerate(zip(host(got), want)):
        assert g.shape == w.shape and g.dtype == w.dtype, (what, n, g.shape, w.shape, g.dtype, w.dtype)
        assert np.array_equal(bits(g), bits(w)), (what, n, int((bits(g) != bits(w)).sum()))


def cut(want, k):
    """The first k results of a reference computed for every entry: the result for k is its prefix."""
    return tuple(w[:, :k] for w in want)


def lists_of(vals, idx):
    """[B,L,M] arrays as the device lists fuse_topk takes."""
    vd, id_ = (None if vals is None else dev(vals)), dev(idx)
    return [(None if vd is None else vd[:, l], id_[:, l]) for l in range(idx.shape[1])]


def ks(E):
    return sorted({1, min(10, E), E})


# ---- the kernel entries ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("L,M", SHAPES)
@pytest.mark.parametrize("B", (1, 33))
def test_rank_form_bit_for_bit(tt, B, L, M):
    """M crosses the wave and the workgroup, L * M one to four entries per thread up to the LDS limit; a table of the caller's
    (a device tensor) and the cached reciprocal-rank table; missing != 0."""
    rs = np.random.RandomState(1000 * B + 10 * M + L)
    E = L * M
    w = tuple(float(x) for x in np.round(rs.rand(L) + 0.5, 3))
    own = (rs.rand(L, M).astype(np.float32) - np.float32(0.3))               # any finite table: not monotone, negative entries
    missing = (rs.rand(L) * 0.01 - 0.005).astype(np.float32)
    for name, idx in fuse_ref.row_patterns(rs, B, L, M).items():
        lists = lists_of(None, idx)
        want_rrf = fuse_ref.fuse_rank(idx, fuse_ref.rrf_table(L, M, 60.0, w), np.zeros(L, np.float32), E)
        want_own = fuse_ref.fuse_rank(idx, own, missing, E)
        for k in ks(E):
            same(tt.fuse_topk(lists, k, weights=w, return_positions=True), cut(want_rrf, k), (name, k, "rrf"))
            same(tt.fuse_topk(lists, k, weights=dev(own), missing=dev(missing), return_positions=True), cut(want_own, k), (name, k, "own"))
        same(tt.fuse_topk(lists, min(10, E), weights=w), cut(want_rrf, min(10, E))[:2], (name, "no positions"))


@pytest.mark.parametrize("L,M", SHAPES)
@pytest.mark.parametrize("B", (1, 33))
def test_score_form_bit_for_bit(tt, B, L, M):
    """Negative values, negative weights and missing != 0: the multiply and every add are separately rounded."""
    rs = np.random.RandomState(2000 * B + 10 * M + L)
    E = L * M
    weight = (rs.standard_normal(L) * 1.7).astype(np.float32)
    missing = (rs.standard_normal(L) * 0.5).astype(np.float32)
    for name, idx in fuse_ref.row_patterns(rs, B, L, M).items():
        vals = fuse_ref.values_for(rs, idx)
        lists = lists_of(vals, idx)
        want = fuse_ref.fuse_score(vals, idx, weight, missing, E)
        for k in ks(E):
            got = tt.fuse_topk(lists, k, method="score", weights=dev(weight), missing=tuple(float(x) for x in missing),
                               return_positions=True)
            same(got, cut(want, k), (name, k))


def test_planted_tie_and_extreme_ids(tt):
    """a at columns (0, 1) and b at (1, 0) with equal weights: the same two terms, so the ids decide -- also at 0 and 2^62."""
    for a, b in ((7, 9), (9, 7), (0, fuse_ref.BIG), (fuse_ref.BIG, fuse_ref.BIG - 1)):
        idx = np.array([[[a, b, 100, 101], [b, a, 102, 103]]], np.int64)
        v, i, p = host(tt.fuse_topk(lists_of(None, idx), 8, return_positions=True))
        assert i[0, :2].tolist() == sorted((a, b)) and v[0, 0] == v[0, 1]
        same(tt.fuse_topk(lists_of(None, idx), 8, return_positions=True),
             fuse_ref.fuse_rank(idx, fuse_ref.rrf_table(2, 4), np.zeros(2, np.float32), 8))
        assert (i[0, 6:] == -1).all() and np.isneginf(v[0, 6:]).all() and (p[0, 6:] == -1).all()


def test_an_fma_would_show(tt):
    """Values chosen so that fl32(acc + fl32(w * v)) differs from the contracted fma(w, v, acc) in most rows."""
    rs = np.random.RandomState(9)
    B, L, M = 33, 2, 32
    idx = fuse_ref.row_patterns(rs, B, L, M)["identical"]
    vals = fuse_ref.values_for(rs, idx)
    weight = np.array([1.0 / 3.0, 0.7], np.float32)
    missing = np.zeros(L, np.float32)
    want = fuse_ref.fuse_score(vals, idx, weight, missing, M)
    t = fuse_ref.terms(vals, weight)
    fused_fma = (t[:, 0].astype(np.float64) + weight[1].astype(np.float64) * vals[:, 1].astype(np.float64)).astype(np.float32)
    separate = (t[:, 0] + t[:, 1]).astype(np.float32)
    assert (bits(fused_fma) != bits(separate)).mean() > 0.05                   # the case can tell the two apart
    same(tt.fuse_topk(lists_of(vals, idx), M, method="score", weights=tuple(float(x) for x in weight), return_positions=True), want)


def test_lists_of_different_widths_and_one_query(tt):
    rs = np.random.RandomState(10)
    B = 5
    a = np.stack([rs.permutation(300)[:40] for _ in range(B)]).astype(np.int64)
    b = np.stack([rs.permutation(300)[:7] for _ in range(B)]).astype(np.int64)
    c = np.stack([rs.permutation(300)[:64] for _ in range(B)]).astype(np.int64)
    c[:, 50:] = -1
    _, idx = fuse_ref.pack([(None, a), (None, b), (None, c)], need_vals=False)
    assert idx.shape == (B, 3, 64)
    want = fuse_ref.fuse_rank(idx, fuse_ref.rrf_table(3, 64, 10.0), np.zeros(3, np.float32), 20)
    lists = [(None, dev(x)) for x in (a, b, c)]
    same(tt.fuse_topk(lists, 20, c=10.0, return_positions=True), want)
    one = tt.fuse_topk([(None, i[2]) for _, i in lists], 20, c=10.0, return_positions=True)
    assert one[0].dim() == 1 and one[2].shape == (20, 3)
    same(one, tuple(w[2] for w in want))


def test_minmax_normalisation_is_torch_in_front_of_the_kernel(tt):
    rs = np.random.RandomState(11)
    B, L, M = 4, 2, 16
    idx = fuse_ref.row_patterns(rs, B, L, M)["ragged"]
    vals = fuse_ref.values_for(rs, idx)
    vals[0, 0, :] = np.where(idx[0, 0] >= 0, np.float32(2.5), fuse_ref.NEG_INF)      # a constant list maps to 1
    vd, id_ = dev(vals), dev(idx)
    valid = id_ >= 0
    lo = torch.where(valid, vd, torch.full_like(vd, float("inf"))).amin(-1, keepdim=True)
    hi = torch.where(valid, vd, torch.full_like(vd, float("-inf"))).amax(-1, keepdim=True)
    unit = torch.where(valid, torch.where(hi > lo, (vd - lo) / (hi - lo), torch.ones_like(vd)), torch.full_like(vd, float("-inf")))
    norm = host((unit,))[0]
    live = idx >= 0
    assert norm[live].min() >= 0.0 and norm[live].max() <= 1.0 and (norm[0, 0][live[0, 0]] == 1.0).all()
    want = fuse_ref.fuse_score(norm, idx, np.ones(L, np.float32), np.zeros(L, np.float32), 10)
    same(tt.fuse_topk(lists_of(vals, idx), 10, method="score", normalize="minmax", return_positions=True), want)


@pytest.mark.parametrize("word", PATTERNS, ids=pattern_id)
def test_outputs_do_not_depend_on_what_they_held(tt, word):
    """Fresh outputs from a poisoning allocator, and out= tensors filled with the pattern: short rows end in (-inf, -1, -1)."""
    from poison import fill_bytes
    rs = np.random.RandomState(12)
    B, L, M = 33, 2, 128
    idx = fuse_ref.row_patterns(rs, B, L, M)["ragged"]
    vals = fuse_ref.values_for(rs, idx)
    weight, missing = np.array([0.5, -1.25], np.float32), np.array([0.125, 0.0], np.float32)
    k = L * M
    want_s = fuse_ref.fuse_score(vals, idx, weight, missing, k)
    want_r = fuse_ref.fuse_rank(idx, fuse_ref.rrf_table(L, M), np.zeros(L, np.float32), k)
    assert (want_r[1] == -1).any()
    lists = lists_of(vals, idx)
    torch.cuda.synchronize()
    with poisoned_empty(word) as p:
        got_s = tt.fuse_topk(lists, k, method="score", weights=tuple(weight.tolist()), missing=tuple(missing.tolist()),
                             return_positions=True)
        got_r = tt.fuse_topk(lists, k, return_positions=True)
    assert p.tensors >= 6
    same(got_s, want_s)
    same(got_r, want_r)
    out = (torch.zeros((B, k), dtype=torch.float32, device="cuda"), torch.zeros((B, k), dtype=torch.int64, device="cuda"),
           torch.zeros((B, k, L), dtype=torch.int32, device="cuda"))
    for t in out:
        fill_bytes(t, word)
    res = tt.fuse_topk(lists, k, return_positions=True, out=out)
    assert all(r is o for r, o in zip(res, out))
    same(out, want_r)
    for t in out[:2]:
        fill_bytes(t, word)
    res = tt.fuse_topk(lists, k, method="score", weights=tuple(weight.tolist()), missing=tuple(missing.tolist()), out=out[:2])
    same(res, want_s[:2])


def test_graph_replay_over_rewritten_inputs_and_weights(tt):
    rs = np.random.RandomState(13)
    B, L, M, k = 9, 3, 85, 10
    cases = []
    for n, name in enumerate(("half_overlap", "duplicate", "ragged")):
        idx = fuse_ref.row_patterns(rs, B, L, M)[name]
        vals = fuse_ref.values_for(rs, idx)
        weight = (rs.standard_normal(L) + 2).astype(np.float32)
        table = fuse_ref.rrf_table(L, M, 20.0 * (n + 1), rs.rand(L) + 0.5)
        cases.append((vals, idx, weight, table, fuse_ref.fuse_score(vals, idx, weight, np.zeros(L, np.float32), k),
                      fuse_ref.fuse_rank(idx, table, np.zeros(L, np.float32), k)))
    vd, id_, wd, td = (dev(x) for x in cases[0][:4])
    lists = [(vd[:, l], id_[:, l]) for l in range(L)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                              # warm-up outside capture: the cached vectors
        tt.fuse_topk(lists, k, method="score", weights=wd, return_positions=True)
        tt.fuse_topk(lists, k, weights=td, return_positions=True)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out_s = tt.fuse_topk(lists, k, method="score", weights=wd, return_positions=True)
        out_r = tt.fuse_topk(lists, k, weights=td, return_positions=True)
    for n in (1, 2, 0):
        vals, idx, weight, table, want_s, want_r = cases[n]
        vd.copy_(dev(vals))
        id_.copy_(dev(idx))
        wd.copy_(dev(weight))
        td.copy_(dev(table))
        for t in (*out_s, *out_r):
            t.fill_(7)
        graph.replay()
        same(out_s, want_s, n)
        same(out_r, want_r, n)


def test_argument_errors_through_the_c_abi(tt):
    from twotowermlretrieval_amd import _lib
    L_ = _lib.lib()
    B, L, M, k = 2, 2, 8, 4
    iv = torch.zeros((B, L, M + 1), dtype=torch.float32, device="cuda")
    ii = torch.zeros((B, L, M + 1), dtype=torch.int64, device="cuda")
    tab = torch.zeros((L, M + 1), dtype=torch.float32, device="cuda")
    miss = torch.zeros(L + 1, dtype=torch.float32, device="cuda")
    ov = torch.full((B, k + 1), 3.0, dtype=torch.float32, device="cuda")
    oi = torch.full((B, k + 1), 3, dtype=torch.int64, device="cuda")
    op = torch.full((B, k + 1, L), 3, dtype=torch.int32, device="cuda")
    p = lambda t: t.data_ptr()  # noqa: E731

    def rank(in_idx=p(ii), B=B, L=L, M=M, table=p(tab), missing=p(miss), k=k, out_val=p(ov), out_idx=p(oi), out_pos=p(op)):
        return L_.tt_topk_fuse_rank_f32(in_idx, B, L, M, table, missing, k, out_val, out_idx, out_pos, None)

    def score(in_val=p(iv), in_idx=p(ii), B=B, L=L, M=M, weight=p(tab), missing=p(miss), k=k, out_val=p(ov), out_idx=p(oi),
              out_pos=p(op)):
        return L_.tt_topk_fuse_score_f32(in_val, in_idx, B, L, M, weight, missing, k, out_val, out_idx, out_pos, None)

    bad, unsup = _lib.TT_ERR_BAD_SHAPE, _lib.TT_ERR_UNSUPPORTED
    for fn in (rank, score):
        assert fn(k=0) == bad and fn(k=L * M + 1) == bad and fn(B=-1) == bad and fn(L=0) == bad and fn(M=0) == bad
        assert fn(L=9, M=1) == unsup and fn(L=1, M=1025, k=1) == unsup and fn(L=8, M=129, k=1) == unsup
        assert b"L=8 M=129" in L_.tt_last_error()
        assert fn(in_idx=None) == bad and fn(missing=None) == bad and fn(out_val=None) == bad and fn(out_idx=None) == bad
        assert fn(in_idx=p(ii) + 4) == bad and fn(out_idx=p(oi) + 4) == bad                  # int64: 8-byte alignment
        assert fn(missing=p(miss) + 2) == bad and fn(out_val=p(ov) + 2) == bad and fn(out_pos=p(op) + 2) == bad
        assert fn(out_idx=p(ii) + 8) == bad and b"alias" in L_.tt_last_error()               # out overlaps in
        assert fn(out_val=p(miss)) == bad and fn(out_pos=p(tab)) == bad
        assert fn(B=0, in_idx=None, out_val=None, out_idx=None, out_pos=None) == _lib.TT_OK  # B = 0 does nothing
    assert rank(table=None) == bad and rank(table=p(tab) + 2) == bad
    assert score(in_val=None) == bad and score(weight=None) == bad and score(in_val=p(iv) + 2) == bad
    assert score(out_val=p(iv) + 4) == bad
    torch.cuda.synchronize()
    assert bool((ov == 3).all()) and bool((oi == 3).all()) and bool((op == 3).all())         # no refused call wrote anything
    assert rank(out_pos=None) == _lib.TT_OK and score(out_pos=None) == _lib.TT_OK            # positions are optional
    torch.cuda.synchronize()
    assert bool((op == 3).all()) and bool((oi.flatten()[:B * k] != 3).all())


# ---- HybridIndex and fused_search --------------------------------------------------------------------------------------------

N, D_, F, NQ = 4096, 64, 512, 40
OFF = 1000
_CORPUS = {}


def corpus():
    """Dense unit rows on the bf16 grid (one corpus serves every layout), a random CSR over the same ids, NQ queries of both
    kinds.  Built once, read-only."""
    if not _CORPUS:
        D = torch.from_numpy(synth.unit_rows(71, N, D_).copy()).to(torch.bfloat16).to(torch.float32).numpy()
        Q = synth.unit_rows(72, NQ, D_).copy()
        Q[3] = D[77]                                                               # a query that is a document
        indptr, cols, vals = lexical_ref.random_corpus(73, N, F, max_len=30)
        rng = np.random.default_rng(74)
        queries = [(np.sort(rng.choice(F, size=int(rng.integers(1, 9)), replace=False)), rng.uniform(0.1, 1.0, size=8)) for _ in range(NQ)]
        queries = [(c, v[:len(c)]) for c, v in queries]
        for a in (D, Q):
            a.setflags(write=False)
        _CORPUS.update(D=D, Q=Q, csr=(indptr, cols, vals), q_csr=lexical_ref.queries_csr(queries))
    return _CORPUS


def dense_index(tt, layout, monkeypatch):
    from twotowermlretrieval_amd import index as _index
    D = torch.from_numpy(corpus()["D"].copy())
    if layout == "f32":
        return tt.BruteForceIndex(D.cuda(), idx_offset=OFF)
    if layout == "bf16":
        return tt.BruteForceIndex(D.cuda().to(torch.bfloat16), idx_offset=OFF)
    if layout == "screened":
        monkeypatch.setattr(_index, "SCREEN_MIN_DOCS", 0)
        monkeypatch.setattr(_index, "SCREEN_PADDED_MIN_BATCH", 33)
        ix = tt.BruteForceIndex(D.cuda(), idx_offset=OFF, screen=True)
        assert ix._screens(NQ, 64)
        return ix
    assert layout == "streamed"
    ix = tt.StreamedIndex(D.to(torch.bfloat16), block_docs=1504, idx_offset=OFF)   # three blocks, on mask-word boundaries
    assert -(-N // ix.block) == 3
    return ix


def lexical_index(tt):
    indptr, cols, vals = corpus()["csr"]
    return tt.LexicalIndex((dev(indptr), dev(cols), dev(vals), F), idx_offset=OFF)


def expect(dl, ll, k, c=60.0, w=None, method="rrf"):
    """fuse_ref over two device lists, with each result's scores in the two lists (NaN where absent)."""
    (dv, di), (lv, li) = host(dl), host(ll)
    vals, idx = fuse_ref.pack([(dv, di), (lv, li)])
    if method == "rrf":
        fv, fi, pos = fuse_ref.fuse_rank(idx, fuse_ref.rrf_table(2, idx.shape[2], c, w), np.zeros(2, np.float32), k)
    else:
        fv, fi, pos = fuse_ref.fuse_score(vals, idx, np.ones(2, np.float32) if w is None else np.asarray(w, np.float32),
                                          np.zeros(2, np.float32), k)
    comp = [np.where(pos[:, :, l] >= 0, np.take_along_axis(vals[:, l], np.maximum(pos[:, :, l], 0), 1), np.float32(np.nan))
            for l in range(2)]
    return fv, fi, comp[0].astype(np.float32), comp[1].astype(np.float32)


def same_nan(got, want, what=""):
    for n, (g, w) in enumerate(zip(host(got), want)):
        assert g.shape == w.shape and g.dtype == w.dtype, (what, n)
        assert lexical_ref.same_bits(g, w) if g.dtype == np.float32 else np.array_equal(g, w), (what, n)


@pytest.mark.parametrize("layout", ["f32", "bf16", "screened", "streamed"])
def test_hybrid_index_equals_the_two_searches_plus_the_rule(tt, layout, monkeypatch):
    c = corpus()
    dense, lex = dense_index(tt, layout, monkeypatch), lexical_index(tt)
    hy = tt.HybridIndex(dense, lex)
    Q, ql = dev(c["Q"]), tuple(dev(a) for a in c["q_csr"])
    # defaults: k = 10 fetches min(max(40, 64), 512) = 64 from each side
    dl, ll = dense.search(Q, 64), lex.search(ql, 64)
    want = expect(dl, ll, 10)
    same(hy.search(Q, ql), want[:2], "defaults")
    same_nan(hy.search(Q, ql, return_components=True), want, "components")
    assert np.isnan(want[2]).any() and np.isnan(want[3]).any() and not (np.isnan(want[2]) & np.isnan(want[3])).any()
    # another fetch_k, c and weights; the score form
    dl, ll = dense.search(Q, 100), lex.search(ql, 100)
    same_nan(hy.search(Q, ql, 25, fetch_k=100, c=5.0, weights=(0.25, 0.75), return_components=True),
             expect(dl, ll, 25, 5.0, (0.25, 0.75)), "weights")
    same_nan(hy.search(Q, ql, 25, fetch_k=100, method="score", weights=(1.0, 0.5), return_components=True),
             expect(dl, ll, 25, w=(1.0, 0.5), method="score"), "score")
    # lex_min_score: documents that share no term with the query stay out of the lexical list
    ll0 = lex.search(ql, 64, min_score=0.5)
    assert bool((ll0[1] < 0).any()) and bool((ll0[1][:, 0] >= 0).any())
    same(hy.search(Q, ql, lex_min_score=0.5), expect(dense.search(Q, 64), ll0, 10)[:2], "min_score")
    # one query
    one = hy.search(Q[3], tuple(dev(a) for a in lexical_ref.queries_csr([(c["q_csr"][1][c["q_csr"][0][3]:c["q_csr"][0][4]],
                                                                       c["q_csr"][2][c["q_csr"][0][3]:c["q_csr"][0][4]])])))
    assert one[0].dim() == 1
    same(one, tuple(w[3] for w in want[:2]), "one query")
    # keep=: both searches see the mask
    keep_bool = torch.ones(N, dtype=torch.bool, device="cuda")
    gone = torch.from_numpy(want[1][:, 0].copy()).cuda() - OFF
    keep_bool[gone] = False
    keep = tt.pack_keep_mask(keep_bool)
    got = hy.search(Q, ql, keep=keep, return_components=True)
    same_nan(got, expect(dense.search(Q, 64, keep=keep), lex.search(ql, 64, keep=keep), 10), "keep")
    assert not bool(torch.isin(got[1], gone + OFF).any())
    # exclude=: per-query lists, filtered out of both sides
    ex = torch.from_numpy(np.ascontiguousarray(want[1][:, :3])).cuda()
    got = hy.search(Q, ql, exclude=ex, return_components=True)
    lv, li = tt.topk_exclude(*lex.search(ql, 67), ex, 64)
    same_nan(got, expect(dense.search(Q, 64, exclude=ex), (lv, li), 10), "exclude")
    assert not bool((got[1].unsqueeze(2) == ex.unsqueeze(1)).any())
    with pytest.raises(ValueError, match="k = "):
        hy.search(Q, ql, 200, fetch_k=64)


def test_fused_search_over_query_variants(tt):
    c = corpus()
    ix = tt.BruteForceIndex(dev(c["D"]), idx_offset=OFF)
    rs = np.random.RandomState(14)
    B, V = 6, 3
    base = c["Q"][:B]
    var = base[:, None, :] + 0.05 * rs.standard_normal((B, V, D_)).astype(np.float32)
    var = (var / np.linalg.norm(var, axis=-1, keepdims=True)).astype(np.float32)
    var[:, 0] = base
    vd = dev(var)
    sv, si = host(ix.search(vd.reshape(B * V, D_), 64))
    vals, idx = sv.reshape(B, V, 64), si.reshape(B, V, 64)
    assert len(np.unique(idx[0])) < idx[0].size                                         # the variants' lists overlap
    want = fuse_ref.fuse_rank(idx, fuse_ref.rrf_table(V, 64), np.zeros(V, np.float32), 10)
    same(tt.fused_search(ix, vd, 10, return_positions=True), want, "rrf")
    same(tt.fused_search(ix, vd, 10), want[:2], "rrf")
    one = tt.fused_search(ix, vd[2], 10)
    assert one[0].dim() == 1
    same(one, tuple(w[2] for w in want[:2]), "one query")
    sv, si = host(ix.search(vd.reshape(B * V, D_), 30))
    w = (0.5, 0.3, 0.2)
    want = fuse_ref.fuse_score(sv.reshape(B, V, 30), si.reshape(B, V, 30), np.asarray(w, np.float32), np.zeros(V, np.float32), 20)
    same(tt.fused_search(ix, vd, 20, fetch_k=30, method="score", weights=w, return_positions=True), want, "score")
    with pytest.raises(TypeError, match="unexpected"):
        tt.fused_search(ix, vd, 10, lam=0.5)
