"""Diversified selection on the GPU: tt_mmr_select_f32 / _bf16 / _rows_f32 and what is built on them (mmr_select,
diverse_search of the resident and the streamed index) against tests/mmr_ref.py -- the rule of include/tt.h in numpy float32
over the oracle's Gram.  Every comparison is equality of values, indices and positions: there are no tolerances."""
import numpy as np
import pytest
import torch

import mmr_ref
import synth
from poison import CONTROL, PATTERNS, pattern_id, poisoned_empty

pytestmark = pytest.mark.gpu

N = 3000
KMAX = 128
NEG_INF = np.float32(-np.inf)
LAMBDAS = (0.0, 0.3, 0.5, 1.0)
CS = (1, 2, 31, 32, 33, 63, 64, 65, 96, 127, 128)


def to_bf16(x):
    """fp32 -> the bf16 grid (truncation), still fp32: the exactly widened rows the oracle scores."""
    return (x.view(np.uint32) & np.uint32(0xffff0000)).view(np.float32)


def dev_rows(D, bf16):
    t = torch.from_numpy(D).cuda()
    return t.to(torch.bfloat16) if bf16 else t  # (exact: the rows are on the bf16 grid already)


_ROWS = {}


def corpus(d, bf16, n=N):
    """D [n,d] fp32 (on the bf16 grid when bf16), made once and never changed."""
    key = (d, bf16, n)
    if key not in _ROWS:
        D = synth.unit_rows(500 + d, n, d)
        _ROWS[key] = to_bf16(D) if bf16 else D
    return _ROWS[key]


def sorted_list(rs, C, off, n=N):
    """What a search writes: distinct ids, relevance descending."""
    idx = off + rs.permutation(n)[:C].astype(np.int64)
    vals = np.sort((rs.rand(C) * 1.5 - 0.25).astype(np.float32))[::-1].copy()
    return vals, idx


def mixed_list(rs, C, off, n=N):
    """Runs of equal relevance, repeated ids, interleaved (-inf, -1) padding, ids that are not the corpus's (below the offset,
    at off + n, at 2^40 beyond it, negative, the int64 edge) and valid ids under a relevance that is not finite."""
    idx = off + rs.randint(0, n, size=C).astype(np.int64)
    vals = np.sort((np.round(rs.rand(C) * 6) / 6).astype(np.float32))[::-1].copy()
    for p in rs.permutation(C)[:C // 6]:                           # repeats
        idx[p] = idx[rs.randint(0, C)]
    pad = rs.rand(C) < 0.15
    vals[pad], idx[pad] = NEG_INF, -1
    special = [off - 1, off + n, off + n + 2 ** 40, -5, np.iinfo(np.int64).max, off, off + n - 1]
    for j, p in enumerate(rs.permutation(C)[:min(C // 3, len(special))]):
        idx[p] = special[j]
        vals[p] = np.float32(0.75)
    for j, p in enumerate(rs.permutation(C)[:min(C // 8, 3)]):
        vals[p] = (np.float32(np.nan), np.float32(np.inf), NEG_INF)[j]
    return vals, idx


def batch(rs, B, C, off, n=N):
    """Row 0 a sorted search output; then mixed lists; row 3 all invalid."""
    rows = [sorted_list(rs, C, off, n) if b == 0 else mixed_list(rs, C, off, n) for b in range(B)]
    vals, idx = np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows])
    if B > 3:
        idx[3] = np.where(np.arange(C) % 2 == 0, -1, off + n + np.arange(C))
    return vals, idx


def expected(oracle, vals, idx, D, off, ks, lams):
    """{(k, lam): (out_val, out_idx, out_pos)}.  The picks for k are the first k picks of a longer run, and the Gram does
    not depend on k or lambda: one Gram per query, one greedy run per lambda."""
    ok = mmr_ref.valid_mask(vals, idx, off, D.shape[0])
    grams = [mmr_ref.gram(oracle, mmr_ref.candidate_rows(D, idx[b], ok[b], off)) for b in range(len(vals))]
    out = {}
    for lam in lams:
        picks = [mmr_ref.greedy(vals[b], ok[b], grams[b], max(ks), lam) for b in range(len(vals))]
        for k in ks:
            rows = [mmr_ref.outputs(vals[b], idx[b], picks[b][:k], k) for b in range(len(vals))]
            out[(k, lam)] = tuple(np.stack([r[j] for r in rows]) for j in range(3))
    return out


def host(t):
    return t.cpu().numpy()


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def same(got, want):
    """(values, indices, positions), bit for bit (NaN never appears in an output: a NaN relevance is never selected)."""
    return all(np.array_equal(host(g), w) for g, w in zip(got, want))


@pytest.mark.parametrize("d,bf16", [(4, False), (36, False), (256, False), (512, False), (8, True), (40, True), (256, True), (512, True)])
def test_grid_against_the_reference(oracle, d, bf16):
    """Every C around the tile and instantiation edges (32, 64, 128), B in {1, 5}, k in {1, min(C, 10), C, C + 3} (held to
    the limit k <= 128, which C + 3 passes at C >= 126) and four lambdas, in one upload of the rows."""
    import twotowermlretrieval_amd as tt
    D = corpus(d, bf16)
    docs = dev_rows(D, bf16)
    rs = np.random.RandomState(7 * d + bf16)
    padded = 0
    for C in CS:
        ks = sorted({1, min(C, 10), C, min(C + 3, KMAX)})
        for B in (1, 5):
            vals, idx = batch(rs, B, C, 0)
            want = expected(oracle, vals, idx, D, 0, ks, LAMBDAS)
            vd, idd = dev(vals), dev(idx)
            for (k, lam), w in want.items():
                got = tt.mmr_select(vd, idd, docs, k, lam, return_pos=True)
                assert same(got, w), (C, B, k, lam)
                padded += int((w[2] == -1).any())
            if C >= 31:   # the list is not simply returned in order
                assert any((np.diff(want[(C, lam)][2][0]) < 0).any() for lam in (0.0, 0.3)), C
    assert padded > 20
    v1 = tt.mmr_select(vd[0], idd[0], docs, 10, 0.3, return_pos=True)       # one query: [C] lists
    assert all(t.dim() == 1 for t in v1) and same(v1, [x[0] for x in want[(10, 0.3)]])
    assert len(tt.mmr_select(vd, idd, docs, 10, 0.3)) == 2


@pytest.mark.parametrize("d,bf16", [(36, False), (40, True)])
def test_list_patterns_offsets_and_empty_corpus(oracle, d, bf16):
    import twotowermlretrieval_amd as tt
    D = corpus(d, bf16)
    docs = dev_rows(D, bf16)
    rs = np.random.RandomState(d)
    for off in (1000, 2 ** 33 + 5, -40):
        vals, idx = batch(rs, 5, 70, off)
        if off > 0:
            idx[2, :6] = [off - 1, 0, off - 2 ** 40, off + N, off + N - 1, off]   # ids below the offset count as foreign
        want = expected(oracle, vals, idx, D, off, (12, 73), (0.3,))
        ok = mmr_ref.valid_mask(vals, idx, off, N)
        assert not ok[3].any() and ok[2].any() and (idx[~ok] >= 0).any()
        for (k, lam), w in want.items():
            assert same(tt.mmr_select(dev(vals), dev(idx), docs, k, lam, idx_offset=off, return_pos=True), w), (off, k)
        assert (want[(12, 0.3)][1][3] == -1).all() and (want[(73, 0.3)][1][:, 70:] == -1).all()
        if off > 0:                                      # (at a negative offset some of row 0's ids are negative: invalid)
            assert (want[(73, 0.3)][1][0, :70] >= 0).all()
    # N = 0: every candidate is foreign; C = 0: nothing to select from; B = 0
    got = tt.mmr_select(dev(vals), dev(idx), docs[:0], 7, 0.5, return_pos=True)
    assert bool(torch.isneginf(got[0]).all()) and bool((got[1] == -1).all()) and bool((got[2] == -1).all())
    got = tt.mmr_select(dev(vals[:, :0]), dev(idx[:, :0]), docs, 7, 0.5, return_pos=True)
    assert tuple(got[0].shape) == (5, 7) and bool(torch.isneginf(got[0]).all()) and bool((got[1] == -1).all()) and bool((got[2] == -1).all())
    got = tt.mmr_select(dev(vals[:0]), dev(idx[:0]), docs, 7, 0.5, return_pos=True)
    assert [tuple(t.shape) for t in got] == [(0, 7)] * 3


def test_more_workgroups_than_compute_units(oracle):
    import twotowermlretrieval_amd as tt
    B, C, d, k = 700, 40, 32, 5
    D = corpus(d, False)
    rs = np.random.RandomState(70)
    vals, idx = batch(rs, B, C, 0)
    want = expected(oracle, vals, idx, D, 0, (k,), (0.4,))[(k, 0.4)]
    assert same(tt.mmr_select(dev(vals), dev(idx), dev_rows(D, False), k, 0.4, return_pos=True), want)


@pytest.mark.parametrize("bf16", [False, True])
def test_rows_form_equals_corpus_form(bf16):
    """The candidates' rows gathered beforehand (widened exactly from bf16): the same picks bit for bit; an entry whose id is
    not the corpus's is made invalid for the rows form by what a search would have written for it, (-inf, -1)."""
    import twotowermlretrieval_amd as tt
    d = 40
    D = corpus(d, bf16)
    docs = dev_rows(D, bf16)
    rs = np.random.RandomState(8)
    for C, k in ((20, 6), (64, 64), (100, 17), (128, 128)):
        vals, idx = batch(rs, 5, C, 0)
        ok = mmr_ref.valid_mask(vals, idx, 0, N)
        vals[~ok], idx[~ok] = NEG_INF, -1
        rows = np.stack([mmr_ref.candidate_rows(D, idx[b], ok[b]) for b in range(5)])
        rows[~ok] = 12345.0                              # never read: an invalid entry's row is arbitrary
        for lam in (0.2, 0.7):
            a = tt.mmr_select(dev(vals), dev(idx), docs, k, lam, return_pos=True)
            b = tt.mmr_select(dev(vals), dev(idx), None, k, lam, rows=dev(rows), return_pos=True)
            assert all(torch.equal(x, y) for x, y in zip(a, b)), (C, lam)
    one = tt.mmr_select(dev(vals[1]), dev(idx[1]), None, 9, 0.7, rows=dev(rows[1]), return_pos=True)   # [C] with rows [C,d]
    assert all(torch.equal(x, y[1, :9]) for x, y in zip(one, tt.mmr_select(dev(vals), dev(idx), docs, 9, 0.7, return_pos=True)))


def test_out_pos_is_consistent_with_out_idx():
    import twotowermlretrieval_amd as tt
    D = corpus(256, False)
    rs = np.random.RandomState(9)
    vals, idx = batch(rs, 5, 90, 0)
    ok = mmr_ref.valid_mask(vals, idx, 0, N)
    v, i, p = (host(t) for t in tt.mmr_select(dev(vals), dev(idx), dev_rows(D, False), 100, 0.5, return_pos=True))
    for b in range(5):
        n = int(ok[b].sum())
        assert sorted(p[b, :n]) == list(np.flatnonzero(ok[b])) and (p[b, n:] == -1).all()     # every valid position once
        assert np.array_equal(i[b, :n], idx[b][p[b, :n]]) and np.array_equal(v[b, :n], vals[b][p[b, :n]])
        assert (i[b, n:] == -1).all() and (v[b, n:] == NEG_INF).all()


@pytest.mark.parametrize("word", PATTERNS, ids=pattern_id)
def test_outputs_do_not_depend_on_what_the_buffers_held(oracle, word):
    import twotowermlretrieval_amd as tt
    D = corpus(36, False)
    docs = dev_rows(D, False)
    rs = np.random.RandomState(10)
    vals, idx = batch(rs, 5, 33, 0)
    want = expected(oracle, vals, idx, D, 0, (40,), (0.5,))[(40, 0.5)]
    vd, idd = dev(vals), dev(idx)
    with poisoned_empty(word) as p:
        got = tt.mmr_select(vd, idd, docs, 40, 0.5, return_pos=True)
        rows_form = tt.mmr_select(vd[:1], idd[:1], None, 40, 0.5, rows=docs[idd[:1]].contiguous(), return_pos=True)
    assert p.tensors >= 6
    assert same(got, want) and same(rows_form, [w[:1] for w in want])


def test_graph_replay_over_rewritten_inputs(oracle):
    import twotowermlretrieval_amd as tt
    D = corpus(256, True)
    docs = dev_rows(D, True)
    rs = np.random.RandomState(11)
    lists = [batch(rs, 5, 128, 0) for _ in range(2)]
    want = [expected(oracle, v, i, D, 0, (10,), (0.5,))[(10, 0.5)] for v, i in lists]
    vd, idd = dev(lists[0][0]), dev(lists[0][1])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                          # warm-up outside capture: kernels loaded, blocks cached
        tt.mmr_select(vd, idd, docs, 10, 0.5, return_pos=True)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = tt.mmr_select(vd, idd, docs, 10, 0.5, return_pos=True)
    for n in (0, 1, 0):
        vd.copy_(dev(lists[n][0]))
        idd.copy_(dev(lists[n][1]))
        for t in out:
            t.fill_(7)
        graph.replay()
        torch.cuda.synchronize()
        assert same(out, want[n]), n


_CLUSTER = {}


def cluster_case(oracle):
    """The planted-cluster corpus at a size that screens (70 000 rows), on the bf16 grid so that one reference serves the
    fp32, the screened and the bf16 layout; the oracle's top-64 and the reference's picks."""
    if not _CLUSTER:
        D, Q, cluster = mmr_ref.planted_cluster(0, n=70_000)
        D = to_bf16(D)
        v, i = oracle.score_topk(Q, D, 64)
        _CLUSTER.update(D=D, Q=Q, cluster=cluster, top=(v, i),
                        want={lam: mmr_ref.select(oracle, v, i, D, 10, lam) for lam in (0.5, 0.3)})
    return _CLUSTER


@pytest.mark.parametrize("layout", ["f32", "screened", "bf16"])
def test_planted_cluster_through_diverse_search(oracle, layout):
    """The plain top-10 is ten members of the query's cluster of near-duplicates; diverse_search returns exactly one."""
    import twotowermlretrieval_amd as tt
    c = cluster_case(oracle)
    D, cluster = torch.from_numpy(c["D"]).cuda(), c["cluster"]
    ix = tt.BruteForceIndex(D.to(torch.bfloat16)) if layout == "bf16" else tt.BruteForceIndex(D, screen=layout == "screened")
    Qd = torch.from_numpy(c["Q"]).cuda()
    if layout == "screened":
        assert ix._screens(len(Qd), 64)
    pv, pi = ix.search(Qd, 10)
    assert all(np.isin(host(pi)[b], cluster[b]).all() for b in range(len(Qd)))
    for lam in (0.5, 0.3):
        v, i = ix.diverse_search(Qd, 10, lam, fetch_k=64)
        assert np.array_equal(host(i), c["want"][lam][1]) and np.array_equal(host(v), c["want"][lam][0]), lam
        assert all(np.isin(host(i)[b], cluster[b]).sum() == 1 for b in range(len(Qd)))
    # lambda = 1 is the plain search; the default fetch_k is min(128, 4 k); one query [d]
    v1, i1 = ix.diverse_search(Qd, 10, 1.0)
    assert torch.equal(i1, pi) and torch.equal(v1, pv)
    fv, fi = ix.search(Qd, 40)
    want = mmr_ref.select(oracle, host(fv), host(fi), c["D"], 10, 0.5)
    v, i = ix.diverse_search(Qd, 10)
    assert np.array_equal(host(i), want[1]) and np.array_equal(host(v), want[0])
    vq, iq = ix.diverse_search(Qd[2], 10)
    assert vq.dim() == 1 and torch.equal(iq, i[2]) and torch.equal(vq, v[2])
    # keep= and exclude= are the search's
    gone = i[:, 0].contiguous()
    ve, ie = ix.diverse_search(Qd, 10, exclude=gone.unsqueeze(1))
    assert not bool((ie == gone.unsqueeze(1)).any()) and bool((ie >= 0).all())
    with pytest.raises(ValueError, match="fetch_k"):
        ix.diverse_search(Qd, 10, fetch_k=5)
    with pytest.raises(ValueError, match="fetch_k"):
        ix.diverse_search(Qd, 10, fetch_k=200)


def test_streamed_index_agrees_with_the_resident_one(oracle):
    import twotowermlretrieval_amd as tt
    d, off = 256, 1000
    D = corpus(d, True)
    host_rows = torch.from_numpy(D).to(torch.bfloat16)
    st = tt.StreamedIndex(host_rows, block_docs=1024, idx_offset=off)
    res = tt.BruteForceIndex(host_rows.cuda(), idx_offset=off)
    Qd = torch.from_numpy(synth.unit_rows(12, 6, d)).cuda()
    Qd[1] = torch.from_numpy(D[77]).cuda()                    # a query that is a document
    for k, lam, fk in ((10, 0.5, None), (5, 0.2, 128), (128, 0.7, 128)):
        a, b = st.diverse_search(Qd, k, lam, fetch_k=fk), res.diverse_search(Qd, k, lam, fetch_k=fk)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), (k, lam)
    fv, fi = res.search(Qd, 40)
    want = mmr_ref.select(oracle, host(fv), host(fi), D, 10, 0.5, off)
    v, i = st.diverse_search(Qd, 10)
    assert np.array_equal(host(i), want[1]) and np.array_equal(host(v), want[0])
    vq, iq = st.diverse_search(Qd[1], 10)
    assert torch.equal(iq, i[1]) and torch.equal(vq, v[1])
    st.remove_ids(i[:, 0])
    res.remove_ids(i[:, 0])
    a, b = st.diverse_search(Qd, 10), res.diverse_search(Qd, 10)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and not bool(torch.isin(a[1], i[:, 0]).any())


def test_rows_beyond_2_to_31_and_2_to_32_elements(oracle):
    """A 16.8M x 256 fp32 corpus (17.2 GB, never initialised) with the candidates' rows planted around element offsets 2^31
    (row 2^23) and 2^32 (row 2^24) and at both ends; only planted rows are named, so no background is needed."""
    import twotowermlretrieval_amd as tt
    n, d, B, C = 16_800_000, 256, 3, 50
    rs = np.random.RandomState(13)
    planted = np.unique(np.concatenate([[0, n - 1, 2 ** 23 - 1, 2 ** 23, 2 ** 23 + 1, 2 ** 24 - 1, 2 ** 24, 2 ** 24 + 1],
                                        rs.randint(2 ** 23, n, size=40), rs.randint(2 ** 24, n, size=12)])).astype(np.int64)
    rows = synth.unit_rows(14, len(planted), d)
    docs = torch.empty((n, d), dtype=torch.float32, device="cuda")
    docs[torch.from_numpy(planted).cuda()] = torch.from_numpy(rows).cuda()
    assert (planted * d >= 2 ** 31).sum() > 30 and (planted * d >= 2 ** 32).sum() > 10
    for off in (0, 2 ** 33 + 5):
        where = np.stack([rs.permutation(len(planted))[:C] for _ in range(B)])      # positions among the planted rows
        vals = np.sort(rs.rand(B, C).astype(np.float32), axis=1)[:, ::-1].copy()
        idx = off + planted[where]
        idx[:, 7] = off + n                                                         # one past the last row
        small = np.where(idx == off + n, off + len(planted), off + where)           # the same lists over the planted rows alone
        want = mmr_ref.select(oracle, vals, small, rows, 20, 0.5, off)
        v, i, p = tt.mmr_select(dev(vals), dev(idx), docs, 20, 0.5, idx_offset=off, return_pos=True)
        assert np.array_equal(host(p), want[2]) and np.array_equal(host(v), want[0])
        assert np.array_equal(host(i), np.take_along_axis(idx, want[2].astype(np.int64), 1))
        assert (host(p) != 7).all() and (host(i) - off >= 2 ** 24).any()
