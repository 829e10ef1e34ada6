"""Collapsed search on the GPU: the filter alone (tt_topk_collapse_table / _gids through topk_collapse), and collapsed_search on
the resident and the streamed index.

The expected value is the contract itself (collapse_ref: the literal walk), applied to the rows handed to the filter, or --
end to end -- to oracle.score_all over the whole corpus.  Nothing is computed on scores, so every comparison is equality."""
import numpy as np
import pytest
import torch

import collapse_ref
import synth
from poison import PATTERNS, pattern_id, poisoned_empty

pytestmark = pytest.mark.gpu

OFF = 1 << 40          # idx_offset of the table-form rows
I64_MIN = -(1 << 63)


@pytest.fixture(scope="module")
def tt():
    import twotowermlretrieval_amd as m
    from twotowermlretrieval_amd import _lib
    _lib.lib()
    assert torch.cuda.is_available()
    return m


@pytest.fixture(autouse=True)
def product_thresholds(monkeypatch):
    """The routing thresholds of the product (other test modules lower them for the rest of the session)."""
    from twotowermlretrieval_amd import index as _index
    monkeypatch.setattr(_index, "SCREEN_MIN_DOCS", 65536)
    monkeypatch.setattr(_index, "SCREEN_MIN_BATCH", 1)
    monkeypatch.setattr(_index, "SCREEN_PADDED_MIN_BATCH", 33)


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()   # (a copy: fixtures hand out read-only arrays)


def host(ts):
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in ts)


def same(got, want, what=""):
    """got: device tensors; want: numpy arrays, compared one by one for equality (shape and dtype included)."""
    for n, (g, w) in enumerate(zip(host(got), want)):
        assert g.shape == w.shape and g.dtype == w.dtype, (what, n, g.shape, w.shape, g.dtype, w.dtype)
        assert np.array_equal(g, w), (what, n, int((g != w).sum()))


# ---- the filter alone --------------------------------------------------------------------------------------------------------

def sorted_rows(seed, B, M, n_pad=0):
    """[B,M] rows as a search writes them: scores descending with runs of equal scores (index ascending inside a run),
    distinct ids per row from [0, 4M), the last n_pad entries padding."""
    rs = np.random.RandomState(seed)
    v = -np.sort(-rs.randint(0, max(M // 3, 2), size=(B, M)).astype(np.float32), axis=1)
    i = np.stack([rs.choice(4 * M, M, replace=False) for _ in range(B)]).astype(np.int64)
    for b in range(B):
        i[b] = i[b][np.lexsort((i[b], -v[b]))]
    if n_pad:
        v[:, M - n_pad:], i[:, M - n_pad:] = -np.inf, -1
    return v, i


def boundary_row(M, m, at=255):
    """gids [M], distinct but for one group whose m-th member sits at entry `at` and whose (m+1)-th at entry at + 1 (as far
    as the row reaches): the first is kept, the second is the first entry of the next 256-entry chunk, and dropped."""
    g = 1000 + np.arange(M, dtype=np.int64)
    members = [p for p in list(range(m - 1)) + [at, at + 1] if p < M]
    g[members] = 7
    return g


def entry_patterns(rs, B, M, m):
    """name -> gids [B,M], one id per entry."""
    p = np.arange(M, dtype=np.int64)
    big = (1 << 32) + (p % 3)
    big[p % 5 == 1] = p[p % 5 == 1] % 3          # 0, 1, 2 next to 2^32 + 0, 1, 2: ids that differ above bit 31 only
    big[p % 7 == 3] = I64_MIN
    out = {"distinct": np.stack([rs.permutation(M) for _ in range(B)]), "one_group": np.full((B, M), 7),
           "all_negative": -1 - rs.randint(0, 3, size=(B, M)), "alternating": np.tile(p % 2, (B, 1)),
           "boundary": np.tile(boundary_row(M, m), (B, 1)), "big": np.tile(big, (B, 1)),
           "few": rs.randint(-1, max(2, M // 8), size=(B, M))}
    return {k: np.ascontiguousarray(v, dtype=np.int64) for k, v in out.items()}


def tables(rs, n):
    """name -> groups [n]: the same patterns over the rows of a table."""
    r = np.arange(n, dtype=np.int64)
    big = (1 << 32) + (r % 3)
    big[r % 5 == 1] = r[r % 5 == 1] % 3
    big[r % 7 == 3] = I64_MIN
    out = {"distinct": rs.permutation(n), "one_group": np.full(n, 7), "all_negative": -1 - rs.randint(0, 3, size=n),
           "alternating": r % 2, "big": big, "few": rs.randint(-1, max(2, n // 32), size=n)}
    return {k: np.ascontiguousarray(v, dtype=np.int64) for k, v in out.items()}


@pytest.mark.parametrize("M", (1, 63, 64, 65, 255, 256, 257, 1024))
@pytest.mark.parametrize("B", (1, 33))
def test_filter_alone_gids_form(tt, B, M):
    """M crosses the wave and the 256-entry chunk; k = 1 and k = M; m = 1, 2, 3; rows with and without a padded tail."""
    rs = np.random.RandomState(100 * B + M)
    for n_pad in sorted({0, min(3, M - 1), M // 2}):
        v, i = sorted_rows(M + n_pad, B, M, n_pad)
        vd, id_ = dev(v), dev(i)
        for m in (1, 2, 3):
            for name, g in entry_patterns(rs, B, M, m).items():
                gd = dev(g)
                for k in sorted({1, M}):
                    want = collapse_ref.collapse(v, i, g, k, m)
                    same(tt.topk_collapse(vd, id_, k, gids=gd, max_per_group=m), want, (name, n_pad, m, k))
                    if name == "all_negative":
                        assert np.array_equal(want[1][:, :min(k, M - n_pad)], i[:, :min(k, M - n_pad)])      # nothing is collapsed
                    if name == "one_group":
                        assert (want[3][:, 0] == min(k, m, M - n_pad)).all()
                    if name == "boundary" and n_pad <= M - 257 and k == M:
                        assert (want[1] == i[:, 255:256]).any(1).all() and not (want[1] == i[:, 256:257]).any()


@pytest.mark.parametrize("M", (1, 63, 64, 65, 255, 256, 257, 1024))
@pytest.mark.parametrize("B", (1, 33))
def test_filter_alone_table_form(tt, B, M):
    """The same through the table: ids numbered from 2^40, the table shorter than the id range (ids beyond it, and ids below
    idx_offset, are ungrouped: the lookup is bounds-checked)."""
    rs = np.random.RandomState(200 * B + M)
    n_table = 3 * M                                   # ids run over [OFF, OFF + 4M): the last quarter lies beyond the table
    for n_pad in sorted({0, M // 2}):
        v, i = sorted_rows(3 * M + n_pad, B, M, n_pad)
        gi = np.where(i >= 0, i + OFF, i)
        below = (i >= 0) & (rs.rand(B, M) < 0.1)
        gi[below] = i[below]                          # ... and a few ids of "another shard", below idx_offset
        for b in range(B):                            # (still a sorted row: index ascending inside a run of equal scores)
            gi[b] = gi[b][np.lexsort((np.where(gi[b] < 0, np.iinfo(np.int64).max, gi[b]), -v[b].astype(np.float64)))]
        vd, id_ = dev(v), dev(gi)
        for name, table in tables(rs, n_table).items():
            g = collapse_ref.table_gids(gi, table, OFF)
            assert (g[(gi >= 0) & ((gi < OFF) | (gi >= OFF + n_table))] == -1).all()
            td = dev(table)
            for m in (1, 2, 3):
                for k in sorted({1, M}):
                    same(tt.topk_collapse(vd, id_, k, groups=td, max_per_group=m, idx_offset=OFF),
                         collapse_ref.collapse(v, gi, g, k, m), (name, n_pad, m, k))
        # an empty table: every entry is ungrouped
        same(tt.topk_collapse(vd, id_, M, groups=torch.zeros(0, dtype=torch.int64, device="cuda"), idx_offset=OFF),
             collapse_ref.collapse(v, gi, np.full(gi.shape, -1, np.int64), M, 1), "empty table")
    # the boundary pattern: one row's ids for every row, the table made from its entries
    v, i = sorted_rows(M, 1, M)
    for m in (1, 2, 3):
        table = np.full(4 * M, -1, np.int64)
        table[i[0]] = boundary_row(M, m)
        vv, ii = np.tile(v, (B, 1)), np.tile(i + OFF, (B, 1))
        same(tt.topk_collapse(dev(vv), dev(ii), M, groups=dev(table), max_per_group=m, idx_offset=OFF),
             collapse_ref.collapse(vv, ii, np.tile(boundary_row(M, m), (B, 1)), M, m), ("boundary", m))


def test_single_row_and_python_checks(tt):
    v, i = sorted_rows(3, 1, 40)
    g = entry_patterns(np.random.RandomState(1), 1, 40, 1)["few"]
    got = tt.topk_collapse(dev(v[0]), dev(i[0]), 10, gids=dev(g[0]))
    want = collapse_ref.collapse(v, i, g, 10, 1)
    same(got, tuple(w[0] for w in want))
    vd, id_, gd = dev(v), dev(i), dev(g)
    with pytest.raises(ValueError, match="k=41"):
        tt.topk_collapse(vd, id_, 41, gids=gd)
    with pytest.raises(ValueError, match="max_per_group=0"):
        tt.topk_collapse(vd, id_, 4, gids=gd, max_per_group=0)
    with pytest.raises(ValueError, match=r"\[1,40\]"):
        tt.topk_collapse(vd, id_, 4, gids=gd[:, :39])
    with pytest.raises(ValueError, match="int64"):
        tt.topk_collapse(vd, id_, 4, gids=gd.to(torch.int32))
    from twotowermlretrieval_amd import _lib
    wide = torch.zeros((1, 1025), device="cuda")
    with pytest.raises(_lib.TTError, match="M=1025"):
        tt.topk_collapse(wide, wide.to(torch.int64), 4, gids=wide.to(torch.int64))


@pytest.mark.parametrize("word", PATTERNS, ids=pattern_id)
def test_filter_into_out_and_poisoned_outputs(tt, word):
    """The result depends on the inputs only: whatever the outputs held (the caller's `out`, or fresh poisoned memory)."""
    v, i = sorted_rows(5, 33, 300, 20)
    g = entry_patterns(np.random.RandomState(6), 33, 300, 2)["few"]
    vd, id_, gd = dev(v), dev(i), dev(g)
    want = collapse_ref.collapse(v, i, g, 280, 2)
    assert (want[3][:, 0] < 280).any()                # short rows: a tail to write
    with poisoned_empty(word) as p:
        same(tt.topk_collapse(vd, id_, 280, gids=gd, max_per_group=2), want)
    assert p.tensors >= 4
    out = (torch.full((33, 280), 7.0, device="cuda"), torch.full((33, 280), 7, dtype=torch.int64, device="cuda"),
           torch.full((33, 280), 7, dtype=torch.int64, device="cuda"), torch.full((33, 2), 7, dtype=torch.int32, device="cuda"))
    got = tt.topk_collapse(vd, id_, 280, gids=gd, max_per_group=2, out=out)
    assert all(a is b for a, b in zip(got, out))
    same(got, want)


def test_filter_replays_in_a_graph_over_rewritten_inputs(tt):
    B, M, k, m = 8, 300, 40, 2
    v, i = sorted_rows(11, B, M)
    table = tables(np.random.RandomState(12), 4 * M)["few"]
    vd, id_, td = dev(v), dev(i + OFF), dev(table)
    out = tuple(torch.empty(s, dtype=t, device="cuda") for s, t in (((B, k), torch.float32), ((B, k), torch.int64),
                                                                      ((B, k), torch.int64), ((B, 2), torch.int32)))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        tt.topk_collapse(vd, id_, k, groups=td, max_per_group=m, idx_offset=OFF, out=out)        # (warm-up outside the capture)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        tt.topk_collapse(vd, id_, k, groups=td, max_per_group=m, idx_offset=OFF, out=out)
    for step in range(3):
        v2, i2 = sorted_rows(20 + step, B, M, 100 * step)
        t2 = tables(np.random.RandomState(30 + step), 4 * M)[("few", "alternating", "big")[step]]
        vd.copy_(dev(v2)), id_.copy_(dev(np.where(i2 >= 0, i2 + OFF, i2))), td.copy_(dev(t2))
        for o in out:
            o.fill_(9)
        graph.replay()
        gi2 = np.where(i2 >= 0, i2 + OFF, i2)
        same(out, collapse_ref.collapse(v2, gi2, collapse_ref.table_gids(gi2, t2, OFF), k, m), step)


# ---- collapsed_search against the contract over the oracle ------------------------------------------------------------------

N_SMALL, D_SMALL, B_SMALL = 3000, 64, 33


def page_groups(rs, n, pages):
    """groups [n]: `pages` pages at random, every 11th row ungrouped."""
    g = rs.randint(0, pages, size=n).astype(np.int64)
    g[::11] = -1 - (np.arange(n)[::11] % 2)
    return g


@pytest.fixture(scope="module")
def small(tt, oracle):
    """bf16 -> (rows on the device, queries [33,64], oracle.score_all [33,3000], groups [3000]); made once each."""
    made = {}

    def get(bf16):
        if bf16 not in made:
            D = torch.from_numpy(synth.unit_rows(61, N_SMALL, D_SMALL)).cuda()
            D = D.to(torch.bfloat16) if bf16 else D
            Q = synth.unit_rows(62, B_SMALL, D_SMALL)
            S = oracle.score_all(Q, np.ascontiguousarray(D.cpu().float().numpy()))
            S.setflags(write=False)
            g = page_groups(np.random.RandomState(63), N_SMALL, 25)
            g.setflags(write=False)
            made[bf16] = (D, torch.from_numpy(Q).cuda(), S, g)
        return made[bf16]

    return get


@pytest.mark.parametrize("bf16", (False, True), ids=("f32", "bf16"))
def test_collapsed_search_resident(tt, small, bf16):
    """25 pages over 3 000 rows and 273 ungrouped ones: k = 10 finishes in round 0 or 1, k = 30 exceeds the pages (ungrouped
    rows fill the rest), k = 200 needs more ungrouped rows than the best 1 024 hold: masked rounds."""
    D, Q, S, g = small(bf16)
    ix = tt.BruteForceIndex(D)
    with pytest.raises(ValueError, match="no groups"):
        ix.collapsed_search(Q, 10)
    ix.set_groups(dev(g))
    assert torch.equal(ix.groups, dev(g))
    masked = 0
    for k, m in ((10, 1), (10, 3), (30, 1), (1, 1), (100, 2), (200, 1)):
        got = ix.collapsed_search(Q, k, m)
        same(got[:3], collapse_ref.search(S, g, k, m), (k, m))
        assert bool((got[3] == 1).all()) and got[3].dtype == torch.int32
        masked += ix.collapse_rounds[1]
    assert masked > 0
    one = ix.collapsed_search(Q[4], 10, 3)                                     # a single query [d]
    want = collapse_ref.search(S[4:5], g, 10, 3)
    same(one[:3], tuple(w[0] for w in want))
    assert one[3].dim() == 0 and int(one[3]) == 1
    # exact=False: one round, no continuation; a complete row is the answer, an incomplete one its exact prefix
    v, i, gg, complete = ix.collapsed_search(Q, 40, 1, exact=False)
    assert ix.collapse_rounds == (1, 0)
    want = collapse_ref.search(S, g, 40, 1)
    v, i, gg, complete = host((v, i, gg, complete))
    assert (complete == 0).any()                                               # 64 fetched rows of 25 pages do not hold 40 to keep
    for b in range(B_SMALL):
        n = 40 if complete[b] else int((i[b] >= 0).sum())
        assert np.array_equal(i[b, :n], want[1][b, :n]) and np.array_equal(v[b, :n], want[0][b, :n])
        assert complete[b] or (i[b, n:] == -1).all()
    with pytest.raises(ValueError, match="512"):
        ix.collapsed_search(Q, 513)
    with pytest.raises(ValueError, match=r"fetch_k \+ E"):
        ix.collapsed_search(Q, 10, fetch_k=1020, exclude=torch.zeros((B_SMALL, 5), dtype=torch.int64, device="cuda"))
    with pytest.raises(ValueError, match="max_per_group"):
        ix.collapsed_search(Q, 10, 0)
    ix.set_groups(None)
    assert ix.groups is None


def test_collapsed_search_composes(tt, small):
    """keep=, remove_ids, exclude= and idx_offset together: the eligible rows are what is left of all three."""
    D, Q, S, g = small(False)
    off = 1 << 33
    ix = tt.BruteForceIndex(D, idx_offset=off)
    ix.set_groups(dev(g))
    rs = np.random.RandomState(9)
    order = np.argsort(-S, axis=1, kind="stable")
    removed = np.unique(order[:, 0])                                            # every query's best row is withdrawn
    ix.remove_ids(dev(removed + off))
    keep = rs.rand(N_SMALL) < 0.7
    ex = order[:, 1:6].copy()                                                   # ... its next five excluded for it alone
    el = np.tile(keep, (B_SMALL, 1))
    el[:, removed] = False
    np.put_along_axis(el, ex, False, axis=1)
    kd, exd = tt.pack_keep_mask(dev(keep)), dev(ex + off)
    for k, m in ((10, 1), (30, 2)):
        got = ix.collapsed_search(Q, k, m, keep=kd, exclude=exd)
        same(got[:3], collapse_ref.search(S, g, k, m, el, off), (k, m))
        assert bool((got[3] == 1).all())
    got = ix.collapsed_search(Q[2], 10, 1, keep=kd, exclude=exd[2])
    same(got[:3], tuple(w[0] for w in collapse_ref.search(S[2:3], g, 10, 1, el[2:3], off)))


def test_tie_group_is_cut_in_index_order(tt, oracle):
    """Six copies of one row on one page, tied at the top: max_per_group = 2 keeps the two lowest ids, in that order; and a
    corpus with fewer than k groups fills the tail."""
    D = synth.unit_rows(71, 512, D_SMALL).copy()
    Q = synth.unit_rows(72, 4, D_SMALL).copy()
    twins = np.array([300, 17, 450, 18, 101, 99])
    D[twins] = Q[0]
    g = np.arange(512, dtype=np.int64) % 5                                      # five pages, nobody ungrouped
    g[twins] = 3
    S = oracle.score_all(Q, D)
    ix = tt.BruteForceIndex(dev(D))
    ix.set_groups(dev(g))
    got = ix.collapsed_search(dev(Q), 10, 2)
    want = collapse_ref.search(S, g, 10, 2)
    same(got[:3], want)
    assert want[1][0, :2].tolist() == [17, 18] and (want[1][:, :10] >= 0).all()
    got = ix.collapsed_search(dev(Q), 12, 2)                                    # 5 pages x 2 = 10 rows exist
    want = collapse_ref.search(S, g, 12, 2)
    same(got[:3], want)
    assert (want[1][:, 10:] == -1).all() and bool((got[3] == 1).all())
    tiny = tt.BruteForceIndex(dev(D[:6]))                                       # a corpus smaller than k
    tiny.set_groups(dev(g[:6]))
    same(tiny.collapsed_search(dev(Q), 10, 1)[:3], collapse_ref.search(S[:, :6], g[:6], 10, 1))


def test_screened_index(tt, oracle):
    """65 536 x 256 (the smallest corpus that screens): round 0 for k = 10 fetches 40 rows through the screen."""
    from test_search_aux_gpu import par_rows
    g_ = torch.Generator(device="cuda").manual_seed(77)
    D = torch.randn((65536, 256), device="cuda", generator=g_).div_(16.0)
    Q = torch.from_numpy(synth.unit_rows(78, B_SMALL, 256)).cuda()
    Dh = D.cpu().numpy()
    S = par_rows(lambda q: oracle.score_all(q, Dh), Q.cpu().numpy())
    g = page_groups(np.random.RandomState(79), 65536, 400)
    ix = tt.BruteForceIndex(D, screen=True)
    ix.set_groups(dev(g))
    assert ix._screens(B_SMALL, 40)
    ix.fallback_flags = None
    got = ix.collapsed_search(Q, 10, 1)
    assert ix.fallback_flags is not None                                        # the screened search ran
    same(got[:3], collapse_ref.search(S, g, 10, 1))
    same(ix.collapsed_search(Q, 20, 2)[:3], collapse_ref.search(S, g, 20, 2))
    del ix, D
    torch.cuda.empty_cache()


# ---- the planted case ---------------------------------------------------------------------------------------------------------

def test_planted_page_owns_the_head(tt, oracle):
    D, Q, g, where = collapse_ref.planted()
    S = oracle.score_all(Q, D)
    ix = tt.BruteForceIndex(dev(D))
    ix.set_groups(dev(g))
    Qd = dev(Q)
    pv, pi = host(ix.search(Qd, 10))
    assert np.isin(pi[0], where).all()                                          # the plain top-10: ten passages of one page
    assert set(np.argsort(-S[0], kind="stable")[:1100].tolist()) == set(where.tolist())       # ... which owns 1 100 places
    v, i, gg, complete = host(ix.collapsed_search(Qd, 10, 1, exact=False))
    assert complete.tolist() == [0, 1, 1] and ix.collapse_rounds == (1, 0)
    assert i[0, 0] == pi[0, 0] and (i[0, 1:] == -1).all()                       # the exact prefix, and it says so
    for m in (1, 3):
        got = ix.collapsed_search(Qd, 10, m)
        want = collapse_ref.search(S, g, 10, m)
        same(got[:3], want, m)
        assert bool((got[3] == 1).all()) and ix.collapse_rounds[0] == 2 and ix.collapse_rounds[1] >= 1
        assert (want[2][0] == 5).sum() == m and (want[1][0] >= 0).all()


def test_streamed_index_over_three_blocks(tt, oracle):
    D, Q, g, where = collapse_ref.planted()
    Db = torch.from_numpy(D).to(torch.bfloat16)
    S = oracle.score_all(Q, np.ascontiguousarray(Db.float().numpy()))
    off = 1 << 20
    ix = tt.StreamedIndex(Db, block_docs=1408, idx_offset=off)                 # 4096 rows = 1408 + 1408 + 1280, whole words each
    with pytest.raises(ValueError, match="no groups"):
        ix.collapsed_search(dev(Q), 10)
    ix.set_groups(dev(g))
    assert ix.groups.is_cuda
    for k, m, exact in ((10, 1, True), (10, 2, True), (10, 1, False)):
        got = ix.collapsed_search(dev(Q), k, m, exact=exact)
        want = collapse_ref.search(S, g, k, m, None, off)
        if exact:
            same(got[:3], want, (k, m))
            assert ix.collapse_rounds[1] >= 1
        else:
            i, complete = host((got[1], got[3]))
            assert complete.tolist() == [0, 1, 1] and np.array_equal(i[1:], want[1][1:]) and i[0, 0] == want[1][0, 0]
