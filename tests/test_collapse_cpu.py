"""Collapsed search (tt_topk_collapse_table / _gids, topk_collapse, collapsed_search), the parts that need no GPU: the rule
against its parallel form, the prefix certificate, the argument checks of the C entries (made before any HIP call), the
rounds of the exact search over numpy-backed stand-ins, and the default fetch_k."""
import ctypes as C

import numpy as np
import pytest
import torch

import collapse_ref


@pytest.fixture(scope="module")
def libtt():
    from twotowermlretrieval_amd import build, _lib
    build.build()
    return _lib.lib()


def _random_row(rs, M):
    """One sorted row's (idx, gids): distinct ids, a padded tail now and then, few groups so that they repeat, some ungrouped."""
    idx = rs.permutation(4 * M)[:M].astype(np.int64)
    if rs.rand() < 0.5:
        idx[M - rs.randint(0, M // 2 + 1):] = -1
    gids = rs.randint(-2, max(2, M // 4), size=M).astype(np.int64)
    return idx, gids


def test_walk_equals_parallel_form():
    rs = np.random.RandomState(5)
    for M in (1, 2, 7, 64, 65, 300):
        for m in (1, 2, 3):
            for _ in range(8):
                idx, gids = _random_row(rs, M)
                assert collapse_ref.walk(idx, gids, m) == collapse_ref.parallel(idx, gids, m)


def test_prefix_certificate():
    """The rule on the top-F of a row is the beginning of the rule on the whole row, for every F; and where the filter says
    complete -- k kept, or the prefix ends in padding -- it is the whole row's answer."""
    rs = np.random.RandomState(6)
    for M, m, k in ((40, 1, 5), (40, 2, 8), (97, 3, 10)):
        idx, gids = _random_row(rs, M)
        vals = -np.arange(M, dtype=np.float32)
        whole = collapse_ref.walk(idx, gids, m)
        full = collapse_ref.collapse_row(vals, idx, gids, k, m)
        for F in range(1, M + 1):
            assert collapse_ref.walk(idx[:F], gids[:F], m) == [p for p in whole if p < F]
            if F >= k:
                ov, oi, og, (kept, complete) = collapse_ref.collapse_row(vals[:F], idx[:F], gids[:F], k, m)
                assert np.array_equal(oi[:kept], full[1][:kept]) and np.array_equal(ov[:kept], full[0][:kept])
                if complete:
                    assert np.array_equal(oi, full[1]) and np.array_equal(og, full[2])


def test_symbols_are_declared_bound_and_exported(libtt):
    from conftest import ROOT
    from twotowermlretrieval_amd import _lib
    for name in ("tt_topk_collapse_table", "tt_topk_collapse_gids"):
        assert name in (ROOT / "include" / "tt.h").read_text() and name in _lib.SIGNATURES and hasattr(libtt, name)


P = C.c_void_p(1 << 20)   # aligned non-null addresses, far apart: a call that fails its checks never reads them
G = C.c_void_p(2 << 20)
OV, OI, OG, INFO = (C.c_void_p(n << 20) for n in (3, 4, 5, 6))


def call(libtt, form, B=4, M=100, N=1000, off=0, m=1, k=10, in_val=P, in_idx=P, src=G, out_val=OV, out_idx=OI, out_gid=OG, info=INFO):
    if form == "table":
        return libtt.tt_topk_collapse_table(in_val, in_idx, B, M, src, N, off, m, k, out_val, out_idx, out_gid, info, None)
    return libtt.tt_topk_collapse_gids(in_val, in_idx, src, B, M, m, k, out_val, out_idx, out_gid, info, None)


@pytest.mark.parametrize("form", ["table", "gids"])
@pytest.mark.parametrize("kw,code,msg", [
    (dict(k=101), "TT_ERR_BAD_SHAPE", "k=101"),                             # k > M
    (dict(k=0), "TT_ERR_BAD_SHAPE", "k=0"),
    (dict(M=1025, k=10), "TT_ERR_UNSUPPORTED", "M=1025 > 1024"),
    (dict(M=1025, k=10, B=0), "TT_ERR_UNSUPPORTED", "M=1025 > 1024"),       # (the shape is judged before B = 0 returns)
    (dict(m=0), "TT_ERR_BAD_SHAPE", "max_per_group=0"),
    (dict(m=-2), "TT_ERR_BAD_SHAPE", "max_per_group=-2"),
    (dict(B=-1), "TT_ERR_BAD_SHAPE", "B=-1"),
    (dict(in_val=None), "TT_ERR_BAD_SHAPE", "null pointer"),
    (dict(in_idx=None), "TT_ERR_BAD_SHAPE", "null pointer"),
    (dict(src=None), "TT_ERR_BAD_SHAPE", "null pointer"),
    (dict(out_val=None), "TT_ERR_BAD_SHAPE", "null pointer"),
    (dict(out_idx=None), "TT_ERR_BAD_SHAPE", "null pointer"),
    (dict(out_gid=None), "TT_ERR_BAD_SHAPE", "null pointer"),
    (dict(info=None), "TT_ERR_BAD_SHAPE", "null pointer"),
    (dict(in_val=C.c_void_p((1 << 20) + 2)), "TT_ERR_BAD_SHAPE", "aligned"),
    (dict(in_idx=C.c_void_p((1 << 20) + 4)), "TT_ERR_BAD_SHAPE", "aligned"),
    (dict(src=C.c_void_p((2 << 20) + 4)), "TT_ERR_BAD_SHAPE", "aligned"),
    (dict(out_gid=C.c_void_p((5 << 20) + 4)), "TT_ERR_BAD_SHAPE", "aligned"),
    (dict(info=C.c_void_p((6 << 20) + 2)), "TT_ERR_BAD_SHAPE", "aligned"),
    (dict(out_val=P), "TT_ERR_BAD_SHAPE", "alias"),                         # out must not overlap in
    (dict(out_idx=C.c_void_p((1 << 20) + 8 * 399)), "TT_ERR_BAD_SHAPE", "alias"),
    (dict(out_gid=P), "TT_ERR_BAD_SHAPE", "alias"),
    (dict(out_gid=G), "TT_ERR_BAD_SHAPE", "alias"),                         # the table / the rows' ids are inputs too
])
def test_argument_validation_without_gpu(libtt, form, kw, code, msg):
    from twotowermlretrieval_amd import _lib
    assert call(libtt, form, **kw) == getattr(_lib, code)
    err = libtt.tt_last_error().decode()
    assert msg in err and f"tt_topk_collapse_{form}" in err


def test_table_form_checks_of_its_own(libtt):
    from twotowermlretrieval_amd import _lib
    assert call(libtt, "table", N=-1) == _lib.TT_ERR_BAD_SHAPE and "N=-1" in libtt.tt_last_error().decode()


@pytest.mark.parametrize("form", ["table", "gids"])
def test_b_zero_does_nothing(libtt, form):
    from twotowermlretrieval_amd import _lib
    assert call(libtt, form, B=0) == _lib.TT_OK
    assert call(libtt, form, B=0, in_val=None, in_idx=None, src=None, out_val=None, out_idx=None, out_gid=None, info=None) == _lib.TT_OK


# ---- the rounds of the exact search, over stand-ins -----------------------------------------------------------------------

N_ROUNDS = 6_000


def _rounds_corpus():
    """Three queries over 6 000 rows: group 0 owns rows [0, 3000), group 1 rows [3000, 4500), the rest is one group per row
    with every 9th row ungrouped.  Query 0 ranks the rows by number (group 0 owns its best 3 000, group 1 the next 1 500), query
    1 at random, query 2 like query 0 in tie groups of 7."""
    n = np.arange(N_ROUNDS)
    groups = np.where(n < 3000, 0, np.where(n < 4500, 1, 10 + n)).astype(np.int64)
    groups[4500::9] = -1
    rs = np.random.RandomState(8)
    scores = np.stack([1.0 - n / N_ROUNDS, rs.rand(N_ROUNDS), 1.0 - (n // 7) / N_ROUNDS]).astype(np.float32)
    return scores, groups


class _Standins:
    """search / filter / mask of an index, in numpy over the corpus above (tensors in and out, on the host)."""

    def __init__(self, scores, groups, exclude, k, m):
        self.scores, self.groups, self.exclude, self.k, self.m = scores, groups, exclude, k, m
        self.calls = []  # (queries, kk, masked) of every search

    def eligible(self, b):
        el = np.ones(N_ROUNDS, bool)
        el[self.exclude[b]] = False
        return el

    def search(self, rows, kk, keep):
        rows = list(range(len(self.scores))) if rows is None else rows.tolist()
        self.calls.append((rows, kk, keep is not None))
        assert kk + self.exclude.shape[1] <= 1024
        vals, idx = np.full((len(rows), kk), -np.inf, np.float32), np.full((len(rows), kk), -1, np.int64)
        for r, b in enumerate(rows):
            v, i = collapse_ref.sorted_row(self.scores[b], self.eligible(b) & (True if keep is None else keep))
            n = min(kk, len(i))
            vals[r, :n], idx[r, :n] = v[:n], i[:n]
        return torch.from_numpy(vals), torch.from_numpy(idx)

    def collapse(self, v, i):
        v, i = v.numpy(), i.numpy()
        assert v.shape[1] <= 1024 and (np.diff(v, axis=1) <= 0).all()      # a sorted row the filter can take
        ov, oi, og, info = collapse_ref.collapse(v, i, collapse_ref.table_gids(i, self.groups), self.k, self.m)
        return tuple(torch.from_numpy(x) for x in (ov, oi, og, info))

    def mask(self, saturated, selected):
        keep = ~np.isin(self.groups, saturated.numpy())
        keep[selected.numpy()] = False
        return keep


@pytest.mark.parametrize("E", [0, 5])
@pytest.mark.parametrize("k,m", [(10, 1), (10, 3), (512, 1)])
def test_rounds_equal_the_rule_on_the_whole_row(k, m, E):
    from twotowermlretrieval_amd import index
    scores, groups = _rounds_corpus()
    exclude = np.stack([np.array([0, 1, 3000, 4500, 4501])[:E], np.arange(E), np.array([6, 7, 8, 4502, 5999])[:E]]).astype(np.int64)
    s = _Standins(scores, groups, exclude, k, m)
    fk = index._collapse_fetch_k(k, N_ROUNDS, None, E)
    stats = {}
    ov, oi, og, complete = index._collapse_rounds(s.search, s.collapse, s.mask, m, fk, E, N_ROUNDS, True, stats)
    el = np.stack([s.eligible(b) for b in range(3)])
    wv, wi, wg = collapse_ref.search(scores, groups, k, m, el)
    assert np.array_equal(oi.numpy(), wi) and np.array_equal(ov.numpy(), wv) and np.array_equal(og.numpy(), wg)
    assert complete.tolist() == [1, 1, 1]
    masked = [c for c in s.calls if c[2]]
    assert len(masked) >= 1 and stats["masked_rounds"] == len(masked)       # query 0 cannot finish without a masked round
    assert all(len(c[0]) == 1 for c in masked)                              # ... which every query runs alone
    assert s.calls[0] == ([0, 1, 2], fk, False)
    if fk < 1024 - E:   # round 1: the incomplete queries as one batch at full width, nothing masked
        assert s.calls[1][1] == 1024 - E and not s.calls[1][2] and 0 in s.calls[1][0] and stats["batched_rounds"] == 2
    else:               # (round 0 was that wide already)
        assert s.calls[1][2] and stats["batched_rounds"] == 1
    assert len(s.calls) <= 2 + 3 * 4                                        # it terminates, in a handful of rounds


def test_one_round_without_exact():
    from twotowermlretrieval_amd import index
    scores, groups = _rounds_corpus()
    s = _Standins(scores, groups, np.zeros((3, 0), np.int64), 10, 1)
    ov, oi, og, complete = index._collapse_rounds(s.search, s.collapse, s.mask, 1, 40, 0, N_ROUNDS, False)
    assert len(s.calls) == 1 and complete[0] == 0
    wi = collapse_ref.search(scores, groups, 10, 1)[1]
    assert oi[0, 0] == wi[0, 0] == 0 and (oi[0, 1:] == -1).all()            # the exact prefix: group 0's best row, then the tail
    for b in range(3):                                                       # a complete row is the answer
        if complete[b]:
            assert np.array_equal(oi[b].numpy(), wi[b])
    # a fetch of the whole corpus is complete whatever its tail
    s = _Standins(scores[:, :], groups, np.zeros((3, 0), np.int64), 10, 1)
    assert index._collapse_rounds(s.search, s.collapse, s.mask, 1, 40, 0, 40, False)[3].tolist() == [1, 1, 1]


def test_default_fetch_k():
    from twotowermlretrieval_amd import index
    f = index._collapse_fetch_k
    big = 10_000_000
    assert [f(k, big) for k in (1, 5, 10, 16, 17, 40, 64)] == [4, 20, 40, 64, 64, 64, 64]     # never across the k = 64 cliff
    assert [f(k, big) for k in (65, 100, 512, 600, 1024)] == [130, 200, 1024, 1024, 1024]
    assert f(10, 25) == 25 and f(100, 150) == 150 and f(10, None) == 40                         # min(ntotal, ...)
    assert f(10, big, 33) == 33 and f(10, big, 10) == 10 and f(10, big, 1024) == 1024
    assert f(512, big, None, 5) == 1019                                                         # the default gives way to E
    with pytest.raises(ValueError, match="fetch_k >= k"):
        f(10, big, 9)
    with pytest.raises(ValueError, match=r"fetch_k \+ E = 1020 \+ 5 = 1025 > 1024"):
        f(10, big, 1020, 5)
    with pytest.raises(ValueError, match="k = 0"):
        f(0, big)


def test_public_surface():
    import inspect
    import twotowermlretrieval_amd as tt
    assert tt.topk_collapse is tt.index.topk_collapse and "topk_collapse" in tt.__all__
    for cls in (tt.BruteForceIndex, tt.ShardedIndex, tt.StreamedIndex):
        p = inspect.signature(cls.collapsed_search).parameters
        assert [p[n].default for n in ("k", "max_per_group", "fetch_k", "keep", "exclude", "exact")] == [10, 1, None, None, None, True]
        assert "SYNCHRONISES" in cls.collapsed_search.__doc__ and isinstance(cls.groups, property) and callable(cls.set_groups)
    assert not hasattr(tt.GraphedSearch, "collapsed_search")
    v, i = torch.zeros(2, 8), torch.zeros((2, 8), dtype=torch.int64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tt.topk_collapse(v, i, 4, groups=torch.zeros(8, dtype=torch.int64))
    with pytest.raises(ValueError, match="exactly one"):
        tt.topk_collapse(v, i, 4)
    with pytest.raises(ValueError, match="exactly one"):
        tt.topk_collapse(v, i, 4, groups=i[0], gids=i)
