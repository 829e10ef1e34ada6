"""Diversified selection (tt_mmr_select_f32 / _bf16 / _rows_f32, mmr_select, diverse_search), the parts that need no GPU: the
reference of tests/mmr_ref.py against the properties the rule promises, the planted-cluster property the feature exists for,
the argument checks of the C entry points (made before any HIP call) and the refusals of the Python surface."""
import ctypes as C

import numpy as np
import pytest
import torch

import mmr_ref
import synth

ENTRIES = ("tt_mmr_select_f32", "tt_mmr_select_bf16", "tt_mmr_select_rows_f32")
NEG_INF = np.float32(-np.inf)


@pytest.fixture(scope="module")
def libtt():
    from twotowermlretrieval_amd import build, _lib
    build.build()
    return _lib.lib()


# ---- the reference against itself

def _lists(seed, C_, n, d):
    rs = np.random.RandomState(seed)
    D = synth.unit_rows(seed, n, d)
    idx = rs.permutation(n)[:C_].astype(np.int64)
    vals = np.sort(rs.rand(C_).astype(np.float32))[::-1].copy()
    return D, vals, idx


def test_lambda_one_is_the_valid_prefix(oracle):
    D, vals, idx = _lists(1, 40, 500, 64)
    vals[[3, 17]], idx[[3, 9]] = [np.nan, np.inf], [-1, 500]      # invalid entries of every kind inside the list
    vals[20:24] = vals[20]                                        # a run of equal relevance keeps its list order
    ov, oi, op = mmr_ref.select(oracle, vals[None], idx[None], D, 12, 1.0)
    ok = np.flatnonzero(mmr_ref.valid_mask(vals[None], idx[None], 0, 500)[0])
    assert len(ok) == 37 and np.array_equal(op[0], ok[:12]) and np.array_equal(oi[0], idx[ok[:12]])
    assert np.array_equal(ov[0], vals[ok[:12]])


def test_gram_is_bitwise_symmetric(oracle):
    for d, bf16 in ((36, False), (256, False), (256, True)):
        X = synth.unit_rows(2 + d, 128, d) * np.float32(3.7)
        if bf16:
            X = (X.view(np.uint32) & np.uint32(0xffff0000)).view(np.float32)
        G = mmr_ref.gram(oracle, X)
        assert np.array_equal(G.view(np.uint32), G.T.view(np.uint32))


def test_a_twin_loses_to_anything_above_its_own_margin(oracle):
    """Candidates 0 and 1 are the same row with the same relevance.  After 0 is picked, 1 stands at a - mu |x|^2; candidate 2,
    less relevant but elsewhere, is above that and goes first -- by the rule alone, no id is compared."""
    d = 64
    X = synth.unit_rows(5, 3, d)
    X[1] = X[0]
    D = X.copy()
    vals = np.array([0.9, 0.9, 0.5], np.float32)
    for idx in (np.array([0, 1, 2], np.int64), np.array([0, 0, 2], np.int64)):   # a twin row, and the same id twice
        lam = np.float32(0.5)
        G = mmr_ref.gram(oracle, mmr_ref.candidate_rows(D, idx, np.ones(3, bool)))
        m_twin = lam * vals[1] - (np.float32(1) - lam) * G[1, 0]
        m_other = lam * vals[2] - (np.float32(1) - lam) * G[2, 0]
        assert G[1, 0] == G[0, 0] and m_other > m_twin
        ov, oi, op = mmr_ref.select(oracle, vals[None], idx[None], D, 3, 0.5)
        assert list(op[0]) == [0, 2, 1] and list(oi[0]) == [idx[0], 2, idx[1]] and list(ov[0]) == [vals[0], vals[2], vals[1]]
    # with relevance alone (lambda = 1) the twin keeps its place
    assert list(mmr_ref.select(oracle, vals[None], idx[None], D, 3, 1.0)[2][0]) == [0, 1, 2]


def test_short_lists_pad(oracle):
    D, vals, idx = _lists(3, 5, 100, 32)
    idx[2] = -1
    ov, oi, op = mmr_ref.select(oracle, vals[None], idx[None], D, 8, 0.3)
    assert sorted(op[0, :4]) == [0, 1, 3, 4] and (op[0, 4:] == -1).all() and (oi[0, 4:] == -1).all() and (ov[0, 4:] == NEG_INF).all()
    ov, oi, op = mmr_ref.select(oracle, vals[None, :0], idx[None, :0], D, 3, 0.3)        # C = 0
    assert (op == -1).all() and (oi == -1).all() and (ov == NEG_INF).all() and ov.shape == (1, 3)
    ov, oi, op = mmr_ref.select(oracle, vals[None], idx[None], D[:0], 3, 0.3)            # N = 0
    assert (op == -1).all() and (oi == -1).all()


# ---- what the feature is for

@pytest.mark.parametrize("seed", [0, 1, 2, 3, 4])
def test_planted_cluster_property(oracle, seed):
    """N = 20 000, d = 256, 8 queries, 40 near-duplicates per query of a row with cosine 0.9 to it: the plain top-10 is ten
    cluster members, the diversified top-10 out of the 64 best holds exactly one, at lambda = 0.5 and at 0.3."""
    D, Q, cluster = mmr_ref.planted_cluster(seed)
    v, i = oracle.score_topk(Q, D, 64)
    for b in range(len(Q)):
        assert np.isin(i[b, :10], cluster[b]).all()
    for lam in (0.5, 0.3):
        ov, oi, op = mmr_ref.select(oracle, v, i, D, 10, lam)
        for b in range(len(Q)):
            assert np.isin(oi[b], cluster[b]).sum() == 1 and oi[b, 0] == i[b, 0], (seed, lam, b)
            assert len(set(oi[b].tolist())) == 10 and (oi[b] >= 0).all()


# ---- the C entry points refuse before any HIP call

# aligned non-null addresses far apart: a call that fails its checks never reads them
IV, II, DP, OV, OI, OP = (C.c_void_p(a << 24) for a in range(1, 7))


def call(libtt, name, B=4, C_=64, d=256, N=1000, lam=0.5, k=10, in_val=IV, in_idx=II, D=DP, out_val=OV, out_idx=OI, out_pos=OP):
    if name.endswith("rows_f32"):
        return getattr(libtt, name)(in_val, in_idx, B, C_, D, d, lam, k, out_val, out_idx, out_pos, None)
    return getattr(libtt, name)(in_val, in_idx, B, C_, D, N, d, 0, lam, k, out_val, out_idx, out_pos, None)


@pytest.mark.parametrize("name", ENTRIES)
@pytest.mark.parametrize("kw,code,msg", [
    (dict(C_=129), "TT_ERR_UNSUPPORTED", "C=129"),
    (dict(k=0), "TT_ERR_UNSUPPORTED", "k=0"),
    (dict(k=129), "TT_ERR_UNSUPPORTED", "k=129"),
    (dict(d=6), "TT_ERR_UNSUPPORTED", "d=6"),
    (dict(d=520), "TT_ERR_UNSUPPORTED", "d=520"),
    (dict(d=0), "TT_ERR_UNSUPPORTED", "d=0"),
    (dict(lam=-0.1), "TT_ERR_BAD_SHAPE", "lambda=-0.1"),
    (dict(lam=1.5), "TT_ERR_BAD_SHAPE", "lambda=1.5"),
    (dict(lam=float("nan")), "TT_ERR_BAD_SHAPE", "nan"),
    (dict(lam=1.5, B=0), "TT_ERR_BAD_SHAPE", "lambda=1.5"),             # (judged before B = 0 returns)
    (dict(B=-1), "TT_ERR_BAD_SHAPE", "B=-1"),
    (dict(C_=-1), "TT_ERR_BAD_SHAPE", "C=-1"),
    (dict(in_val=None), "TT_ERR_BAD_SHAPE", "null pointer"),
    (dict(in_idx=None), "TT_ERR_BAD_SHAPE", "null pointer"),
    (dict(D=None), "TT_ERR_BAD_SHAPE", "null pointer"),
    (dict(out_val=None), "TT_ERR_BAD_SHAPE", "null pointer"),
    (dict(out_idx=None), "TT_ERR_BAD_SHAPE", "null pointer"),
    (dict(D=C.c_void_p((3 << 24) + 8)), "TT_ERR_BAD_SHAPE", "aligned"),
    (dict(in_idx=C.c_void_p((2 << 24) + 4)), "TT_ERR_BAD_SHAPE", "aligned"),
    (dict(out_pos=C.c_void_p((6 << 24) + 2)), "TT_ERR_BAD_SHAPE", "aligned"),
    (dict(out_val=IV), "TT_ERR_BAD_SHAPE", "overlap"),
    (dict(out_pos=OV), "TT_ERR_BAD_SHAPE", "overlap"),
])
def test_argument_validation_without_gpu(libtt, name, kw, code, msg):
    from twotowermlretrieval_amd import _lib
    assert call(libtt, name, **kw) == getattr(_lib, code)
    err = libtt.tt_last_error().decode()
    assert msg in err and name in err


def test_bf16_rows_need_a_multiple_of_eight_and_empty_calls_do_nothing(libtt):
    from twotowermlretrieval_amd import _lib
    assert call(libtt, "tt_mmr_select_bf16", d=36) == _lib.TT_ERR_UNSUPPORTED and "d=36" in libtt.tt_last_error().decode()
    assert call(libtt, "tt_mmr_select_f32", d=36, out_val=None) == _lib.TT_ERR_BAD_SHAPE                  # (f32 takes d = 36)
    assert call(libtt, "tt_mmr_select_f32", N=-1) == _lib.TT_ERR_BAD_SHAPE and "N=-1" in libtt.tt_last_error().decode()
    for name in ENTRIES:
        assert call(libtt, name, B=0) == _lib.TT_OK
        assert call(libtt, name, B=0, in_val=None, in_idx=None, D=None, out_val=None, out_idx=None, out_pos=None) == _lib.TT_OK


def test_symbols_are_declared_bound_and_exported(libtt):
    from conftest import ROOT
    from twotowermlretrieval_amd import _lib
    header = (ROOT / "include" / "tt.h").read_text()
    for name in ENTRIES:
        assert name in header and name in _lib.SIGNATURES and hasattr(libtt, name)


# ---- the Python surface

def test_public_surface_and_refusals():
    import inspect
    import twotowermlretrieval_amd as tt
    from twotowermlretrieval_amd import index
    assert tt.mmr_select is index.mmr_select and "mmr_select" in tt.__all__ and "mmr_select" in index.__all__
    assert list(inspect.signature(tt.mmr_select).parameters) == ["vals", "idx", "docs", "k", "lambda_", "idx_offset", "rows", "return_pos"]
    for cls in (tt.BruteForceIndex, tt.ShardedIndex, tt.StreamedIndex):
        p = inspect.signature(cls.diverse_search).parameters
        assert list(p) == ["self", "q", "k", "lambda_", "fetch_k", "keep", "exclude"]
        assert p["k"].default == 10 and p["lambda_"].default == 0.5 and p["fetch_k"].default is None
        assert "fetch_k" in cls.diverse_search.__doc__
    assert "4 bytes" in tt.ShardedIndex.diverse_search.__doc__ and "SYNCHRONIS" in tt.StreamedIndex.diverse_search.__doc__
    # fetch_k: by default min(128, 4 k); k <= fetch_k <= 128
    assert [index._mmr_fetch_k(k, None) for k in (1, 10, 32, 33, 128)] == [4, 40, 128, 128, 128]
    assert index._mmr_fetch_k(10, 10) == 10 and index._mmr_fetch_k(10, 128) == 128
    with pytest.raises(ValueError, match="fetch_k = 9 < k = 10"):
        index._mmr_fetch_k(10, 9)
    with pytest.raises(ValueError, match="fetch_k = 129"):
        index._mmr_fetch_k(10, 129)
    for k in (0, 129):
        with pytest.raises(ValueError, match=f"k = {k}"):
            index._mmr_fetch_k(k, None)
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="lambda_ must lie in"):
            index._check_lambda(bad)
    assert index._check_lambda(0) == 0.0 and index._check_lambda(1) == 1.0
    # no CPU fallback, in either form and for a single query
    vals, idx = torch.zeros(2, 8), torch.zeros((2, 8), dtype=torch.int64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tt.mmr_select(vals, idx, torch.zeros(10, 256), 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tt.mmr_select(vals, idx, None, 3, rows=torch.zeros(2, 8, 256))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tt.mmr_select(vals[0], idx[0], torch.zeros(10, 256), 3)
    with pytest.raises(ValueError, match="lambda_ must lie in"):
        tt.mmr_select(vals, idx, torch.zeros(10, 256), 3, lambda_=2.0)
    with pytest.raises(ValueError, match="docs or rows"):
        tt.mmr_select(vals, idx, None, 3)
    with pytest.raises(ValueError, match=r"takes idx \[C\]"):
        tt.mmr_select(vals[0], idx, torch.zeros(10, 256), 3)
