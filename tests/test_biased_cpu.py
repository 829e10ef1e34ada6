"""CPU-side checks of biased search (tt_score_topk_biased_*, score_topk_biased, the indexes' biased_search, the L2 recipe): the
declarations, the size query, argument validation, the Python shims' refusals and the numpy reference's own semantics.  No GPU."""
import ctypes
import re

import numpy as np
import pytest
import torch

import biased_ref
from conftest import ROOT

NAMES = ("tt_score_topk_biased_workspace_bytes", "tt_score_topk_biased_f32", "tt_score_topk_biased_bf16")


@pytest.fixture(scope="module")
def libtt():
    from twotowermlretrieval_amd import build, _lib
    build.build()
    return _lib.lib()


def test_header_declares_the_calls_and_the_table_binds_them(libtt):
    from twotowermlretrieval_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "tt.h").read_text(), flags=re.S)
    for name in NAMES:
        assert re.search(rf"\b{name}\s*\(", header), name
        assert name in _lib.SIGNATURES and hasattr(libtt, name), name
    _vp, _i, _i64, _sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_size_t
    assert _lib.SIGNATURES[NAMES[0]] == (_sz, [_i, _i64, _i, _i, _i])
    call = (_i, [_vp, _i, _i, _vp, _i64, _vp, _vp, _i, _i64, _vp, _vp, _vp, _sz, _vp])
    assert _lib.SIGNATURES[NAMES[1]] == call and _lib.SIGNATURES[NAMES[2]] == call
    # the header states the idiom the call replaces
    text = (ROOT / "include" / "tt.h").read_text()
    assert "scores = torch.matmul(q, D.t()) + bias[None, :]; torch.topk(scores, k)" in text


@pytest.mark.parametrize("B,N,d,k,bf16", [(32, 1_000_000, 256, 10, 0), (5, 300_001, 512, 64, 0), (130, 70_000, 128, 1, 1),
                                          (1024, 10_000_000, 256, 10, 1), (3, 0, 64, 7, 0)])
def test_size_query(libtt, B, N, d, k, bf16):
    n = libtt.tt_score_topk_biased_workspace_bytes(B, N, d, k, bf16)
    assert n > 0 and n == libtt.tt_score_topk_masked_workspace_bytes(B, N, d, k, bf16)
    assert libtt.tt_score_topk_biased_workspace_bytes(0, N, d, k, bf16) == 0
    assert libtt.tt_score_topk_biased_workspace_bytes(B, N, d, 65, bf16) == 0


def test_argument_validation_without_gpu(libtt):
    from twotowermlretrieval_amd import _lib
    p = ctypes.c_void_p(16)
    t = ctypes.c_void_p(256)
    f32, bf16 = libtt.tt_score_topk_biased_f32, libtt.tt_score_topk_biased_bf16
    rc = f32(None, 4, 256, None, 10, t, None, 65, 0, p, p, None, 0, None)
    assert rc == _lib.TT_ERR_UNSUPPORTED and b"k=65" in libtt.tt_last_error()
    rc = bf16(None, 4, 256, None, 10, None, None, 65, 0, p, p, None, 0, None)              # also as the masked call
    assert rc == _lib.TT_ERR_UNSUPPORTED and b"k=65" in libtt.tt_last_error()
    rc = f32(None, 4, 100, None, 10, t, None, 5, 0, p, p, None, 0, None)
    assert rc == _lib.TT_ERR_UNSUPPORTED and b"d=100" in libtt.tt_last_error()
    rc = bf16(None, 4, 96, None, 10, t, None, 5, 0, p, p, None, 0, None)                   # the exact search's widths per dtype
    assert rc == _lib.TT_ERR_UNSUPPORTED and b"d=96" in libtt.tt_last_error()
    for addr in (258, 260, 264):                                                           # 16-byte alignment, not 4 or 8
        rc = f32(None, 4, 256, None, 10, ctypes.c_void_p(addr), None, 5, 0, p, p, None, 0, None)
        assert rc == _lib.TT_ERR_BAD_SHAPE and b"bias" in libtt.tt_last_error()
    rc = f32(None, 4, 256, None, 10, t, ctypes.c_void_p(18), 5, 0, p, p, None, 0, None)
    assert rc == _lib.TT_ERR_BAD_SHAPE and b"keep" in libtt.tt_last_error()
    rc = f32(None, 4, 256, None, -1, t, None, 5, 0, p, p, None, 0, None)
    assert rc == _lib.TT_ERR_BAD_SHAPE and b"N=-1" in libtt.tt_last_error()


def test_python_shims_refuse_cpu_tensors_and_wrong_arguments():
    import twotowermlretrieval_amd as tt
    from twotowermlretrieval_amd import index
    for name in ("score_topk_biased", "l2_bias", "l2_distances"):
        assert getattr(tt, name) is getattr(index, name)
        assert name in tt.__all__ and name in index.__all__
    q, D = torch.zeros(2, 256), torch.zeros(100, 256)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tt.score_topk_biased(q, D, torch.zeros(100), 5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tt.score_topk_biased(q[0], D, torch.zeros(128), 5)
    cpu = torch.device("cpu")
    padded = torch.arange(128, dtype=torch.float32)
    assert index._check_bias(padded, 100, cpu) is padded                       # already whole tiles: taken as it is
    got = index._check_bias(padded[:100], 100, cpu)                            # [N]: padded with zeros
    assert got.shape == (128,) and got.dtype == torch.float32
    assert torch.equal(got[:100], padded[:100]) and float(got[100:].abs().sum()) == 0.0
    assert index._check_bias(torch.zeros(0), 0, cpu).shape == (0,)
    for bad in (torch.zeros(99), torch.zeros(127), torch.zeros((100, 1))):
        with pytest.raises(ValueError, match="bias must hold"):
            index._check_bias(bad, 100, cpu)
    for bad in (torch.zeros(100, dtype=torch.float64), torch.zeros(100, dtype=torch.bfloat16), torch.zeros(100, dtype=torch.int32),
                [0.0] * 100, None):
        with pytest.raises(TypeError, match="float32"):
            index._check_bias(bad, 100, cpu)
    with pytest.raises(ValueError, match="live on"):
        index._check_bias(padded, 100, torch.device("cuda", 0))
    # set_bias checks finiteness once -- of the N values, not of the padding -- and None clears
    for cls, attrs in ((tt.BruteForceIndex, {"docs": D}), (tt.StreamedIndex, {"N": 100, "device": cpu})):
        ix = cls.__new__(cls)
        ix._bias = None
        for a, v in attrs.items():
            setattr(ix, a, v)
        assert ix.bias is None
        with pytest.raises(ValueError, match=r"no bias \(set_bias\)"):
            ix.biased_search(q, 5)
        with pytest.raises(ValueError, match=r"no bias \(set_bias\)"):         # before it looks at anything else
            ix.biased_search("not even a tensor", -3)
        for bad in (float("nan"), float("inf"), float("-inf")):
            b = torch.zeros(100)
            b[37] = bad
            with pytest.raises(ValueError, match="finite"):
                ix.set_bias(b)
            assert ix.bias is None
        ok = torch.zeros(128)
        ok[100:] = float("nan")                                                # the padding is the kernels' to ignore
        ix.set_bias(ok)
        assert ix.bias is ok
        if cls is tt.BruteForceIndex:                                          # out of scope, refused by name
            with pytest.raises(ValueError, match="candidates"):
                ix.biased_search(q, 5, candidates=torch.zeros((2, 1), dtype=torch.int64))
        ix.set_bias(None)
        assert ix.bias is None
    for cls in (tt.BruteForceIndex, tt.ShardedIndex, tt.StreamedIndex):
        assert callable(cls.set_bias) and callable(cls.biased_search) and isinstance(cls.bias, property)


def planted(seed, N, d, B):
    """Unit-scale rows with planted duplicates: rows 5, N // 2 and N - 1 are copies of one row, query 0 is that row."""
    rs = np.random.RandomState(seed)
    D = (rs.standard_normal((N, d)) / np.sqrt(d)).astype(np.float32)
    Q = (rs.standard_normal((B, d)) / np.sqrt(d)).astype(np.float32)
    D[[N // 2, N - 1]] = D[5]
    Q[0] = D[5] * np.float32(4.0)
    return Q, D


@pytest.mark.parametrize("d,N,B,k", [(256, 3001, 4, 64), (32, 1000, 3, 10), (512, 700, 2, 64)])
def test_reference_with_zero_bias_is_the_oracle(oracle, d, N, B, k):
    Q, D = planted(d + N, N, d, B)
    pats = biased_ref.bias_patterns(N, 3)
    ov, oi = oracle.score_topk(Q, D, k)
    assert oi[0, :3].tolist() == [5, N // 2, N - 1]                             # the planted tie, index ascending
    rv, ri = biased_ref.expected(oracle, Q, D, pats["zero"], k, np.arange(B))
    assert np.array_equal(ri, oi) and np.array_equal(rv, ov)
    cv, ci = biased_ref.expected(oracle, Q, D, pats["constant"], k, np.arange(B))
    assert np.array_equal(ci, oi) and np.array_equal(cv, (ov + np.float32(0.25)).astype(np.float32))
    for name in ("random", "lane_map", "alt_tiles", "ramp"):                    # the patterns are not vacuous
        _, bi = biased_ref.expected(oracle, Q, D, pats[name], k, np.arange(B))
        assert all(not np.array_equal(bi[b], oi[b]) for b in range(1, B)), name


def test_reference_patterns():
    N = 1000
    p = biased_ref.bias_patterns(N, 1)
    assert sorted(p) == ["absorbing", "alt_tiles", "constant", "lane_map", "ramp", "random", "spikes", "zero"]
    assert all(v.dtype == np.float32 and v.shape == (N,) and np.isfinite(v).all() for v in p.values())
    assert all(len(set(p["lane_map"][t:t + 32].tolist())) == 32 for t in range(0, N - 31, 32))
    assert p["alt_tiles"][:32].tolist() == [-1.0] * 32 and p["alt_tiles"][32:64].tolist() == [1.0] * 32
    assert np.flatnonzero(p["spikes"]).tolist() == [0, N - 1]
    assert 0 < int((p["absorbing"] == 0).sum()) < N // 20 and np.float32(0.7) + np.float32(-1e30) == np.float32(-1e30)


def test_reference_offset_keep_and_float64_order(oracle):
    rs = np.random.RandomState(0)
    N, d, B, k = 200, 32, 3, 5
    D = rs.standard_normal((N, d)).astype(np.float32)                           # well-separated scores
    Q = rs.standard_normal((B, d)).astype(np.float32)
    bias = rs.standard_normal(N).astype(np.float32)
    keep = rs.rand(N) < 0.5
    v, i = biased_ref.expected(oracle, Q, D, bias, k, [0, 2], keep=keep, idx_offset=1000)
    for out, b in enumerate((0, 2)):
        s = Q[b].astype(np.float64) @ D.T.astype(np.float64) + bias.astype(np.float64)
        s[~keep] = -np.inf
        order = np.argsort(-s, kind="stable")[:k]
        assert i[out].tolist() == (order + 1000).tolist()
        assert keep[i[out] - 1000].all() and np.abs(v[out] - s[order]).max() < 1e-5
    v, i = biased_ref.expected(oracle, Q, D, bias, 7, [1], keep=np.arange(N) < 3)
    assert sorted(i[0, :3].tolist()) == [0, 1, 2] and i[0, 3:].tolist() == [-1] * 4 and np.isneginf(v[0, 3:]).all()
    v, i = biased_ref.expected(oracle, Q, D[:0], bias[:0], 4, [0, 1])
    assert (i == -1).all() and np.isneginf(v).all()


def integer_rows(seed, n, d):
    return np.random.RandomState(seed).randint(-2, 3, size=(n, d)).astype(np.float32)


def test_l2_recipe_on_integer_valued_rows(oracle):
    """Entries in {-2..2}, d = 512: every product, partial sum, half sum of squares and biased score is a multiple of 1/2 below
    2^24, so float32 carries them exactly and the distances must equal float64 brute force with ==, ties included."""
    import twotowermlretrieval_amd as tt
    N, d, B, k = 5000, 512, 5, 64
    D, Q = integer_rows(1, N, d), integer_rows(2, B, d)
    bias = tt.l2_bias(torch.from_numpy(D))
    assert bias.dtype == torch.float32 and bias.shape == (N,)
    assert np.array_equal(bias.numpy().astype(np.float64), -0.5 * (D.astype(np.float64) ** 2).sum(1))
    assert torch.equal(tt.l2_bias(torch.from_numpy(D).to(torch.bfloat16)), bias)   # (small integers are bf16 values)
    v, i = biased_ref.expected(oracle, Q, D, bias.numpy(), k, np.arange(B))
    dist = tt.l2_distances(torch.from_numpy(Q), torch.from_numpy(v)).numpy()
    full = ((Q.astype(np.float64)[:, None, :] - D.astype(np.float64)[None, :, :]) ** 2).sum(-1)
    ties = 0
    for b in range(B):
        order = np.lexsort((np.arange(N), full[b]))[:k]
        assert i[b].tolist() == order.tolist()
        assert np.array_equal(dist[b].astype(np.float64), full[b][order])
        ties = max(ties, k - len(np.unique(full[b][order])))
    assert ties > 0                                                             # the case has ties among the first 64
    # the tail maps to +inf, a tiny negative rounding residue to 0, a single query works
    tail = tt.l2_distances(torch.ones(3), torch.tensor([1.5 + 1e-7, float("-inf")]))
    assert tail.tolist() == [0.0, float("inf")]
