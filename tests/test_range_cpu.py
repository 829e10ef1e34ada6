"""Threshold search (tt_score_count_f32 / _bf16, tt_topk_cut_below, score_count, count / range_search of the indexes), the parts
that need no GPU: the exports, the argument checks of the C entry points (made before any HIP call), the workspace query and
the checks of the Python surface."""
import ctypes as C
import inspect

import pytest
import torch

NAMES = ("tt_score_count_workspace_bytes", "tt_score_count_f32", "tt_score_count_bf16", "tt_topk_cut_below")


@pytest.fixture(scope="module")
def libtt():
    from twotowermlretrieval_amd import build, _lib
    build.build()
    return _lib.lib()


def test_symbols_are_declared_bound_and_exported(libtt):
    from conftest import ROOT
    from twotowermlretrieval_amd import _lib
    header = (ROOT / "include" / "tt.h").read_text()
    for name in NAMES:
        assert name in header and name in _lib.SIGNATURES and hasattr(libtt, name), name
    assert "backend/evaluators.py:185-186" in header[header.index("Threshold search"):header.index("tt_score_count_workspace_bytes")]


P = C.c_void_p(4096)   # any aligned non-null address: a call that fails its checks never reads it
BIG = 1 << 40          # "enough workspace"


def count(libtt, fn="tt_score_count_f32", Q=P, B=4, d=256, D=P, N=1000, keep=None, min_score=P, count=P, accumulate=0, ws=P,
          ws_bytes=BIG):
    return getattr(libtt, fn)(Q, B, d, D, N, keep, min_score, count, accumulate, ws, ws_bytes, None)


@pytest.mark.parametrize("kw,code,msg", [
    (dict(B=-1), "TT_ERR_BAD_SHAPE", "B=-1"),
    (dict(N=-1), "TT_ERR_BAD_SHAPE", "N=-1"),
    (dict(Q=None), "TT_ERR_BAD_SHAPE", "null pointer"),
    (dict(D=None), "TT_ERR_BAD_SHAPE", "null pointer"),
    (dict(min_score=None), "TT_ERR_BAD_SHAPE", "null pointer"),
    (dict(count=None), "TT_ERR_BAD_SHAPE", "count"),
    (dict(count=None, N=0), "TT_ERR_BAD_SHAPE", "count"),                    # an empty corpus still writes count
    (dict(count=C.c_void_p(4100)), "TT_ERR_BAD_SHAPE", "8-byte aligned"),
    (dict(keep=C.c_void_p(4098)), "TT_ERR_BAD_SHAPE", "keep must be 4-byte aligned"),
    (dict(D=C.c_void_p(4100)), "TT_ERR_BAD_SHAPE", "aligned"),
    (dict(min_score=C.c_void_p(4098)), "TT_ERR_BAD_SHAPE", "aligned"),
    (dict(ws=C.c_void_p(4096 + 128)), "TT_ERR_BAD_SHAPE", "256-byte aligned"),
    (dict(d=100), "TT_ERR_UNSUPPORTED", "d=100 (supported: 32, 64, 96, 128, 192, 256, 320, 384, 448, 512)"),
    (dict(d=32, fn="tt_score_count_bf16"), "TT_ERR_UNSUPPORTED", "d=32 (supported: 64, 128, 192, 256)"),
    (dict(d=320, fn="tt_score_count_bf16"), "TT_ERR_UNSUPPORTED", "d=320"),
    (dict(N=(1 << 31) - 64), "TT_ERR_UNSUPPORTED", "N=2147483584 >= 2^31-64"),
    (dict(ws=None), "TT_ERR_WORKSPACE", "workspace"),
    (dict(ws_bytes=0), "TT_ERR_WORKSPACE", "workspace 0 <"),
    (dict(ws_bytes=255, fn="tt_score_count_bf16"), "TT_ERR_WORKSPACE", "workspace 255 <"),
])
def test_count_argument_validation_without_gpu(libtt, kw, code, msg):
    from twotowermlretrieval_amd import _lib
    assert count(libtt, **kw) == getattr(_lib, code)
    text = libtt.tt_last_error().decode()
    assert msg in text and kw.get("fn", "tt_score_count_f32") in text


def test_workspace_one_byte_short_is_refused(libtt):
    from twotowermlretrieval_amd import _lib
    for fn, bf16 in (("tt_score_count_f32", 0), ("tt_score_count_bf16", 1)):
        need = libtt.tt_score_count_workspace_bytes(4, 1000, 256, bf16)
        assert count(libtt, fn=fn, ws_bytes=need - 1) == _lib.TT_ERR_WORKSPACE


def test_b_zero_does_nothing(libtt):
    from twotowermlretrieval_amd import _lib
    for fn in ("tt_score_count_f32", "tt_score_count_bf16"):
        assert count(libtt, fn=fn, B=0) == _lib.TT_OK
        assert count(libtt, fn=fn, B=0, Q=None, D=None, min_score=None, count=None, ws=None, ws_bytes=0) == _lib.TT_OK


def test_workspace_query_needs_no_gpu(libtt):
    for bf16 in (0, 1):
        small = libtt.tt_score_count_workspace_bytes(32, 1_000_000, 256, bf16)
        large = libtt.tt_score_count_workspace_bytes(1024, 10_000_000, 256, bf16)
        assert 0 < small and 0 < large and small % 256 == 0 and large % 256 == 0
        # one int64 per (query, chunk) and the pacing slots: far below the search's candidate buffers
        assert large < libtt.tt_score_topk_workspace_bytes(1024, 10_000_000, 256, 10)
        assert libtt.tt_score_count_workspace_bytes(0, 10, 256, bf16) == 0
        assert libtt.tt_score_count_workspace_bytes(4, -1, 256, bf16) == 0
        assert libtt.tt_score_count_workspace_bytes(4, 0, 256, bf16) >= 0


def cut(libtt, val=P, idx=C.c_void_p(8192), B=4, k=10, min_score=C.c_void_p(1 << 20)):
    return libtt.tt_topk_cut_below(val, idx, B, k, min_score, None)


@pytest.mark.parametrize("kw,code,msg", [
    (dict(B=-1), "TT_ERR_BAD_SHAPE", "B=-1"),
    (dict(k=0), "TT_ERR_BAD_SHAPE", "k=0"),
    (dict(k=-2), "TT_ERR_BAD_SHAPE", "k=-2"),
    (dict(val=None), "TT_ERR_BAD_SHAPE", "null pointer"),
    (dict(idx=None), "TT_ERR_BAD_SHAPE", "null pointer"),
    (dict(min_score=None), "TT_ERR_BAD_SHAPE", "null pointer"),
    (dict(idx=C.c_void_p(8196)), "TT_ERR_BAD_SHAPE", "aligned"),
    (dict(val=C.c_void_p(4098)), "TT_ERR_BAD_SHAPE", "aligned"),
])
def test_cut_argument_validation_without_gpu(libtt, kw, code, msg):
    from twotowermlretrieval_amd import _lib
    assert cut(libtt, **kw) == getattr(_lib, code)
    assert msg in libtt.tt_last_error().decode()


def test_cut_b_zero_does_nothing(libtt):
    from twotowermlretrieval_amd import _lib
    assert cut(libtt, B=0) == _lib.TT_OK
    assert cut(libtt, B=0, val=None, idx=None, min_score=None) == _lib.TT_OK


def test_python_checks_of_min_score():
    from twotowermlretrieval_amd import index
    cpu = torch.device("cpu")
    t = torch.tensor([0.5, 0.25, 0.0, -1.0])
    assert index._min_score(t, 4, cpu) is t
    assert index._min_score(torch.arange(8, dtype=torch.float32)[::2], 4, cpu).is_contiguous()
    got = index._min_score(0.5, 3, cpu)
    assert got.dtype == torch.float32 and got.tolist() == [0.5, 0.5, 0.5]
    assert index._min_score(1, 2, cpu).tolist() == [1.0, 1.0]
    assert index._min_score(float("-inf"), 1, cpu).tolist() == [float("-inf")]
    assert tuple(index._min_score(torch.tensor(0.5), 1, cpu).shape) == (1,)      # a single query's 0-d threshold
    with pytest.raises(ValueError, match=r"\[B\] = \[4\]"):
        index._min_score(t[:3], 4, cpu)
    with pytest.raises(ValueError, match=r"\[B\] = \[4\]"):
        index._min_score(t.reshape(2, 2), 4, cpu)
    with pytest.raises(ValueError, match=r"\[B\] = \[4\]"):
        index._min_score(torch.tensor(0.5), 4, cpu)
    with pytest.raises(TypeError, match="float32"):
        index._min_score(t.double(), 4, cpu)
    with pytest.raises(TypeError, match="float32"):
        index._min_score(t.to(torch.int64), 4, cpu)
    with pytest.raises(TypeError, match="float"):
        index._min_score("0.5", 4, cpu)
    with pytest.raises(TypeError, match="float"):
        index._min_score(None, 4, cpu)
    with pytest.raises(TypeError, match="float"):
        index._min_score(True, 4, cpu)
    with pytest.raises(ValueError, match="runs on meta"):
        index._min_score(t, 4, torch.device("meta"))


def test_public_surface_and_exclude_refused():
    import twotowermlretrieval_amd as tt
    for name in ("score_count", "topk_cut_below"):
        assert getattr(tt, name) is getattr(tt.index, name) and name in tt.__all__ and name in tt.index.__all__
    for cls in (tt.BruteForceIndex, tt.ShardedIndex, tt.StreamedIndex):
        for fn in (cls.count, cls.range_search):
            params = inspect.signature(fn).parameters
            assert "exclude" not in params and params["keep"].default is None and "min_score" in params, fn
            with pytest.raises(TypeError, match="exclude"):                       # refused before anything is looked at
                fn(None, torch.zeros(2, 64), 0.5, exclude=torch.zeros((2, 1), dtype=torch.int64))
        assert inspect.signature(cls.range_search).parameters["k"].default == 10
        assert "EXACT kernel" in cls.range_search.__doc__                         # the cost is stated where the caller reads it
    with pytest.raises(TypeError, match="exclude"):
        tt.score_count(torch.zeros(2, 64), torch.zeros(10, 64), 0.5, exclude=torch.zeros((2, 1), dtype=torch.int64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tt.score_count(torch.zeros(2, 64), torch.zeros(10, 64), 0.5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tt.topk_cut_below(torch.zeros(2, 8), torch.zeros((2, 8), dtype=torch.int64), 0.5)


def test_sharded_constructors_still_forward_their_keywords():
    """The alternative constructors of ShardedIndex pass shard_k, screen, ... through to __init__."""
    import twotowermlretrieval_amd as tt
    for fn in (tt.ShardedIndex.from_global, tt.ShardedIndex.from_host_bf16, tt.ShardedIndex.from_documents):
        kinds = [p.kind for p in inspect.signature(fn).parameters.values()]
        assert inspect.Parameter.VAR_KEYWORD in kinds, fn
