"""Candidate search (tt_score_ids_f32 / _bf16, score_ids, search(..., candidates=)), the parts that need no GPU: the exports,
the argument checks of the C entry points (made before any HIP call) and the checks of the Python surface."""
import ctypes as C

import pytest
import torch

ENTRIES = ("tt_score_ids_f32", "tt_score_ids_bf16")


@pytest.fixture(scope="module")
def libtt():
    from twotowermlretrieval_amd import build, _lib
    build.build()
    return _lib.lib()


def test_symbols_are_declared_bound_and_exported(libtt):
    from conftest import ROOT
    from twotowermlretrieval_amd import _lib
    header = (ROOT / "include" / "tt.h").read_text()
    for name in ENTRIES:
        assert name in header and name in _lib.SIGNATURES and hasattr(libtt, name)


# aligned non-null addresses far apart: a call that fails its checks never reads them
QP, DP, IDS, OV, OI, KEEP = (C.c_void_p(a << 24) for a in range(1, 7))


def call(libtt, name, B=4, d=256, N=1000, C_=100, Q=QP, D=DP, keep=None, ids=IDS, off=0, out_val=OV, out_idx=OI):
    return getattr(libtt, name)(Q, B, d, D, N, keep, ids, C_, off, out_val, out_idx, None)


@pytest.mark.parametrize("name", ENTRIES)
@pytest.mark.parametrize("kw,code,msg", [
    (dict(d=0), "TT_ERR_UNSUPPORTED", "d=0"),
    (dict(d=-8), "TT_ERR_UNSUPPORTED", "d=-8"),
    (dict(d=100 + 2), "TT_ERR_UNSUPPORTED", "d=102"),                   # no multiple of 4 (nor of 8)
    (dict(d=520), "TT_ERR_UNSUPPORTED", "d=520"),                       # a multiple of 8 beyond 512
    (dict(d=520, B=0), "TT_ERR_UNSUPPORTED", "d=520"),                  # (the shape is judged before B = 0 returns)
    (dict(B=-1), "TT_ERR_BAD_SHAPE", "B=-1"),
    (dict(C_=-1), "TT_ERR_BAD_SHAPE", "C=-1"),
    (dict(N=-1), "TT_ERR_BAD_SHAPE", "N=-1"),
    (dict(B=-1, d=7), "TT_ERR_BAD_SHAPE", "B=-1"),                      # negative sizes come first
    (dict(Q=None), "TT_ERR_BAD_SHAPE", "null pointer"),
    (dict(ids=None), "TT_ERR_BAD_SHAPE", "null pointer"),
    (dict(out_val=None), "TT_ERR_BAD_SHAPE", "null pointer"),
    (dict(D=None), "TT_ERR_BAD_SHAPE", "null pointer"),                 # N > 0 needs rows
    (dict(ids=C.c_void_p((3 << 24) + 4)), "TT_ERR_BAD_SHAPE", "aligned"),
    (dict(out_idx=C.c_void_p((5 << 24) + 4)), "TT_ERR_BAD_SHAPE", "aligned"),
    (dict(out_val=C.c_void_p((4 << 24) + 2)), "TT_ERR_BAD_SHAPE", "aligned"),
    (dict(keep=C.c_void_p((6 << 24) + 2)), "TT_ERR_BAD_SHAPE", "aligned"),
    (dict(Q=C.c_void_p((1 << 24) + 8)), "TT_ERR_BAD_SHAPE", "aligned"),
    (dict(D=C.c_void_p((2 << 24) + 8)), "TT_ERR_BAD_SHAPE", "aligned"),
    (dict(out_val=IDS), "TT_ERR_BAD_SHAPE", "overlap"),                 # out must not overlap in
    (dict(out_idx=C.c_void_p((3 << 24) + 8 * 399)), "TT_ERR_BAD_SHAPE", "overlap"),  # the last id
    (dict(out_val=C.c_void_p((1 << 24) + 4 * 1023)), "TT_ERR_BAD_SHAPE", "overlap"),  # the last element of Q
    (dict(out_idx=OV), "TT_ERR_BAD_SHAPE", "overlap"),                  # nor the other output
])
def test_argument_validation_without_gpu(libtt, name, kw, code, msg):
    from twotowermlretrieval_amd import _lib
    assert call(libtt, name, **kw) == getattr(_lib, code)
    err = libtt.tt_last_error().decode()
    assert msg in err and name in err


def test_bf16_rows_need_a_multiple_of_eight(libtt):
    from twotowermlretrieval_amd import _lib
    assert call(libtt, "tt_score_ids_bf16", d=132) == _lib.TT_ERR_UNSUPPORTED
    assert "d=132" in libtt.tt_last_error().decode()
    # (f32 takes d = 132: the call gets past the shape checks and is refused for the next thing wrong with it)
    assert call(libtt, "tt_score_ids_f32", d=132, Q=None) == _lib.TT_ERR_BAD_SHAPE
    assert "null pointer" in libtt.tt_last_error().decode()


@pytest.mark.parametrize("name", ENTRIES)
def test_empty_calls_do_nothing(libtt, name):
    from twotowermlretrieval_amd import _lib
    assert call(libtt, name, B=0) == _lib.TT_OK
    assert call(libtt, name, C_=0) == _lib.TT_OK
    assert call(libtt, name, B=0, Q=None, D=None, ids=None, out_val=None, out_idx=None) == _lib.TT_OK
    assert call(libtt, name, C_=0, N=0, Q=None, D=None, ids=None, out_val=None, out_idx=None) == _lib.TT_OK


def test_python_checks_of_the_lists():
    from twotowermlretrieval_amd import index
    cpu = torch.device("cpu")
    ids = torch.zeros((4, 5), dtype=torch.int64)
    assert index._check_ids(ids, 4, cpu) is ids
    assert index._check_ids(ids.t()[:4, :4], 4, cpu).is_contiguous()
    assert tuple(index._check_ids(ids[:, :0], 4, cpu).shape) == (4, 0)
    with pytest.raises(TypeError, match="int64"):
        index._check_ids(ids.to(torch.int32), 4, cpu)
    with pytest.raises(TypeError, match="int64"):
        index._check_ids([[1, 2]], 1, cpu)
    with pytest.raises(TypeError, match="candidates must be an int64"):
        index._check_ids(ids.float(), 4, cpu, "candidates")
    with pytest.raises(ValueError, match="runs on meta"):        # ids on another device
        index._check_ids(ids, 4, torch.device("meta"))
    with pytest.raises(ValueError, match=r"\[4,C\]"):            # [B',C] with B' != B
        index._check_ids(ids[:3], 4, cpu)
    with pytest.raises(ValueError, match=r"\[4,C\]"):
        index._check_ids(ids[0], 4, cpu)
    assert index._ids_row(None) is None and tuple(index._ids_row(ids[0]).shape) == (1, 5)
    with pytest.raises(ValueError, match=r"takes ids \[C\]"):    # a 1-D q with 2-D ids
        index._ids_row(ids)
    with pytest.raises(ValueError, match=r"takes candidates \[C\]"):
        index._ids_row(ids, "candidates")


def test_public_surface_and_cpu_refusal():
    import inspect
    import twotowermlretrieval_amd as tt
    assert tt.score_ids is tt.index.score_ids and "score_ids" in tt.__all__ and "score_ids" in tt.index.__all__
    for fn in (tt.BruteForceIndex.search, tt.ShardedIndex.search, tt.ShardedIndex.submit, tt.StreamedIndex.search):
        params = inspect.signature(fn).parameters
        assert params["candidates"].default is None and list(params)[-1] == "candidates"
    for cls in (tt.BruteForceIndex, tt.ShardedIndex, tt.StreamedIndex):
        assert list(inspect.signature(cls.score_ids).parameters)[:3] == ["self", "q", "ids"]
    assert "candidates" not in inspect.signature(tt.GraphedSearch.__call__).parameters
    assert inspect.signature(tt.HybridSearcher.__init__).parameters["lexical_candidates"].default == 0
    ids = torch.zeros((2, 3), dtype=torch.int64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tt.score_ids(torch.zeros(2, 256), torch.zeros(10, 256), ids)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tt.score_ids(torch.zeros(256), torch.zeros(10, 256), ids[0])
    with pytest.raises(ValueError, match=r"takes ids \[C\]"):    # (the squeeze is judged first: a 1-D q with 2-D ids)
        tt.score_ids(torch.zeros(256), torch.zeros(10, 256), ids)
