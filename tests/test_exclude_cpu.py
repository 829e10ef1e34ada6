"""Per-query exclusion lists (tt_topk_exclude_ids, topk_exclude, search(..., exclude=)), the parts that need no GPU: the
export, the argument checks of the C entry point (made before any HIP call) and the checks of the Python surface."""
import ctypes as C

import pytest
import torch


@pytest.fixture(scope="module")
def libtt():
    from twotowermlretrieval_amd import build, _lib
    build.build()
    return _lib.lib()


def test_symbol_is_declared_bound_and_exported(libtt):
    from conftest import ROOT
    from twotowermlretrieval_amd import _lib
    assert "tt_topk_exclude_ids" in (ROOT / "include" / "tt.h").read_text()
    assert "tt_topk_exclude_ids" in _lib.SIGNATURES
    assert hasattr(libtt, "tt_topk_exclude_ids")


P = C.c_void_p(4096)   # any aligned non-null address: a call that fails its checks never reads it
Q = C.c_void_p(1 << 20)


def call(libtt, B=4, M=100, E=5, k=10, in_val=P, in_idx=P, exclude=P, out_val=Q, out_idx=Q):
    return libtt.tt_topk_exclude_ids(in_val, in_idx, B, M, exclude, E, k, out_val, out_idx, None)


@pytest.mark.parametrize("kw,code,msg", [
    (dict(k=101), "TT_ERR_BAD_SHAPE", "M=100 E=5 k=101"),                   # k > M
    (dict(k=0), "TT_ERR_BAD_SHAPE", "k=0"),
    (dict(k=-3), "TT_ERR_BAD_SHAPE", "k=-3"),
    (dict(E=-1), "TT_ERR_BAD_SHAPE", "E=-1"),
    (dict(B=-1), "TT_ERR_BAD_SHAPE", "B=-1"),
    (dict(M=-1, k=1), "TT_ERR_BAD_SHAPE", "M=-1"),
    (dict(E=1024, M=2000), "TT_ERR_UNSUPPORTED", "E=1024 > 1023"),
    (dict(E=1024, M=2000, B=0), "TT_ERR_UNSUPPORTED", "E=1024 > 1023"),     # (the shape is judged before B = 0 returns)
    (dict(in_val=None), "TT_ERR_BAD_SHAPE", "null pointer"),
    (dict(in_idx=None), "TT_ERR_BAD_SHAPE", "null pointer"),
    (dict(out_val=None), "TT_ERR_BAD_SHAPE", "null pointer"),
    (dict(out_idx=None), "TT_ERR_BAD_SHAPE", "null pointer"),
    (dict(exclude=None), "TT_ERR_BAD_SHAPE", "null pointer"),               # E > 0 needs a list
    (dict(exclude=C.c_void_p(4100)), "TT_ERR_BAD_SHAPE", "aligned"),
    (dict(out_val=P), "TT_ERR_BAD_SHAPE", "alias"),                         # out must not overlap in
    (dict(out_idx=C.c_void_p(4096 + 8 * 399)), "TT_ERR_BAD_SHAPE", "alias"),
])
def test_argument_validation_without_gpu(libtt, kw, code, msg):
    from twotowermlretrieval_amd import _lib
    assert call(libtt, **kw) == getattr(_lib, code)
    assert msg in libtt.tt_last_error().decode()


def test_b_zero_does_nothing(libtt):
    from twotowermlretrieval_amd import _lib
    assert call(libtt, B=0) == _lib.TT_OK
    assert call(libtt, B=0, E=1023, M=2000, in_val=None, in_idx=None, exclude=None, out_val=None, out_idx=None) == _lib.TT_OK


def test_python_checks_of_the_list():
    from twotowermlretrieval_amd import index
    cpu = torch.device("cpu")
    ex = torch.zeros((4, 5), dtype=torch.int64)
    got, kk = index._check_exclude(ex, 4, 10, cpu)
    assert got is ex and kk == 15
    assert index._check_exclude(ex.t()[:4, :4], 4, 10, cpu)[0].is_contiguous()
    assert index._check_exclude(torch.zeros((4, 1014), dtype=torch.int64), 4, 10, cpu)[1] == 1024
    with pytest.raises(ValueError, match=r"k \+ E = 10 \+ 1015 = 1025 > 1024"):
        index._check_exclude(torch.zeros((4, 1015), dtype=torch.int64), 4, 10, cpu)
    with pytest.raises(ValueError, match="int64"):
        index._check_exclude(ex.to(torch.int32), 4, 10, cpu)
    with pytest.raises(ValueError, match="int64"):
        index._check_exclude([[1, 2]], 1, 10, cpu)
    with pytest.raises(ValueError, match=r"\[4,E\]"):
        index._check_exclude(ex[:3], 4, 10, cpu)
    with pytest.raises(ValueError, match=r"\[4,E\]"):
        index._check_exclude(ex[0], 4, 10, cpu)
    with pytest.raises(ValueError, match="runs on meta"):
        index._check_exclude(ex, 4, 10, torch.device("meta"))
    with pytest.raises(ValueError, match="k = 0"):
        index._check_exclude(ex, 4, 0, cpu)
    assert index._exclude_row(None) is None and tuple(index._exclude_row(ex[0]).shape) == (1, 5)
    with pytest.raises(ValueError, match=r"takes exclude \[E\]"):
        index._exclude_row(ex)


def test_public_surface():
    import inspect
    import twotowermlretrieval_amd as tt
    assert tt.topk_exclude is tt.index.topk_exclude and "topk_exclude" in tt.__all__
    for fn in (tt.BruteForceIndex.search, tt.ShardedIndex.search, tt.ShardedIndex.submit, tt.StreamedIndex.search):
        assert inspect.signature(fn).parameters["exclude"].default is None
    assert inspect.signature(tt.GraphedSearch.__init__).parameters["exclude_width"].default == 0
    assert inspect.signature(tt.GraphedSearch.__call__).parameters["exclude"].default is None
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tt.topk_exclude(torch.zeros(2, 8), torch.zeros((2, 8), dtype=torch.int64), torch.zeros((2, 3), dtype=torch.int64), 4)
