"""CPU-side checks of tagged search (tt_score_topk_tagged_*, score_topk_tagged, the indexes' tagged_search): the declarations,
the size query, argument validation, the Python shims' refusals and the numpy reference's own semantics.  No GPU, no compute."""
import ctypes
import re

import numpy as np
import pytest
import torch

import tagged_ref
from conftest import ROOT

NAMES = ("tt_score_topk_tagged_workspace_bytes", "tt_score_topk_tagged_f32", "tt_score_topk_tagged_bf16")


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
    call = (_i, [_vp, _i, _i, _vp, _i64, _vp, _vp, _vp, _vp, _i, _i64, _vp, _vp, _vp, _sz, _vp])
    assert _lib.SIGNATURES[NAMES[1]] == call and _lib.SIGNATURES[NAMES[2]] == call
    # the header states the idiom the call replaces
    text = (ROOT / "include" / "tt.h").read_text()
    assert "scores[b, ~elig[b]] = -inf" in text and "backend/evaluators.py:185-186" in text


@pytest.mark.parametrize("B,N,d,k,bf16", [(32, 1_000_000, 256, 10, 0), (5, 300_001, 512, 64, 0), (130, 70_000, 128, 1, 1),
                                          (1024, 10_000_000, 256, 10, 1), (3, 0, 64, 7, 0)])
def test_size_query(libtt, B, N, d, k, bf16):
    n = libtt.tt_score_topk_tagged_workspace_bytes(B, N, d, k, bf16)
    assert n > 0 and n == libtt.tt_score_topk_masked_workspace_bytes(B, N, d, k, bf16)
    assert libtt.tt_score_topk_tagged_workspace_bytes(0, N, d, k, bf16) == 0
    assert libtt.tt_score_topk_tagged_workspace_bytes(B, N, d, 65, bf16) == 0


def test_argument_validation_without_gpu(libtt):
    from twotowermlretrieval_amd import _lib
    p = ctypes.c_void_p(16)
    t = ctypes.c_void_p(256)
    f32, bf16 = libtt.tt_score_topk_tagged_f32, libtt.tt_score_topk_tagged_bf16
    rc = f32(None, 4, 256, None, 10, t, p, p, None, 65, 0, p, p, None, 0, None)
    assert rc == _lib.TT_ERR_UNSUPPORTED and b"k=65" in libtt.tt_last_error()
    rc = bf16(None, 4, 256, None, 10, None, None, None, None, 65, 0, p, p, None, 0, None)   # also as the masked call
    assert rc == _lib.TT_ERR_UNSUPPORTED and b"k=65" in libtt.tt_last_error()
    rc = f32(None, 4, 100, None, 10, t, p, p, None, 5, 0, p, p, None, 0, None)
    assert rc == _lib.TT_ERR_UNSUPPORTED and b"d=100" in libtt.tt_last_error()
    rc = bf16(None, 4, 96, None, 10, t, p, p, None, 5, 0, p, p, None, 0, None)             # the exact search's widths per dtype
    assert rc == _lib.TT_ERR_UNSUPPORTED and b"d=96" in libtt.tt_last_error()
    rc = f32(None, 4, 256, None, 10, ctypes.c_void_p(258), p, p, None, 5, 0, p, p, None, 0, None)
    assert rc == _lib.TT_ERR_BAD_SHAPE and b"tags" in libtt.tt_last_error()
    rc = f32(None, 4, 256, None, 10, t, ctypes.c_void_p(18), p, None, 5, 0, p, p, None, 0, None)
    assert rc == _lib.TT_ERR_BAD_SHAPE and b"match_mask" in libtt.tt_last_error()
    rc = f32(None, 4, 256, None, 10, None, p, p, None, 5, 0, p, p, None, 0, None)           # tags NULL, match non-NULL
    assert rc == _lib.TT_ERR_BAD_SHAPE and b"all NULL or all non-NULL" in libtt.tt_last_error()
    rc = f32(None, 4, 256, None, 10, t, p, None, None, 5, 0, p, p, None, 0, None)
    assert rc == _lib.TT_ERR_BAD_SHAPE and b"all NULL or all non-NULL" in libtt.tt_last_error()
    rc = f32(None, 4, 256, None, 10, t, p, p, ctypes.c_void_p(18), 5, 0, p, p, None, 0, None)
    assert rc == _lib.TT_ERR_BAD_SHAPE and b"keep" in libtt.tt_last_error()
    rc = f32(None, 4, 256, None, -1, t, p, p, None, 5, 0, p, p, None, 0, None)
    assert rc == _lib.TT_ERR_BAD_SHAPE and b"N=-1" in libtt.tt_last_error()


def test_python_shims_refuse_cpu_tensors_and_wrong_arguments():
    import twotowermlretrieval_amd as tt
    from twotowermlretrieval_amd import index
    assert tt.score_topk_tagged is index.score_topk_tagged
    assert "score_topk_tagged" in tt.__all__ and "score_topk_tagged" in index.__all__
    q, D = torch.zeros(2, 256), torch.zeros(100, 256)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tt.score_topk_tagged(q, D, torch.zeros(100, dtype=torch.int32), 0, 0, 5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tt.score_topk_tagged(q[0], D, torch.zeros(128, dtype=torch.int32), torch.zeros(1, dtype=torch.int32), 0, 5)
    cpu = torch.device("cpu")
    assert index._tag_words(0) == 0 and index._tag_words(1) == 32 and index._tag_words(32) == 32 and index._tag_words(33) == 64
    padded = torch.arange(128, dtype=torch.int32)
    assert index._check_tags(padded, 100, cpu) is padded                       # already whole tiles: taken as it is
    got = index._check_tags(padded[:100], 100, cpu)                            # [N]: padded with zeros
    assert got.shape == (128,) and torch.equal(got[:100], padded[:100]) and int(got[100:].abs().sum()) == 0
    for bad in (torch.zeros(99, dtype=torch.int32), torch.zeros(127, dtype=torch.int32), torch.zeros((100, 1), dtype=torch.int32)):
        with pytest.raises(ValueError, match="tags must hold"):
            index._check_tags(bad, 100, cpu)
    for bad in (torch.zeros(100, dtype=torch.int64), torch.zeros(100, dtype=torch.float32), [0] * 100):
        with pytest.raises(TypeError, match="int32"):
            index._check_tags(bad, 100, cpu)
    with pytest.raises(ValueError, match="live on"):
        index._check_tags(padded, 100, torch.device("cuda", 0))
    # match words: a [B] int32 tensor, or an int that is a 32-bit word
    ok = torch.zeros(4, dtype=torch.int32)
    assert index._match_words(ok, 4, cpu, "match_mask") is ok
    assert index._match_words(0xFFFFFFFF, 3, cpu, "match_mask").tolist() == [-1, -1, -1]
    assert index._match_words(0x80000001, 2, cpu, "match_value").tolist() == [-(1 << 31) + 1] * 2
    assert index._match_words(-1, 2, cpu, "match_mask").tolist() == [-1, -1] and index._match_words(7, 1, cpu, "x").tolist() == [7]
    for bad in (torch.zeros(3, dtype=torch.int32), torch.zeros((4, 1), dtype=torch.int32)):
        with pytest.raises(ValueError, match="one word per query"):
            index._match_words(bad, 4, cpu, "match_mask")
    for bad in (torch.zeros(4, dtype=torch.int64), 1.0, True, None):
        with pytest.raises(TypeError, match="match_value must be"):
            index._match_words(bad, 4, cpu, "match_value")
    for bad in (1 << 32, -(1 << 31) - 1):
        with pytest.raises(ValueError, match="32-bit"):
            index._match_words(bad, 4, cpu, "match_mask")
    with pytest.raises(ValueError, match="search runs on"):
        index._match_words(ok, 4, torch.device("cuda", 0), "match_mask")
    # an index without tags refuses before it looks at anything else
    for cls in (tt.BruteForceIndex, tt.StreamedIndex):
        ix = cls.__new__(cls)
        ix._tags = None
        assert ix.tags is None
        with pytest.raises(ValueError, match="no tags"):
            ix.tagged_search(q, 5, 0, 0)
    for cls in (tt.BruteForceIndex, tt.ShardedIndex, tt.StreamedIndex):
        assert callable(cls.set_tags) and callable(cls.tagged_search) and isinstance(cls.tags, property)


def test_reference_semantics():
    tags = np.array([0, 1, 2, 3, 0x80000000, 0x80000001, 0xFFFFFFFF, 0x00000301], dtype=np.uint32).view(np.int32)
    N = len(tags)
    e = tagged_ref.eligibility(tags, np.zeros(3, dtype=np.int32), np.zeros(3, dtype=np.int32))
    assert e.shape == (3, N) and e.all()                                        # mask 0, value 0: everything
    assert not tagged_ref.eligibility(tags, 0x0F, 0x10, B=2).any()              # a value bit outside the mask: nothing
    assert not tagged_ref.eligibility(tags, 0, 1, B=2).any()
    e = tagged_ref.eligibility(tags, 0xFFFFFFFF, np.array([0x80000000, -(1 << 31), 3], dtype=np.int64))
    assert e[0].tolist() == e[1].tolist() == [False] * 4 + [True] + [False] * 3  # bit 31: unsigned, whatever dtype carries it
    assert e[2].tolist() == [False, False, False, True, False, False, False, False]
    e = tagged_ref.eligibility(tags, np.array([0x80000000], dtype=np.uint32), np.array([0x80000000], dtype=np.uint32))
    assert e[0].tolist() == [False] * 4 + [True] * 3 + [False]
    e = tagged_ref.eligibility(tags, np.array([0xFF, 0x3FF]), np.array([0x01, 0x301]))      # one field, both fields
    assert e[0].tolist() == [False, True, False, False, False, True, False, True]
    assert e[1].tolist() == [False] * 7 + [True]
    keep = np.array([True, False] * 4)
    assert tagged_ref.eligibility(tags, 0, 0, keep=keep, B=1)[0].tolist() == keep.tolist()
    assert [(m, v, r.tolist()) for m, v, r in tagged_ref.distinct_filters(0xFFFFFFFF, np.array([1, 2, 1, -1]), 4)] == \
        [(0xFFFFFFFF, 1, [0, 2]), (0xFFFFFFFF, 2, [1]), (0xFFFFFFFF, 0xFFFFFFFF, [3])]


def test_reference_expected_maps_indices_back(oracle):
    rs = np.random.RandomState(0)
    D = rs.standard_normal((200, 32)).astype(np.float32)
    Q = rs.standard_normal((3, 32)).astype(np.float32)
    tags = (np.arange(200) % 3).astype(np.int32)
    elig = tagged_ref.eligibility(tags, 0xFFFFFFFF, np.array([0, 1, 7]))
    v, i = tagged_ref.expected(oracle, Q, D, elig, 5, [0, 1, 2], idx_offset=1000)
    for b in (0, 1):
        s = (Q[b].astype(np.float64) @ D.T.astype(np.float64))
        s[~elig[b]] = -np.inf
        assert i[b].tolist() == (np.argsort(-s, kind="stable")[:5] + 1000).tolist()
        assert ((i[b] - 1000) % 3 == b).all()
    assert (i[2] == -1).all() and np.isneginf(v[2]).all()                       # tenant 7 has no documents
