"""CPU-side checks of the masked exact search (tt_score_topk_masked_*, tt_keep_mask_*): size query, argument validation and
the Python shims' refusals.  No GPU, no compute."""
import ctypes

import pytest
import torch


@pytest.fixture(scope="module")
def libtt():
    from twotowermlretrieval_amd import build, _lib
    build.build()
    return _lib.lib()


@pytest.mark.parametrize("B,N,d,k,bf16", [(32, 1_000_000, 256, 10, 0), (5, 300_001, 512, 64, 0), (130, 70_000, 128, 100, 1),
                                          (1024, 10_000_000, 256, 1000, 1), (3, 0, 64, 7, 0)])
def test_workspace_is_the_large_calls(libtt, B, N, d, k, bf16):
    n = libtt.tt_score_topk_masked_workspace_bytes(B, N, d, k, bf16)
    assert n > 0 and n == libtt.tt_score_topk_large_workspace_bytes(B, N, d, k, bf16)
    assert libtt.tt_score_topk_masked_workspace_bytes(0, N, d, k, bf16) == 0
    assert libtt.tt_score_topk_masked_workspace_bytes(B, N, d, 1025, bf16) == 0


def test_argument_validation_without_gpu(libtt):
    from twotowermlretrieval_amd import _lib
    p = ctypes.c_void_p(16)
    rc = libtt.tt_score_topk_masked_f32(None, 4, 256, None, 10, None, 1025, 0, p, p, None, 0, None)
    assert rc == _lib.TT_ERR_UNSUPPORTED and b"k=1025" in libtt.tt_last_error()
    rc = libtt.tt_score_topk_masked_bf16(None, 4, 96, None, 10, None, 5, 0, p, p, None, 0, None)
    assert rc == _lib.TT_ERR_UNSUPPORTED and b"d=96" in libtt.tt_last_error()
    rc = libtt.tt_score_topk_masked_f32(None, 4, 256, None, 10, ctypes.c_void_p(18), 5, 0, p, p, None, 0, None)
    assert rc == _lib.TT_ERR_BAD_SHAPE and b"keep" in libtt.tt_last_error()
    rc = libtt.tt_score_topk_masked_f32(None, 4, 256, None, -1, None, 5, 0, p, p, None, 0, None)
    assert rc == _lib.TT_ERR_BAD_SHAPE and b"N=-1" in libtt.tt_last_error()
    rc = libtt.tt_keep_mask_pack(None, -1, None, None)
    assert rc == _lib.TT_ERR_BAD_SHAPE and b"N=-1" in libtt.tt_last_error()
    rc = libtt.tt_keep_mask_pack(p, 10, ctypes.c_void_p(18), None)
    assert rc == _lib.TT_ERR_BAD_SHAPE
    rc = libtt.tt_keep_mask_clear_ids(None, 10, None, 3, 0, None)
    assert rc == _lib.TT_ERR_BAD_SHAPE
    assert libtt.tt_keep_mask_clear_ids(None, 10, None, 0, 0, None) == _lib.TT_OK     # nothing to clear


def test_python_shims_refuse_cpu_tensors_and_wrong_masks():
    import twotowermlretrieval_amd as tt
    from twotowermlretrieval_amd import index
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tt.pack_keep_mask(torch.ones(100, dtype=torch.bool))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tt.score_topk(torch.zeros(2, 256), torch.zeros(100, 256), 5, keep=torch.zeros(4, dtype=torch.int32))
    cpu = torch.device("cpu")
    assert index._keep_words(1) == 1 and index._keep_words(32) == 1 and index._keep_words(33) == 2 and index._keep_words(0) == 0
    ok = torch.zeros(32, dtype=torch.int32)
    assert index._check_keep(ok, 1000, cpu) is ok
    with pytest.raises(ValueError, match="32 words"):
        index._check_keep(torch.zeros(31, dtype=torch.int32), 1000, cpu)
    with pytest.raises(ValueError, match="32 words"):
        index._check_keep(torch.zeros((32, 1), dtype=torch.int32), 1000, cpu)
    with pytest.raises(TypeError, match="int32"):
        index._check_keep(torch.zeros(32, dtype=torch.bool), 1000, cpu)
    with pytest.raises(TypeError, match="int32"):
        index._check_keep(torch.zeros(32, dtype=torch.int64), 1000, cpu)
    with pytest.raises(ValueError, match="live on"):
        index._check_keep(ok, 1000, torch.device("cuda", 0))
