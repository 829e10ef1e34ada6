"""bf16-resident search, the parts that need no GPU: the new exports are declared, exported and bound; the bf16 kernel
refuses an unsupported width before touching the device; a CPU bf16 matrix is refused (there is no CPU fallback)."""
import ctypes

import pytest

from test_abi_cpu import _declared, libtt  # noqa: F401  (the fixture builds the library when it is missing)

BF16_EXPORTS = ("tt_score_topk_bf16", "tt_score_topk_bf16_workspace_bytes", "tt_index_stats_bf16",
                "tt_score_topk_screened_bf16", "tt_score_topk_screened_seed_list_bf16", "tt_score_topk_screened_seeded_bf16",
                "tt_score_topk_screened_bf16_workspace_bytes")


def test_bf16_exports_are_declared_exported_and_bound(libtt):
    from twotowermlretrieval_amd import _lib
    names = _declared()
    for name in BF16_EXPORTS:
        assert name in names and name in _lib.SIGNATURES
        assert hasattr(libtt, name)


def test_bf16_kernel_refuses_unsupported_width_without_gpu(libtt):
    from twotowermlretrieval_amd import _lib
    for d in (100, 32, 96, 320, 512):
        rc = libtt.tt_score_topk_bf16(None, 4, d, None, 10, 5, 0, ctypes.c_void_p(16), ctypes.c_void_p(16), None, 0, None)
        assert rc == _lib.TT_ERR_UNSUPPORTED, d
        assert f"d={d}".encode() in libtt.tt_last_error()
    rc = libtt.tt_score_topk_bf16(None, 4, 256, None, 10, 65, 0, ctypes.c_void_p(16), ctypes.c_void_p(16), None, 0, None)
    assert rc == _lib.TT_ERR_UNSUPPORTED


def test_debug_twin_is_exported_not_bound(libtt):
    from twotowermlretrieval_amd import _lib
    assert "tt_debug_screen_s16_bf16" in _declared("tt_debug.h") and hasattr(libtt, "tt_debug_screen_s16_bf16")
    assert "tt_debug_screen_s16_bf16" not in _lib.SIGNATURES


def test_screened_bf16_refuses_other_widths_without_gpu(libtt):
    from twotowermlretrieval_amd import _lib
    rc = libtt.tt_score_topk_screened_bf16(None, 4, 128, None, 100, 5, 1.0, 0, None, None, None, None, 0, None, None)
    assert rc == _lib.TT_ERR_UNSUPPORTED and b"d=128" in libtt.tt_last_error()


def test_bf16_workspace_query_needs_no_gpu(libtt):
    n = libtt.tt_score_topk_bf16_workspace_bytes(32, 1_000_000, 256, 10)
    assert n > 0 and n % 8 == 0
    assert libtt.tt_score_topk_bf16_workspace_bytes(0, 10, 256, 10) == 0
    # above 16 queries the layout is the fp32 kernel's (tt.h): its diagnostic offsets apply as they are
    assert n == libtt.tt_score_topk_workspace_bytes(32, 1_000_000, 256, 10)


def test_cpu_bf16_matrix_is_refused():
    import torch
    import twotowermlretrieval_amd as tt
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tt.score_topk(torch.zeros(2, 256), torch.zeros(10, 256, dtype=torch.bfloat16), 5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tt.BruteForceIndex(torch.zeros(10, 256, dtype=torch.bfloat16))
