"""Large-k search (k up to TT_TOPK_LARGE_KMAX = 1024), the parts that need no GPU: the new exports are declared, exported
and bound; the workspace query works without a device; the entry points refuse bad shapes before touching the device; the
Python layer routes k > 64 to them and k <= 64 to the calls it always used."""
import ctypes

import pytest

from test_abi_cpu import _declared, libtt  # noqa: F401  (the fixture builds the library when it is missing)

LARGE_EXPORTS = ("tt_score_topk_large_workspace_bytes", "tt_score_topk_large_tier_offset", "tt_score_topk_large_f32",
                 "tt_score_topk_large_bf16", "tt_topk_merge_large", "tt_topk_merge_shards_large")
KMAX = 1024


def test_large_exports_are_declared_exported_and_bound(libtt):
    from twotowermlretrieval_amd import _lib
    names = _declared()
    for name in LARGE_EXPORTS:
        assert name in names and name in _lib.SIGNATURES, name
        assert hasattr(libtt, name), name


@pytest.mark.parametrize("bf16,d", [(0, 256), (0, 512), (0, 32), (1, 64), (1, 256)])
def test_large_workspace_query_needs_no_gpu(libtt, bf16, d):
    prev = 0
    for k in (1, 10, 64, 65, 100, 256, 1000, KMAX):
        n = libtt.tt_score_topk_large_workspace_bytes(33, 1_000_000, d, k, bf16)
        assert n > 0 and n % 8 == 0, (k, n)
        assert n >= prev, (k, n, prev)  # non-decreasing in k
        prev = n
        off = libtt.tt_score_topk_large_tier_offset(33, 1_000_000, d, k, bf16)
        assert off % 4 == 0 and off + 33 * 4 <= n
    assert libtt.tt_score_topk_large_workspace_bytes(0, 10, d, 100, bf16) == 0
    assert libtt.tt_score_topk_large_workspace_bytes(4, 10, d, KMAX + 1, bf16) == 0
    # the k <= 64 calls fit in the large call's workspace (the large entry point IS that call there)
    small = (libtt.tt_score_topk_bf16_workspace_bytes if bf16 else libtt.tt_score_topk_workspace_bytes)(33, 1_000_000, d, 64)
    assert libtt.tt_score_topk_large_workspace_bytes(33, 1_000_000, d, 64, bf16) >= small


def _call(libtt, fn, B=4, d=256, k=100):
    return getattr(libtt, fn)(None, B, d, None, 10, k, 0, ctypes.c_void_p(16), ctypes.c_void_p(16), None, 0, None)


@pytest.mark.parametrize("fn", ["tt_score_topk_large_f32", "tt_score_topk_large_bf16"])
def test_large_search_refusals_without_gpu(libtt, fn):
    from twotowermlretrieval_amd import _lib
    assert _call(libtt, fn, k=0) == _lib.TT_ERR_BAD_SHAPE
    assert _call(libtt, fn, k=KMAX + 1) == _lib.TT_ERR_UNSUPPORTED
    assert b"1024" in libtt.tt_last_error()
    for d in (100, 48):
        assert _call(libtt, fn, d=d) == _lib.TT_ERR_UNSUPPORTED
        assert f"d={d}".encode() in libtt.tt_last_error()
    if fn.endswith("bf16"):
        assert _call(libtt, fn, d=512) == _lib.TT_ERR_UNSUPPORTED
    # a supported shape with no workspace: refused before any launch
    p = ctypes.c_void_p(256)
    assert getattr(libtt, fn)(p, 4, 256, p, 10, KMAX, 0, p, p, None, 0, None) == _lib.TT_ERR_WORKSPACE


def test_large_merge_refusals_without_gpu(libtt):
    from twotowermlretrieval_amd import _lib
    v, i = ctypes.c_void_p(16), ctypes.c_void_p(16)
    assert libtt.tt_topk_merge_large(v, i, 4, 10, 0, v, i, None) == _lib.TT_ERR_BAD_SHAPE
    assert libtt.tt_topk_merge_large(v, i, 4, 10, KMAX + 1, v, i, None) == _lib.TT_ERR_UNSUPPORTED
    assert libtt.tt_topk_merge_large(v, i, 0, 10, KMAX, v, i, None) == _lib.TT_OK  # B = 0: nothing to do
    assert libtt.tt_topk_merge_shards_large(v, 2, 4096, 1024, 4, 100, 0, v, i, None) == _lib.TT_ERR_BAD_SHAPE
    assert libtt.tt_topk_merge_shards_large(v, 2, 4096, 1024, 4, 100, KMAX + 1, v, i, None) == _lib.TT_ERR_UNSUPPORTED
    # the existing merges keep their limit
    assert libtt.tt_topk_merge(v, i, 4, 10, 65, v, i, None) == _lib.TT_ERR_UNSUPPORTED


def test_python_routing_by_k():
    import torch
    from twotowermlretrieval_amd import index
    def fn(k, dtype):
        return index._exact_route(dtype, k, False).fn

    assert fn(1, torch.float32) == "tt_score_topk_f32"
    assert fn(64, torch.float32) == "tt_score_topk_f32"
    assert fn(64, torch.bfloat16) == "tt_score_topk_bf16"
    assert fn(65, torch.float32) == "tt_score_topk_large_f32"
    assert fn(1024, torch.bfloat16) == "tt_score_topk_large_bf16"
    assert fn(1025, torch.float32) == "tt_score_topk_large_f32"  # the refusal comes from the new entry point
    assert index._merge_fn(64) == "tt_topk_merge"
    assert index._merge_fn(65) == "tt_topk_merge_large"
    assert index._merge_fn(10, 50, shards=True) == "tt_topk_merge_shards"
    assert index._merge_fn(10, 200, shards=True) == "tt_topk_merge_shards_large"
    assert index._merge_fn(200, 200, shards=True) == "tt_topk_merge_shards_large"


def test_python_workspace_sizing_by_k(libtt):
    import torch
    from twotowermlretrieval_amd import index
    def ws_bytes(B, N, d, k, dtype):
        return index._exact_route(dtype, k, False).workspace_bytes(B, N, d, k, dtype)

    assert ws_bytes(8, 100_000, 256, 10, torch.float32) == libtt.tt_score_topk_workspace_bytes(8, 100_000, 256, 10)
    assert ws_bytes(8, 100_000, 256, 100, torch.float32) == libtt.tt_score_topk_large_workspace_bytes(8, 100_000, 256, 100, 0)
    assert ws_bytes(8, 100_000, 128, 1000, torch.bfloat16) == libtt.tt_score_topk_large_workspace_bytes(8, 100_000, 128, 1000, 1)
    # seed exchange stays off above 64
    assert index.seed_plan(8, 65) is None


def test_python_routing_of_the_screened_phases():
    """_screened_fn is the one place that names the screened entry points: every (phase, dtype) pair gives a bound export,
    and the six of them are exactly the tt_score_topk_screened_{seed_list_,seeded_,}{f32,bf16} the header declares."""
    import re
    from twotowermlretrieval_amd import _lib, index
    names = {index._screened_fn(phase, bf16) for phase in ("whole", "seed_list", "seeded") for bf16 in (False, True)}
    assert names <= set(_lib.SIGNATURES)
    declared = {n for n in _declared() if re.fullmatch(r"tt_score_topk_screened_(seed_list_|seeded_|)(f32|bf16)", n)}
    assert len(declared) == 6 and names == declared
    assert index._screened_fn("whole", False) == "tt_score_topk_screened_f32"
    assert index._screened_fn("seed_list", True) == "tt_score_topk_screened_seed_list_bf16"
    assert index._screened_fn("seeded", False) == "tt_score_topk_screened_seeded_f32"
    with pytest.raises(KeyError):
        index._screened_fn("seed", False)  # (tt_score_topk_screened_seed_f32 exists, with another signature)


def test_fp16_range_rule():
    from twotowermlretrieval_amd.index import _fp16_range_ok
    nan, below = float("nan"), 59999.996  # the largest float32 below 6.0e4
    assert _fp16_range_ok(1.0, 0.5) and _fp16_range_ok(below, below)
    assert not _fp16_range_ok(nan, 0.5) and not _fp16_range_ok(1.0, nan) and not _fp16_range_ok(nan, nan)
    assert not _fp16_range_ok(6.0e4, 0.5) and not _fp16_range_ok(below, 6.0e4)
    assert not _fp16_range_ok(float("inf"), 0.5)
