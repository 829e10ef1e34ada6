"""What the thirteen screened-search entry points answer to bad calls, without a GPU: return code and the identifying part of
tt_last_error(), which starts with the name of the entry that was called; and what their size / offset queries answer.

The table was taken from the library as it stood before the entries shared one call record and one validator; it pins the
answers, quirks included (a misaligned bf16 corpus pointer is a *workspace* refusal whose message compares a size with itself;
B == 0 is refused here and TT_OK on the exact entries).  Every case is refused before the first launch: none reaches a kernel."""
import ctypes
import math

import pytest

from test_abi_cpu import libtt  # noqa: F401  (the fixture builds the library when it is missing)
from twotowermlretrieval_amd._lib import (TT_ERR_BAD_SHAPE as BAD_SHAPE, TT_ERR_UNSUPPORTED as UNSUPPORTED,
                                          TT_ERR_WORKSPACE as WORKSPACE, TT_OK as OK)

N_TOO_LARGE = 2**31 - 64
WHOLE, SEED, SEED_LIST, SEEDED = "whole", "seed", "seed_list", "seeded"

# entry point -> (phase, bf16 rows, takes a keep-bitmask)
ENTRIES = {
    "tt_score_topk_screened_f32": (WHOLE, False, False),
    "tt_score_topk_screened_bf16": (WHOLE, True, False),
    "tt_score_topk_screened_masked_f32": (WHOLE, False, True),
    "tt_score_topk_screened_masked_bf16": (WHOLE, True, True),
    "tt_score_topk_screened_seed_f32": (SEED, False, False),
    "tt_score_topk_screened_seed_list_f32": (SEED_LIST, False, False),
    "tt_score_topk_screened_seed_list_bf16": (SEED_LIST, True, False),
    "tt_score_topk_screened_seed_list_masked_f32": (SEED_LIST, False, True),
    "tt_score_topk_screened_seed_list_masked_bf16": (SEED_LIST, True, True),
    "tt_score_topk_screened_seeded_f32": (SEEDED, False, False),
    "tt_score_topk_screened_seeded_bf16": (SEEDED, True, False),
    "tt_score_topk_screened_seeded_masked_f32": (SEEDED, False, True),
    "tt_score_topk_screened_seeded_masked_bf16": (SEEDED, True, True),
}

# A call that would launch: pointers that satisfy every alignment rule (never dereferenced), 4 queries over 1000 rows.
# D16: the rows the screen reads (the fp16 shadow, or the bf16 rows of a bf16 entry, which has no other row pointer);
# D32: the fp32 rows of a Whole / Seeded f32 entry.
BASE = dict(Q=256, B=4, d=256, D32=512, D16=1024, N=1000, keep=1536, k=10, k_seed=5, dmax=1.0, idx_offset=0, out_val=2048,
            out_idx=2560, flag=3072, seed=3584, ws=4096, ws_short=0)
POINTERS = ("Q", "D32", "D16", "keep", "out_val", "out_idx", "flag", "seed", "ws")


def _need(lib, fn, a):
    """What the entry's own size query asks for."""
    _, bf16, masked = ENTRIES[fn]
    if masked:
        return lib.tt_score_topk_screened_masked_workspace_bytes(a["B"], a["N"], a["d"], a["k"], int(bf16))
    query = lib.tt_score_topk_screened_bf16_workspace_bytes if bf16 else lib.tt_score_topk_screened_workspace_bytes
    return query(a["B"], a["N"], a["d"], a["k"])


def _call(lib, fn, **over):
    """One call of `fn` with BASE's arguments, `over` replacing some; the workspace is ws_short bytes short of what the entry's
    size query asks for, or ws_bytes long (shapes that no size query should be asked about)."""
    phase, bf16, masked = ENTRIES[fn]
    a = dict(BASE, **over)
    nbytes = a["ws_bytes"] if "ws_bytes" in a else max(_need(lib, fn, a) - a["ws_short"], 0)
    p = {key: (ctypes.c_void_p(a[key]) if a[key] else None) for key in POINTERS}
    search = phase in (WHOLE, SEEDED)
    args = [p["Q"], a["B"], a["d"]]
    args += [p["D16"]] if bf16 else ([p["D32"], p["D16"]] if search else [p["D16"]])
    args += [a["N"]] + ([p["keep"]] if masked else []) + [a["k"]] + ([] if search else [a["k_seed"]]) + [a["dmax"]]
    args += [a["idx_offset"], p["out_val"], p["out_idx"]] if search else []
    args += [p["flag"]] + ([] if phase == WHOLE else [p["seed"]]) + [p["ws"], nbytes] + ([None] if search else []) + [None]
    return getattr(lib, fn)(*args)


def _all(phase, bf16, masked):
    return True


def _searches(phase, bf16, masked):
    return phase in (WHOLE, SEEDED)


def _seed_phases(phase, bf16, masked):
    return phase in (SEED, SEED_LIST)


# case -> (arguments that differ from BASE, which entries it applies to, return code, part of the message), in the order
# of the checks: shape, d, k, N, corpus norm, pointers, k_seed, keep, workspace
CASES = {
    "B=-1": (dict(B=-1), _all, BAD_SHAPE, "B=-1 N=1000 k=10"),
    "B=0": (dict(B=0), _all, BAD_SHAPE, "B=0 N=1000 k=10"),  # (TT_OK on the exact entries)
    "N=-1": (dict(N=-1), _all, BAD_SHAPE, "B=4 N=-1 k=10"),
    "N=0": (dict(N=0), _all, BAD_SHAPE, "B=4 N=0 k=10"),
    "k=0": (dict(k=0), _all, BAD_SHAPE, "B=4 N=1000 k=0"),
    "d=128": (dict(d=128, ws_bytes=0), _all, UNSUPPORTED, "d=128 (supported: 256)"),
    "d=252": (dict(d=252, ws_bytes=0), _all, UNSUPPORTED, "d=252 (supported: 256)"),
    "k=65": (dict(k=65), _all, UNSUPPORTED, "k=65 > 64"),
    "N=2^31-64": (dict(N=N_TOO_LARGE, ws_bytes=0), _all, UNSUPPORTED, "N too large; shard the corpus"),
    "dmax=-1": (dict(dmax=-1.0), _all, UNSUPPORTED, "corpus norm -1 outside the fp16 range"),
    "dmax=nan": (dict(dmax=math.nan), _all, UNSUPPORTED, "nan outside the fp16 range"),
    "dmax=60000": (dict(dmax=60000.0), _all, UNSUPPORTED, "corpus norm 60000 outside the fp16 range"),
    "dmax=inf": (dict(dmax=math.inf), _all, UNSUPPORTED, "corpus norm inf outside the fp16 range"),
    "null Q": (dict(Q=0), _all, BAD_SHAPE, "null pointer"),
    "null screen rows": (dict(D16=0), _all, BAD_SHAPE, "null pointer"),
    "null fallback_flag": (dict(flag=0), _all, BAD_SHAPE, "null pointer"),
    "null exact rows": (dict(D32=0), lambda phase, bf16, masked: phase in (WHOLE, SEEDED) and not bf16, BAD_SHAPE, "null pointer"),
    "null out_val": (dict(out_val=0), _searches, BAD_SHAPE, "null pointer"),
    "null out_idx": (dict(out_idx=0), _searches, BAD_SHAPE, "null pointer"),
    "null seed": (dict(seed=0), lambda phase, bf16, masked: phase != WHOLE, BAD_SHAPE, "null pointer"),
    "k_seed=0": (dict(k_seed=0), _seed_phases, BAD_SHAPE, "k_seed=0 outside [1, k=10]"),
    "k_seed=k+1": (dict(k_seed=11), _seed_phases, BAD_SHAPE, "k_seed=11 outside [1, k=10]"),
    "misaligned keep": (dict(keep=1536 + 2), lambda phase, bf16, masked: masked, BAD_SHAPE, "keep must be 4-byte aligned"),
    "no workspace": (dict(ws=0), _all, WORKSPACE, "workspace"),
    "workspace one byte short": (dict(ws_short=1), _all, WORKSPACE, "workspace"),
    "workspace one byte short, k=64": (dict(ws_short=1, k=64), _all, WORKSPACE, "workspace"),
    "misaligned workspace": (dict(ws=4096 + 128), _all, WORKSPACE, "workspace"),
    # (a workspace refusal, not a shape one; the fp16 shadow of the f32 entries has no such rule)
    "misaligned bf16 rows": (dict(D16=1024 + 8), lambda phase, bf16, masked: bf16, WORKSPACE, "workspace"),
    # two faults: the check that comes first answers
    "B=0, d=128": (dict(B=0, d=128, ws_bytes=0), _all, BAD_SHAPE, "B=0 N=1000 k=10"),
    "k=0, null Q": (dict(k=0, Q=0), _all, BAD_SHAPE, "B=4 N=1000 k=0"),
    "d=128, k=65": (dict(d=128, k=65, ws_bytes=0), _all, UNSUPPORTED, "d=128 (supported: 256)"),
    "k=65, N=2^31-64": (dict(k=65, N=N_TOO_LARGE, ws_bytes=0), _all, UNSUPPORTED, "k=65 > 64"),
    "N=2^31-64, dmax=-1": (dict(N=N_TOO_LARGE, dmax=-1.0, ws_bytes=0), _all, UNSUPPORTED, "N too large"),
    "dmax=nan, null Q": (dict(dmax=math.nan, Q=0), _all, UNSUPPORTED, "outside the fp16 range"),
    "null Q, k_seed=0": (dict(Q=0, k_seed=0), _seed_phases, BAD_SHAPE, "null pointer"),
    "null Q, misaligned keep": (dict(Q=0, keep=1536 + 2), lambda phase, bf16, masked: masked, BAD_SHAPE, "null pointer"),
    "null Q, no workspace": (dict(Q=0, ws=0, ws_bytes=0), _all, BAD_SHAPE, "null pointer"),
    "k_seed=0, misaligned keep": (dict(k_seed=0, keep=1536 + 2), lambda phase, bf16, masked: masked and phase == SEED_LIST,
                                  BAD_SHAPE, "k_seed=0 outside [1, k=10]"),
    "misaligned keep, no workspace": (dict(keep=1536 + 2, ws=0), lambda phase, bf16, masked: masked, BAD_SHAPE,
                                      "keep must be 4-byte aligned"),
    "misaligned bf16 rows, misaligned keep": (dict(D16=1024 + 8, keep=1536 + 2), lambda phase, bf16, masked: bf16 and masked,
                                              BAD_SHAPE, "keep must be 4-byte aligned"),
}


def _params():
    for fn, traits in ENTRIES.items():
        for case, (over, applies, rc, msg) in CASES.items():
            assert rc != OK, case  # a case that passed the checks would launch
            if applies(*traits):
                yield pytest.param(fn, over, rc, msg, id=f"{fn}-{case}")


@pytest.mark.parametrize("fn,over,rc,msg", list(_params()))
def test_screened_entry_answers(libtt, fn, over, rc, msg):  # noqa: F811
    assert _call(libtt, fn, **over) == rc
    err = libtt.tt_last_error().decode()
    assert err.startswith(fn + ": ") and msg in err, err


@pytest.mark.parametrize("fn", list(ENTRIES))
def test_workspace_refusal_names_the_bytes(libtt, fn):  # noqa: F811
    """The refusal of a short workspace names the bytes given and the bytes the entry's own query asks for; a workspace of
    the right size that is missing or misaligned (or, on a bf16 entry, misaligned rows) gets the same message, with the two
    figures equal."""
    for k in (10, 64):
        need = _need(libtt, fn, dict(BASE, k=k))
        assert _call(libtt, fn, k=k, ws_short=1) == WORKSPACE
        assert libtt.tt_last_error().decode() == f"{fn}: workspace {need - 1} < {need} bytes"
    need = _need(libtt, fn, BASE)
    for over in (dict(ws=0), dict(ws=4096 + 128)) + ((dict(D16=1024 + 8),) if ENTRIES[fn][1] else ()):
        assert _call(libtt, fn, **over) == WORKSPACE
        assert libtt.tt_last_error().decode() == f"{fn}: workspace {need} < {need} bytes", over


def test_size_and_offset_queries(libtt):  # noqa: F811
    f32, bf16 = libtt.tt_score_topk_screened_workspace_bytes, libtt.tt_score_topk_screened_bf16_workspace_bytes
    stats, masked = libtt.tt_score_topk_screened_stats_offset, libtt.tt_score_topk_screened_masked_workspace_bytes
    for B, N in ((-1, 1000), (0, 1000), (4, -1), (4, 0), (0, 0)):
        for k in (0, 10):
            assert f32(B, N, 256, k) == 0 and bf16(B, N, 256, k) == 0 and stats(B, N, 256, k) == 0, (B, N, k)
            assert masked(B, N, 256, k, 0) == 0 and masked(B, N, 256, k, 1) == 0, (B, N, k)
    for B, N, k in ((1, 1, 1), (4, 1000, 10), (65, 70_001, 64), (1024, 1_250_000, 10)):
        # the screen's own part first, the statistics inside it; behind it the exact search's workspace over the same rows
        own = f32(B, N, 256, k) - libtt.tt_score_topk_workspace_bytes(B, N, 256, k)
        assert own > 0 and own % 256 == 0 and own == bf16(B, N, 256, k) - libtt.tt_score_topk_bf16_workspace_bytes(B, N, 256, k)
        assert stats(B, N, 256, k) % 256 == 0 and 0 < stats(B, N, 256, k) + 8 * B <= own
        assert masked(B, N, 256, k, 0) == f32(B, N, 256, k) and masked(B, N, 256, k, 1) == bf16(B, N, 256, k)


def test_debug_entry_answers(libtt):  # noqa: F811
    """tt_debug_screen_s16 and its bf16 twin (include/tt_debug.h): both answer under the first one's name."""
    size = libtt.tt_debug_screen_s16_workspace_bytes
    size.restype, size.argtypes = ctypes.c_size_t, [ctypes.c_int, ctypes.c_int64, ctypes.c_int]
    for B, N, form in ((0, 1000, 0), (-1, 1000, 1), (4, 0, 0), (4, -1, 2), (4, 1000, 3), (4, 1000, 5), (4, 1000, -1)):
        assert size(B, N, form) == 0, (B, N, form)
    need = size(4, 1000, 2)
    assert need > 0 and need % 256 == 0
    for name in ("tt_debug_screen_s16", "tt_debug_screen_s16_bf16"):
        fn = getattr(libtt, name)
        fn.restype = ctypes.c_int
        fn.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_float, ctypes.c_void_p, ctypes.c_int,
                       ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]

        def call(Q=256, B=4, D=1024, N=1000, form=2, out=2048, ws=4096, nbytes=need):
            return fn(Q or None, B, D or None, N, 1.0, None, form, out or None, ws or None, nbytes, None)

        for over, rc, msg in ((dict(B=0), BAD_SHAPE, "B=0 N=1000 form=2"), (dict(N=0), BAD_SHAPE, "B=4 N=0 form=2"),
                              (dict(N=N_TOO_LARGE), BAD_SHAPE, "B=4 N=2147483584 form=2"), (dict(form=3), BAD_SHAPE, "B=4 N=1000 form=3"),
                              (dict(form=3, Q=0), BAD_SHAPE, "B=4 N=1000 form=3"),
                              (dict(Q=0), BAD_SHAPE, "null pointer"), (dict(D=0), BAD_SHAPE, "null pointer"),
                              (dict(out=0), BAD_SHAPE, "null pointer"), (dict(out=0, ws=0), BAD_SHAPE, "null pointer"),
                              (dict(ws=0), WORKSPACE, f"workspace {need} < {need} bytes"),
                              (dict(ws=4096 + 128), WORKSPACE, f"workspace {need} < {need} bytes"),
                              (dict(nbytes=need - 1), WORKSPACE, f"workspace {need - 1} < {need} bytes")):
            assert call(**over) == rc, (name, over)
            assert libtt.tt_last_error().decode() == "tt_debug_screen_s16: " + msg, (name, over)
