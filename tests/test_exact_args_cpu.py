"""What the exact-search entry points answer to bad and edge calls, without a GPU: return code and the identifying part of
tt_last_error() for the k <= 64, large, masked and partials calls, the four merges, and the workspace / offset queries.

The table was taken from the library as it stood before the entries shared one validator; it pins the answers, including
the places where the entries disagree (B == 0 with an unsupported d: TT_OK from the k <= 64 calls, a refusal from the large and
masked ones).  Nothing here reaches a launch: every case is refused, or has B == 0."""
import ctypes

import pytest

from test_abi_cpu import libtt  # noqa: F401  (the fixture builds the library when it is missing)
from twotowermlretrieval_amd._lib import (TT_ERR_BAD_SHAPE as BAD_SHAPE, TT_ERR_UNSUPPORTED as UNSUPPORTED,
                                          TT_ERR_WORKSPACE as WORKSPACE, TT_OK as OK)

NONE = ctypes.c_size_t(-1).value  # (size_t)-1 of the offset queries
N_TOO_LARGE = 2**31 - 64


def _p(addr):
    return ctypes.c_void_p(addr)


# A call that would launch: pointers that satisfy every alignment rule (never dereferenced), 4 queries over 1000 rows.
BASE = dict(Q=256, B=4, d=256, D=512, N=1000, keep=768, k=10, idx_offset=0, out_val=1024, out_idx=2048, ws=4096, ws_short=0)

# family -> (entry points, k cap)
SEARCHES = {
    "small": (("tt_score_topk_f32", "tt_score_topk_bf16"), 64),
    "large": (("tt_score_topk_large_f32", "tt_score_topk_large_bf16"), 1024),
    "masked": (("tt_score_topk_masked_f32", "tt_score_topk_masked_bf16"), 1024),
    "partials": (("tt_score_topk_partials_f32",), 64),
}


def _need(lib, family, fn, a):
    bf = int(fn.endswith("bf16"))
    if family == "large":
        return lib.tt_score_topk_large_workspace_bytes(a["B"], a["N"], a["d"], a["k"], bf)
    if family == "masked":
        return lib.tt_score_topk_masked_workspace_bytes(a["B"], a["N"], a["d"], a["k"], bf)
    return (lib.tt_score_topk_bf16_workspace_bytes if bf else lib.tt_score_topk_workspace_bytes)(a["B"], a["N"], a["d"], a["k"])


def _search(lib, family, fn, **over):
    """One call of `fn` with BASE's arguments, `over` replacing some; the workspace is ws_short bytes short of what the entry's
    size query asks for, or ws_bytes long (shapes that no size query should be asked about)."""
    a = dict(BASE, **over)
    nbytes = a["ws_bytes"] if "ws_bytes" in a else max(_need(lib, family, fn, a) - a["ws_short"], 0)
    ptr = {key: (_p(a[key]) if a[key] else None) for key in ("Q", "D", "keep", "out_val", "out_idx", "ws")}
    head = (ptr["Q"], a["B"], a["d"], ptr["D"], a["N"])
    if family == "partials":
        return getattr(lib, fn)(*head, a["k"], a["idx_offset"], ptr["ws"], nbytes, None, None, None, None, None)
    mid = (ptr["keep"], a["k"]) if family == "masked" else (a["k"],)
    return getattr(lib, fn)(*head, *mid, a["idx_offset"], ptr["out_val"], ptr["out_idx"], ptr["ws"], nbytes, None)


# case -> (arguments that differ from BASE, {family: (return code, part of the message)}); "*" = every family not named.
# An unsupported d is 100 for the fp32 entries and 512 (fp32 only) for the bf16 ones: BAD_D stands for it.
BAD_D = "bad d"
SEARCH_CASES = {
    "B=-1": (dict(B=-1), {"*": (BAD_SHAPE, "B=-1 N=1000 k=10")}),
    "B=0": (dict(B=0), {"*": (OK, ""), "partials": (BAD_SHAPE, "B=0 N=1000 k=10")}),
    "N=-1": (dict(N=-1), {"*": (BAD_SHAPE, "B=4 N=-1 k=10")}),
    # (N == 0 with B > 0 and outputs is a launch; without outputs the refusal shows that the shape itself passed)
    "N=0, no outputs": (dict(N=0, out_val=0, out_idx=0), {"small": (BAD_SHAPE, "null output pointer"), "*": (BAD_SHAPE, "null pointer"),
                                                          "partials": (BAD_SHAPE, "B=4 N=0 k=10")}),
    "N=0, B=0": (dict(N=0, B=0), {"*": (OK, ""), "partials": (BAD_SHAPE, "B=0 N=0 k=10")}),
    "N=2^31-64": (dict(N=N_TOO_LARGE, ws_bytes=0), {"*": (UNSUPPORTED, "N=2147483584 >= 2^31-64")}),
    "N=2^31-64, B=0": (dict(N=N_TOO_LARGE, B=0, ws_bytes=0), {"small": (OK, ""), "*": (UNSUPPORTED, "N=2147483584 >= 2^31-64"),
                                                             "partials": (BAD_SHAPE, "B=0 N=2147483584")}),
    "k=0": (dict(k=0), {"*": (BAD_SHAPE, "B=4 N=1000 k=0")}),
    "k=65": (dict(k=65, ws_short=1), {"small": (UNSUPPORTED, "k=65 > 64"), "partials": (UNSUPPORTED, "k=65 > 64"), "*": (WORKSPACE, "workspace")}),
    "k=1025": (dict(k=1025, ws_bytes=0), {"small": (UNSUPPORTED, "k=1025 > 64"), "partials": (UNSUPPORTED, "k=1025 > 64"),
                                          "*": (UNSUPPORTED, "k=1025 > 1024")}),
    "k=65, B=0": (dict(k=65, B=0), {"*": (OK, ""), "partials": (BAD_SHAPE, "B=0 N=1000 k=65")}),
    "k=1025, B=0": (dict(k=1025, B=0, ws_bytes=0), {"small": (OK, ""), "*": (UNSUPPORTED, "k=1025 > 1024"),
                                                    "partials": (BAD_SHAPE, "B=0 N=1000 k=1025")}),
    "bad d": (dict(d=BAD_D, ws_bytes=0), {"*": (UNSUPPORTED, "d=%d (supported: ")}),
    "bad d, B=0": (dict(d=BAD_D, B=0, ws_bytes=0), {"small": (OK, ""), "*": (UNSUPPORTED, "d=%d (supported: "),
                                                   "partials": (BAD_SHAPE, "B=0 N=1000 k=10")}),
    "bad d, k=0": (dict(d=BAD_D, k=0, ws_bytes=0), {"*": (BAD_SHAPE, "k=0")}),
    "bad d, k=1025": (dict(d=BAD_D, k=1025, ws_bytes=0), {"*": (UNSUPPORTED, "d=%d (supported: ")}),
    "null Q": (dict(Q=0), {"*": (BAD_SHAPE, "null pointer")}),
    "null D": (dict(D=0), {"*": (BAD_SHAPE, "null pointer")}),
    "null out_val": (dict(out_val=0), {"small": (BAD_SHAPE, "null output pointer"), "*": (BAD_SHAPE, "null pointer"),
                                       "partials": None}),
    "null out_idx": (dict(out_idx=0), {"small": (BAD_SHAPE, "null output pointer"), "*": (BAD_SHAPE, "null pointer"),
                                       "partials": None}),
    "null out_idx, N too large": (dict(out_idx=0, N=N_TOO_LARGE, ws_bytes=0), {"small": (BAD_SHAPE, "null output pointer"),
                                                                                "*": (UNSUPPORTED, ">= 2^31-64"), "partials": None}),
    "null Q, no workspace": (dict(Q=0, ws=0, ws_bytes=0), {"*": (BAD_SHAPE, "null pointer")}),
    "null Q, B=0": (dict(Q=0, D=0, out_val=0, out_idx=0, ws=0, B=0), {"*": (OK, ""), "partials": (BAD_SHAPE, "B=0")}),
    "misaligned D": (dict(D=512 + 8), {"*": (BAD_SHAPE, "D must be 16-byte and the workspace 256-byte aligned")}),
    "misaligned Q": (dict(Q=256 + 2), {"*": (BAD_SHAPE, "D must be 16-byte and the workspace 256-byte aligned")}),
    "misaligned workspace": (dict(ws=4096 + 128), {"*": (BAD_SHAPE, "D must be 16-byte and the workspace 256-byte aligned")}),
    "misaligned workspace, one byte short": (dict(ws=4096 + 128, ws_short=1), {"*": (WORKSPACE, "workspace")}),
    "misaligned keep": (dict(keep=768 + 2), {"masked": (BAD_SHAPE, "keep must be 4-byte aligned"), "*": None}),
    "misaligned keep, B=0": (dict(keep=768 + 2, B=0), {"masked": (BAD_SHAPE, "keep must be 4-byte aligned"), "*": None}),
    "misaligned keep, null Q": (dict(keep=768 + 2, Q=0), {"masked": (BAD_SHAPE, "keep must be 4-byte aligned"), "*": None}),
    "no keep, null Q": (dict(keep=0, Q=0), {"masked": (BAD_SHAPE, "null pointer"), "*": None}),
    "workspace one byte short": (dict(ws_short=1), {"*": (WORKSPACE, "workspace")}),
    "workspace one byte short, k=64": (dict(ws_short=1, k=64), {"*": (WORKSPACE, "workspace")}),
    "workspace one byte short, k=100": (dict(ws_short=1, k=100), {"large": (WORKSPACE, "workspace"), "masked": (WORKSPACE, "workspace"),
                                                                  "*": None}),
    "no workspace": (dict(ws=0), {"*": (WORKSPACE, "workspace")}),
    "no workspace, misaligned D": (dict(ws=0, D=512 + 8), {"*": (WORKSPACE, "workspace")}),
}


def _search_params():
    for family, (fns, _) in SEARCHES.items():
        for fn in fns:
            for case, (over, expect) in SEARCH_CASES.items():
                want = expect.get(family, expect.get("*"))
                if want is not None:
                    yield pytest.param(family, fn, over, want, id=f"{fn}-{case}")


@pytest.mark.parametrize("family,fn,over,want", list(_search_params()))
def test_search_entry_answers(libtt, family, fn, over, want):  # noqa: F811
    bad_d = 512 if fn.endswith("bf16") else 100
    over = {key: (bad_d if val is BAD_D else val) for key, val in over.items()}
    rc, msg = want
    msg = msg % bad_d if "%d" in msg else msg
    assert _search(libtt, family, fn, **over) == rc
    if rc != OK:
        err = libtt.tt_last_error().decode()
        assert err.startswith(fn + ": ") and msg in err, err


def test_one_byte_short_names_the_need(libtt):  # noqa: F811
    """The workspace refusal reports the bytes given and the bytes the entry's own query asks for."""
    for family, (fns, _) in SEARCHES.items():
        for fn in fns:
            for k in (10, 100) if family in ("large", "masked") else (10,):
                need = _need(libtt, family, fn, dict(BASE, k=k))
                assert _search(libtt, family, fn, k=k, ws_short=1) == WORKSPACE
                assert f"workspace {need - 1} < {need} bytes" in libtt.tt_last_error().decode(), (fn, k)
                assert _search(libtt, family, fn, k=k, ws_bytes=0, B=0) == (BAD_SHAPE if family == "partials" else OK)


def test_bf16_entries_take_the_narrow_widths_only(libtt):  # noqa: F811
    for family in ("small", "large", "masked"):
        f32, bf16 = SEARCHES[family][0]
        for d in (32, 96, 320, 384, 448, 512):
            assert _search(libtt, family, bf16, d=d, ws_bytes=0) == UNSUPPORTED
            assert f"d={d} (supported: 64, 128, 192, 256)" in libtt.tt_last_error().decode()
        for d in (0, -4, 16, 100, 160, 224, 288, 576):
            assert _search(libtt, family, f32, d=d, ws_bytes=0) == UNSUPPORTED
            assert f"d={d} (supported: 32, 64, 96, 128, 192, 256, 320, 384, 448, 512)" in libtt.tt_last_error().decode()


# ---- the merges ------------------------------------------------------------------------------------------------------------------
V, I, G = 1024, 2048, 4096  # values, indices, a gathered buffer


def _merge(lib, fn, B=4, M=100, k=10, v=V, i=I):
    return getattr(lib, fn)(_p(v), _p(i), B, M, k, _p(v) if v else None, _p(i) if i else None, None)


# B = 4 rows of kp = 10: [4,10] f32 = 160 bytes, [4,10] i64 = 320 bytes; the tightest layout is (stride 480, idx offset 160)
def _shards(lib, fn, g=G, world=2, stride=480, off=160, B=4, kp=10, k=10, v=V, i=I):
    return getattr(lib, fn)(_p(g) if g else None, world, stride, off, B, kp, k, _p(v) if v else None, _p(i) if i else None, None)


MERGE_CASES = [
    # (entry point, arguments, return code, part of the message)
    ("tt_topk_merge", dict(B=-1), BAD_SHAPE, "tt_topk_merge: B=-1 M=100 k=10"),
    ("tt_topk_merge", dict(M=-1), BAD_SHAPE, "tt_topk_merge: B=4 M=-1 k=10"),
    ("tt_topk_merge", dict(k=0), BAD_SHAPE, "tt_topk_merge: B=4 M=100 k=0"),
    ("tt_topk_merge", dict(k=65), UNSUPPORTED, "tt_topk_merge: k=65 > 64"),
    ("tt_topk_merge", dict(k=1025), UNSUPPORTED, "tt_topk_merge: k=1025 > 64"),
    ("tt_topk_merge", dict(B=0), OK, ""),
    ("tt_topk_merge", dict(B=0, k=65), UNSUPPORTED, "tt_topk_merge: k=65 > 64"),
    ("tt_topk_merge_large", dict(B=-1, k=100), BAD_SHAPE, "tt_topk_merge_large: B=-1 M=100 k=100"),
    ("tt_topk_merge_large", dict(k=0), BAD_SHAPE, "tt_topk_merge_large: B=4 M=100 k=0"),
    ("tt_topk_merge_large", dict(k=1025), UNSUPPORTED, "tt_topk_merge_large: k=1025 > 1024"),
    ("tt_topk_merge_large", dict(B=0, k=65), OK, ""),
    ("tt_topk_merge_large", dict(B=0, k=64), OK, ""),
    ("tt_topk_merge_large", dict(B=0, k=1025), UNSUPPORTED, "tt_topk_merge_large: k=1025 > 1024"),
]
SHARD_CASES = [
    # (arguments, return code, message after the entry point's name) for k = 10 on tt_topk_merge_shards and k = 100 on _large
    (dict(B=-1), BAD_SHAPE, "world=2 B=-1 kp=10 k=%d"),
    (dict(world=0), BAD_SHAPE, "world=0 B=4 kp=10 k=%d"),
    (dict(kp=0), BAD_SHAPE, "world=2 B=4 kp=0 k=%d"),
    (dict(world=2**20, kp=2**12, stride=2**40, off=2**30), UNSUPPORTED, "world*kp too large"),
    (dict(stride=484), BAD_SHAPE, "layout (stride 484, idx offset 160) does not hold [B,kp] f32 + i64, 8-byte aligned"),
    (dict(stride=472), BAD_SHAPE, "layout (stride 472, idx offset 160)"),
    (dict(off=152), BAD_SHAPE, "layout (stride 480, idx offset 152)"),
    (dict(off=164, stride=488), BAD_SHAPE, "layout (stride 488, idx offset 164)"),
    (dict(g=G + 4), BAD_SHAPE, "layout (stride 480, idx offset 160)"),
    (dict(g=0), BAD_SHAPE, "layout (stride 480, idx offset 160)"),
    (dict(v=0), BAD_SHAPE, "layout (stride 480, idx offset 160)"),
    (dict(i=0), BAD_SHAPE, "layout (stride 480, idx offset 160)"),
    (dict(B=0, stride=4), BAD_SHAPE, "layout (stride 4, idx offset 160)"),
    (dict(B=0), OK, ""),
    (dict(B=0, stride=0, off=0), OK, ""),
]


@pytest.mark.parametrize("fn,over,rc,msg", MERGE_CASES, ids=[f"{c[0]}-{c[1]}" for c in MERGE_CASES])
def test_merge_answers(libtt, fn, over, rc, msg):  # noqa: F811
    assert _merge(libtt, fn, **over) == rc
    if rc != OK:
        assert msg in libtt.tt_last_error().decode(), libtt.tt_last_error()


@pytest.mark.parametrize("over,rc,msg", SHARD_CASES, ids=[str(c[0]) for c in SHARD_CASES])
def test_shard_merge_answers(libtt, over, rc, msg):  # noqa: F811
    for fn, k in (("tt_topk_merge_shards", 10), ("tt_topk_merge_shards_large", 100)):
        assert _shards(libtt, fn, k=k, **over) == rc, fn
        if rc != OK:
            err = libtt.tt_last_error().decode()
            assert err.startswith(fn + ": ") and (msg % k if "%d" in msg else msg) in err, err


def test_shard_merge_k_caps_and_the_handover_at_64(libtt):  # noqa: F811
    assert _shards(libtt, "tt_topk_merge_shards", k=0) == BAD_SHAPE
    assert _shards(libtt, "tt_topk_merge_shards", k=65) == UNSUPPORTED
    assert b"tt_topk_merge_shards: k=65 > 64" in libtt.tt_last_error()
    assert _shards(libtt, "tt_topk_merge_shards_large", k=0) == BAD_SHAPE
    assert b"tt_topk_merge_shards_large: world=2 B=4 kp=10 k=0" in libtt.tt_last_error()
    assert _shards(libtt, "tt_topk_merge_shards_large", k=1025) == UNSUPPORTED
    assert b"tt_topk_merge_shards_large: k=1025 > 1024" in libtt.tt_last_error()
    # k <= 64 on the large entry point is the k <= 64 call, and it is that call's name the layout refusal carries
    assert _shards(libtt, "tt_topk_merge_shards_large", k=64, stride=484) == BAD_SHAPE
    assert libtt.tt_last_error().decode().startswith("tt_topk_merge_shards: layout (stride 484, idx offset 160)")
    assert _shards(libtt, "tt_topk_merge_shards_large", k=10, world=2**20, kp=2**12, stride=2**40, off=2**30) == UNSUPPORTED
    assert libtt.tt_last_error().decode().startswith("tt_topk_merge_shards: world*kp too large")
    assert _shards(libtt, "tt_topk_merge_shards_large", k=10, B=-1) == BAD_SHAPE
    assert libtt.tt_last_error().decode().startswith("tt_topk_merge_shards_large: world=2 B=-1")
    assert _shards(libtt, "tt_topk_merge_shards_large", k=64, B=0) == OK


# ---- the workspace and offset queries -------------------------------------------------------------------------------------------
def test_workspace_queries(libtt):  # noqa: F811
    small = (libtt.tt_score_topk_workspace_bytes, libtt.tt_score_topk_bf16_workspace_bytes)
    for q in small:
        for B, N, k in ((-1, 1000, 10), (0, 1000, 10), (4, -1, 10), (4, 1000, 0), (0, 0, 0)):
            assert q(B, N, 256, k) == 0, (B, N, k)
        # no cap on k or N here: the search entry refuses, the size query answers
        for B, N, k in ((4, 0, 10), (4, 1000, 10), (4, 1000, 65), (4, 1000, 1025), (4, N_TOO_LARGE, 10)):
            assert q(B, N, 256, k) > 0, (B, N, k)
        assert q(4, 0, 256, 10) <= q(4, 1000, 256, 10) <= q(4, 1000, 256, 65) <= q(4, 1000, 256, 1025)
    for B in (4, 16, 17, 96):
        assert small[1](B, 1000, 256, 10) == small[0](B, 1000, 256, 10) or B <= 16  # (one layout above 16 queries)
    for q in (libtt.tt_score_topk_large_workspace_bytes, libtt.tt_score_topk_masked_workspace_bytes):
        for bf16 in (0, 1):
            for B, N, k in ((-1, 1000, 10), (0, 1000, 10), (4, -1, 10), (4, 1000, 0), (4, 1000, 1025), (0, 0, 0)):
                assert q(B, N, 256, k, bf16) == 0, (B, N, k)
            for B, N, k in ((4, 0, 10), (4, 1000, 10), (4, 1000, 65), (4, 1000, 1024), (4, N_TOO_LARGE, 10), (4, 0, 100)):
                assert q(B, N, 256, k, bf16) > 0, (B, N, k)
            # at k <= 64 the large call is the k <= 64 call plus one int per query (rounded up to 32 queries, then to 256 bytes)
            assert q(4, 1000, 256, 10, bf16) == small[bf16](4, 1000, 256, 10) + 256
            assert q(4, 1000, 256, 64, bf16) < q(4, 1000, 256, 65, bf16)


def test_offset_queries(libtt):  # noqa: F811
    for q in (libtt.tt_score_topk_pace_timeouts_offset, libtt.tt_score_topk_redo_flags_offset):
        for B, N, k in ((-1, 1000, 10), (0, 1000, 10), (4, -1, 10), (4, 0, 10), (4, 1000, 0), (4, 1000, 10), (64, 10_000_000, 10)):
            assert q(B, N, 256, k) == NONE, (B, N, k)  # refused, or fewer than three 32-query tiles: never paced
        assert q(96, 1000, 512, 10) == NONE           # 16-query tiles are never paced
    # three query tiles over a corpus with a tail pool: both exist, inside the workspace, behind one another
    need = libtt.tt_score_topk_workspace_bytes(96, 10_000_000, 256, 10)
    pace = libtt.tt_score_topk_pace_timeouts_offset(96, 10_000_000, 256, 10)
    redo = libtt.tt_score_topk_redo_flags_offset(96, 10_000_000, 256, 10)
    assert pace % 4 == 0 and redo % 256 == 0 and 0 < pace < redo and redo + 3 * 4 <= need
    # paced but no pool (too few tiles per chunk to set a tail aside): the time-out count exists, the redo flags do not
    assert libtt.tt_score_topk_pace_timeouts_offset(96, 1000, 256, 10) != NONE
    assert libtt.tt_score_topk_redo_flags_offset(96, 1000, 256, 10) == NONE
    for bf16 in (0, 1):
        q = libtt.tt_score_topk_large_tier_offset
        for B, N, k in ((-1, 1000, 100), (0, 1000, 100), (4, -1, 100), (4, 1000, 0), (4, 1000, 1025)):
            assert q(B, N, 256, k, bf16) == NONE, (B, N, k)
        for B, N, k in ((4, 0, 100), (4, 1000, 10), (4, 1000, 65), (4, 1000, 1024), (4, N_TOO_LARGE, 100)):
            off = q(B, N, 256, k, bf16)
            assert off % 256 == 0 and off + 4 * B <= libtt.tt_score_topk_large_workspace_bytes(B, N, 256, k, bf16), (B, N, k)
        assert q(4, 1000, 256, 10, bf16) == (libtt.tt_score_topk_bf16_workspace_bytes if bf16
                                            else libtt.tt_score_topk_workspace_bytes)(4, 1000, 256, 10)
