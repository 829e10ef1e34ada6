"""What the encoder entry points answer to bad calls, without a GPU: return code and the identifying part of tt_last_error()
for the three forward entries, the backward, tt_encoder_prepare_f32, tt_encoder_project_table_f32, tt_concat_ids_i64 and the
four size queries.

The table was taken from the library as it stood before the entries shared one call record and one validator; it pins the
answers, including the places where the entries disagree (a bad rnn_type is the projected entry's "projected table" refusal
and everyone else's "rnn_type="; the backward looks at rnn_type after the pointers and never at dropout_p; a misaligned
`prepared` is TT_ERR_WORKSPACE to the forward entries and TT_ERR_BAD_SHAPE to tt_encoder_project_table_f32).  Nothing here
reaches a launch: every call is refused by the argument checks, or (tt_concat_ids_i64) has nothing to copy."""
import ctypes

import pytest

from test_abi_cpu import libtt  # noqa: F401  (the fixture builds the library when it is missing)
from twotowermlretrieval_amd._lib import (TT_ENC_F32 as F32, TT_ENC_ONE_WORKGROUP as ONE_WG, TT_ENC_PHASE_BEGIN as BEGIN,
                                          TT_ENC_PHASE_FINISH as FINISH, TT_ENC_PROJECTED as PROJECTED,
                                          TT_ENC_SEED_ON_DEVICE as SEED_DEV, TT_ERR_BAD_SHAPE as BAD_SHAPE,
                                          TT_ERR_UNSUPPORTED as UNSUPPORTED, TT_ERR_WORKSPACE as WORKSPACE, TT_OK as OK)

FWD, PREP, PROJ, BWD = ("tt_encoder_forward_f32", "tt_encoder_forward_prepared_f32", "tt_encoder_forward_projected_f32",
                        "tt_encoder_backward_f32")
ENTRIES = (FWD, PREP, PROJ, BWD)
NAN = float("nan")


def _p(addr):
    return ctypes.c_void_p(addr) if addr else None


# A call that would launch: 256-byte aligned pointers (never dereferenced), 4 rows of 8 ids, the north-star tower's widths.
# `train` is the forward's train word and the other entries' opts; the backward counts as train 2 when g_table is given.
BASE = dict(ids=0x1000, B=4, T=8, table=0x2000, V=1000, E=300, H=256, L=1, bidir=0, rnn=0, weights=0x3000, prepared=0x4000,
            projected=0x5000, proj_w=0x6000, proj_b=0x6100, normalize=1, train=0, p=0.0, seed=0, out=0x7000, ws=0x10000,
            ws_short=0, status=0x8000, d_out=0x9000, grads=0xA000, g_proj_w=0xB000, g_proj_b=0xB100, g_table=0)


def _need(lib, fn, a):
    """The bytes the entry's size query asks for (the forward: train mode of the call, dropout buffers when it drops)."""
    mode = {FWD: a["train"] & 0xFF if a["train"] > 0 else 0, PREP: 0, PROJ: PROJECTED, BWD: 2 if a["g_table"] else 1}[fn]
    drop = int((fn == BWD or (fn == FWD and mode != 0)) and a["p"] > 0 and a["L"] > 1)
    return lib.tt_encoder_workspace_bytes(a["B"], a["T"], a["E"], a["H"], a["L"], a["bidir"], a["rnn"], mode, drop)


def _call(lib, fn, **over):
    """One call of `fn` with BASE's arguments, `over` replacing some; the workspace is ws_short bytes short of what the size
    query asks for, or ws_bytes long (shapes that no size query should be asked about)."""
    a = dict(BASE, **over)
    nbytes = a["ws_bytes"] if "ws_bytes" in a else max(_need(lib, fn, a) - a["ws_short"], 0)
    head = (_p(a["ids"]), a["B"], a["T"], _p(a["projected"] if fn == PROJ else a["table"]), a["V"], a["E"], a["H"], a["L"],
            a["bidir"], a["rnn"], _p(a["weights"]))
    proj = (_p(a["proj_w"]), _p(a["proj_b"]), a["normalize"])
    tail = (_p(a["ws"]), nbytes)
    if fn == FWD:
        return lib.tt_encoder_forward_f32(*head, *proj, a["train"], a["p"], a["seed"], _p(a["out"]), *tail, _p(a["status"]), None, None)
    if fn == BWD:
        return lib.tt_encoder_backward_f32(*head, *proj, a["p"], a["seed"], _p(a["d_out"]), _p(a["grads"]), _p(a["g_proj_w"]),
                                           _p(a["g_proj_b"]), _p(a["g_table"]), *tail, a["train"], _p(a["status"]), None, None)
    return getattr(lib, fn)(*head, _p(a["prepared"]), *proj, a["train"], _p(a["out"]), *tail, _p(a["status"]), None)


EMPTY = (BAD_SHAPE, "Cannot pack empty tensors")
TOO_LARGE = (UNSUPPORTED, "B*T or V too large for 32-bit token indices")
NULL = (BAD_SHAPE, "null pointer")
SHORT = (WORKSPACE, "workspace")  # the call passed every other check: only its workspace (one byte short) is refused
RNN_TYPE = (UNSUPPORTED, "rnn_type=%d (0 GRU, 1 LSTM, 2 RNN)")
NO_TABLE = (UNSUPPORTED, "a projected table serves inference calls of the f16-split GRU (H = 128, 256) only")
NO_PREPARED = (WORKSPACE, "prepared buffer null or not 256-B aligned")
NO_PROJECTED = (WORKSPACE, "prepared / projected buffer null or not 256-B aligned")
OPTS = {PREP: "opts=0x%x (0, TT_ENC_ONE_WORKGROUP, TT_ENC_F32)", PROJ: "opts=0x%x (0 or TT_ENC_ONE_WORKGROUP)",
        BWD: "opts=0x%x (0, TT_ENC_ONE_WORKGROUP, TT_ENC_SEED_ON_DEVICE, TT_ENC_F32)",
        FWD: "train=0x%x (0, 1 or 2, optionally | TT_ENC_ONE_WORKGROUP | one TT_ENC_PHASE_* | TT_ENC_F32)"}


def _opts(word, *entries):
    """The train / opts refusal of `entries` (all four when none is named) for `word`."""
    return {fn: (BAD_SHAPE, OPTS[fn] % (word & 0xFFFFFFFF)) for fn in (entries or ENTRIES)}


# case -> (arguments that differ from BASE, {entry: (return code, part of the message)}); "*" = every entry not named,
# None = the entry is not asked (the call would launch there, or the argument is not its own)
CASES = {
    # ---- shape (enc_check_shape: the first check of the forward and the backward; the prepared and projected entries look at
    #      their buffers and opts before it)
    "B=0": (dict(B=0, ws_bytes=0), {"*": (BAD_SHAPE, "Cannot pack empty tensors (B=0 T=8)")}),
    "B=-1": (dict(B=-1, ws_bytes=0), {"*": (BAD_SHAPE, "Cannot pack empty tensors (B=-1 T=8)")}),
    "T=0": (dict(T=0, ws_bytes=0), {"*": (BAD_SHAPE, "Cannot pack empty tensors (B=4 T=0)")}),
    "T=-1": (dict(T=-1, ws_bytes=0), {"*": (BAD_SHAPE, "Cannot pack empty tensors (B=4 T=-1)")}),
    "H=0": (dict(H=0, ws_bytes=0), {"*": (UNSUPPORTED, "HIDDEN_DIM=0 (supported: multiples of 32 in [32,512])")}),
    "H=100": (dict(H=100, ws_bytes=0), {"*": (UNSUPPORTED, "HIDDEN_DIM=100 (supported: multiples of 32 in [32,512])")}),
    "H=544": (dict(H=544, ws_bytes=0), {"*": (UNSUPPORTED, "HIDDEN_DIM=544 (supported: multiples of 32 in [32,512])")}),
    "E=0": (dict(E=0, ws_bytes=0), {"*": (UNSUPPORTED, "EMBED_DIM=0 must be a multiple of 4")}),
    "E=6": (dict(E=6, ws_bytes=0), {"*": (UNSUPPORTED, "EMBED_DIM=6 must be a multiple of 4")}),
    "L=0": (dict(L=0, ws_bytes=0), {"*": (UNSUPPORTED, "NUM_LAYERS=0 (supported: 1..4)")}),
    "L=5": (dict(L=5, ws_bytes=0), {"*": (UNSUPPORTED, "NUM_LAYERS=5 (supported: 1..4)")}),
    "B*T=2^29": (dict(B=32768, T=16384, ws_bytes=0), {"*": TOO_LARGE}),
    "B*T=2^29-2^15": (dict(B=32768, T=16383, ws_bytes=0), {"*": SHORT}),  # (the largest B*T that passes; no workspace given)
    "V=0": (dict(V=0, ws_bytes=0), {"*": TOO_LARGE}),
    "V=2^31-1": (dict(V=2**31 - 1, ws_bytes=0), {"*": TOO_LARGE}),
    "V=2^31-2": (dict(V=2**31 - 2, ws_short=1), {"*": SHORT}),
    "V=2^40": (dict(V=2**40, ws_bytes=0), {"*": TOO_LARGE}),
    # ---- train / opts: each entry names its own word and its own set of bits
    "train=3": (dict(train=3), _opts(3)),
    "train=-1": (dict(train=-1), _opts(-1)),
    "train=-2^31": (dict(train=-2**31), _opts(-2**31)),
    "unknown bit": (dict(train=0x4000), _opts(0x4000)),
    "unknown bit | 1": (dict(train=0x4001), _opts(0x4001)),
    "TT_ENC_PROJECTED is the size query's": (dict(train=PROJECTED), _opts(PROJECTED)),
    "both PHASE bits": (dict(train=BEGIN | FINISH), _opts(BEGIN | FINISH)),
    "both PHASE bits | 1": (dict(train=1 | BEGIN | FINISH), _opts(1 | BEGIN | FINISH)),
    "PHASE_BEGIN": (dict(train=BEGIN, ws_short=1), {FWD: SHORT, **_opts(BEGIN, PREP, PROJ, BWD)}),
    "PHASE_FINISH": (dict(train=FINISH, ws_short=1), {FWD: SHORT, **_opts(FINISH, PREP, PROJ, BWD)}),
    "SEED_ON_DEVICE": (dict(train=SEED_DEV, ws_short=1), {FWD: SHORT, BWD: SHORT, **_opts(SEED_DEV, PREP, PROJ)}),
    "TT_ENC_F32": (dict(train=F32, ws_short=1), {"*": SHORT, **_opts(F32, PROJ)}),
    "ONE_WORKGROUP": (dict(train=ONE_WG, ws_short=1), {"*": SHORT}),
    "train=1 on the inference entries": (dict(train=1), {FWD: None, **_opts(1, PREP, PROJ, BWD)}),
    "every option of the forward": (dict(train=2 | ONE_WG | BEGIN | SEED_DEV | F32, ws_short=1), {FWD: SHORT, "*": None}),
    "every option of the backward": (dict(train=ONE_WG | SEED_DEV | F32, ws_short=1), {BWD: SHORT, "*": None}),
    # ---- rnn_type: the projected entry answers with its own refusal (a table exists for the f16-split GRU only)
    "rnn_type=-1": (dict(rnn=-1, ws_bytes=0), {"*": (UNSUPPORTED, RNN_TYPE[1] % -1), PROJ: NO_TABLE}),
    "rnn_type=3": (dict(rnn=3, ws_bytes=0), {"*": (UNSUPPORTED, RNN_TYPE[1] % 3), PROJ: NO_TABLE}),
    # ---- dropout_p: checked by tt_encoder_forward_f32 alone (whatever `train` is); the backward takes any value
    "dropout_p=-0.1": (dict(p=-0.1, ws_short=1), {FWD: (BAD_SHAPE, "dropout_p=-0.1"), BWD: SHORT, "*": None}),
    "dropout_p=1": (dict(p=1.0, ws_short=1), {FWD: (BAD_SHAPE, "dropout_p=1"), BWD: SHORT, "*": None}),
    "dropout_p=nan": (dict(p=NAN, ws_short=1), {FWD: (BAD_SHAPE, "dropout_p=nan"), BWD: SHORT, "*": None}),
    "dropout_p=1, train=1, L=2": (dict(p=1.0, train=1, L=2, ws_short=1), {FWD: (BAD_SHAPE, "dropout_p=1"), "*": None}),
    "dropout_p=1, L=2, backward": (dict(p=1.0, L=2, ws_short=1), {BWD: SHORT, "*": None}),
    # ---- pointers.  The backward reads neither ids nor proj_b; proj_w / proj_b (and their gradients) matter when bidirectional
    "null ids": (dict(ids=0, ws_short=1), {"*": NULL, BWD: SHORT}),
    "null table": (dict(table=0, ws_short=1), {"*": NULL, PROJ: None}),
    "null weights": (dict(weights=0), {"*": NULL}),
    "null out": (dict(out=0, ws_short=1), {"*": NULL, BWD: SHORT}),
    "null status": (dict(status=0, ws_short=1), {"*": SHORT}),
    "null proj_w": (dict(proj_w=0, ws_short=1), {"*": SHORT}),
    "null proj_b": (dict(proj_b=0, ws_short=1), {"*": SHORT}),
    "null proj_w, bidirectional": (dict(proj_w=0, bidir=1), {"*": NULL}),
    "null proj_b, bidirectional": (dict(proj_b=0, bidir=1, ws_short=1), {"*": NULL, BWD: SHORT}),
    "null d_out": (dict(d_out=0), {BWD: NULL, "*": None}),
    "null grads": (dict(grads=0), {BWD: NULL, "*": None}),
    "null g_proj_w": (dict(g_proj_w=0, ws_short=1), {BWD: SHORT, "*": None}),
    "null g_proj_b": (dict(g_proj_b=0, ws_short=1), {BWD: SHORT, "*": None}),
    "null g_proj_w, bidirectional": (dict(g_proj_w=0, bidir=1), {BWD: NULL, "*": None}),
    "null g_proj_b, bidirectional": (dict(g_proj_b=0, bidir=1), {BWD: NULL, "*": None}),
    # ---- the projected table: inference of the f16-split GRU only
    "projected, H=64": (dict(H=64, ws_bytes=0), {PROJ: NO_TABLE, "*": None}),
    "projected, H=512": (dict(H=512, ws_bytes=0), {PROJ: NO_TABLE, "*": None}),
    "projected, LSTM": (dict(rnn=1, ws_bytes=0), {PROJ: NO_TABLE, "*": None}),
    "projected, RNN": (dict(rnn=2, ws_bytes=0), {PROJ: NO_TABLE, "*": None}),
    "projected, H=128": (dict(H=128, ws_short=1), {PROJ: SHORT, "*": None}),
    # ---- prepared / projected buffers: the two entries' own first check
    "null prepared": (dict(prepared=0), {PREP: NO_PREPARED, PROJ: NO_PROJECTED, "*": None}),
    "misaligned prepared": (dict(prepared=0x4000 + 128), {PREP: NO_PREPARED, PROJ: NO_PROJECTED, "*": None}),
    "null projected": (dict(projected=0), {PROJ: NO_PROJECTED, "*": None}),
    "misaligned projected": (dict(projected=0x5000 + 16), {PROJ: NO_PROJECTED, "*": None}),
    # ---- workspace, for train 0 / 1 / 2 (the backward: g_table absent / given)
    "workspace one byte short": (dict(ws_short=1), {"*": SHORT}),
    "workspace one byte short, train=1": (dict(ws_short=1, train=1), {FWD: SHORT, "*": None}),
    "workspace one byte short, train=2": (dict(ws_short=1, train=2), {FWD: SHORT, "*": None}),
    "workspace one byte short, g_table": (dict(ws_short=1, g_table=0xC000), {BWD: SHORT, "*": None}),
    "workspace one byte short, 2 layers, dropout": (dict(ws_short=1, train=1, L=2, bidir=1, p=0.2), {FWD: SHORT, "*": None}),
    "workspace one byte short, 2 layers, dropout, backward": (dict(ws_short=1, L=2, bidir=1, p=0.2), {BWD: SHORT, "*": None}),
    "no workspace": (dict(ws=0), {"*": SHORT}),
    "no workspace, train=1": (dict(ws=0, train=1), {FWD: SHORT, "*": None}),
    "no workspace, train=2": (dict(ws=0, train=2), {FWD: SHORT, "*": None}),
    "no workspace, g_table": (dict(ws=0, g_table=0xC000), {BWD: SHORT, "*": None}),
    "misaligned workspace": (dict(ws=0x10000 + 128), {"*": SHORT}),
    "misaligned workspace, train=1": (dict(ws=0x10000 + 128, train=1), {FWD: SHORT, "*": None}),
    "misaligned workspace, train=2": (dict(ws=0x10000 + 128, train=2), {FWD: SHORT, "*": None}),
    "misaligned workspace, g_table": (dict(ws=0x10000 + 128, g_table=0xC000), {BWD: SHORT, "*": None}),
    "train=1 workspace for a train=2 call": (dict(train=2, ws_bytes=-1), {FWD: SHORT, "*": None}),
    # ---- pairs of faults: the order of the checks
    "B=0, H=100": (dict(B=0, H=100, ws_bytes=0), {"*": EMPTY}),
    "H=100, E=6": (dict(H=100, E=6, ws_bytes=0), {"*": (UNSUPPORTED, "HIDDEN_DIM=100")}),
    "E=6, L=5": (dict(E=6, L=5, ws_bytes=0), {"*": (UNSUPPORTED, "EMBED_DIM=6")}),
    "L=5, V=0": (dict(L=5, V=0, ws_bytes=0), {"*": (UNSUPPORTED, "NUM_LAYERS=5")}),
    "H=100, null ids": (dict(H=100, ids=0, ws_bytes=0), {"*": (UNSUPPORTED, "HIDDEN_DIM=100")}),
    # (the prepared and projected entries refuse their opts before the shape is looked at)
    "H=100, train=3": (dict(H=100, train=3, ws_bytes=0), {FWD: (UNSUPPORTED, "HIDDEN_DIM=100"), BWD: (UNSUPPORTED, "HIDDEN_DIM=100"),
                                                         **_opts(3, PREP, PROJ)}),
    # (and their buffers before their opts)
    "B=0, null prepared, train=3": (dict(B=0, prepared=0, train=3, ws_bytes=0), {PREP: NO_PREPARED, PROJ: NO_PROJECTED, "*": EMPTY}),
    "train=3, null weights": (dict(train=3, weights=0), _opts(3)),
    "null weights, dropout_p=1": (dict(weights=0, p=1.0), {FWD: NULL, "*": None}),
    "null weights, rnn_type=3": (dict(weights=0, rnn=3, ws_bytes=0), {"*": NULL}),
    "dropout_p=1, rnn_type=3": (dict(p=1.0, rnn=3, ws_bytes=0), {FWD: (BAD_SHAPE, "dropout_p=1"), "*": None}),
    "rnn_type=3, no workspace": (dict(rnn=3, ws=0, ws_bytes=0), {"*": (UNSUPPORTED, RNN_TYPE[1] % 3), PROJ: NO_TABLE}),
    "projected, H=64, null weights": (dict(H=64, weights=0, ws_bytes=0), {PROJ: NULL, "*": None}),
    "projected, LSTM, no workspace": (dict(rnn=1, ws=0, ws_bytes=0), {PROJ: NO_TABLE, "*": None}),
    "null weights, no workspace": (dict(weights=0, ws=0, ws_bytes=0), {"*": NULL}),
}


def _params():
    for case, (over, expect) in CASES.items():
        for fn in ENTRIES:
            want = expect.get(fn, expect.get("*"))
            if want is not None:
                yield pytest.param(fn, over, want, id=f"{fn}-{case}")


@pytest.mark.parametrize("fn,over,want", list(_params()))
def test_encoder_entry_answers(libtt, fn, over, want):  # noqa: F811
    over = dict(over)
    if over.get("ws_bytes") == -1:  # the bytes of the same call with train = 1
        over["ws_bytes"] = _need(libtt, fn, dict(BASE, **dict(over, train=1)))
    rc, msg = want
    assert rc != OK
    assert _call(libtt, fn, **over) == rc
    err = libtt.tt_last_error().decode()
    assert err.startswith(fn + ": ") and msg in err, err


def test_one_byte_short_names_the_need(libtt):  # noqa: F811
    """The workspace refusal reports the bytes given and the bytes the size query asks for; the backward's names the train
    mode of the forward call that has to have filled it."""
    for fn, over in ((FWD, {}), (FWD, dict(train=1)), (FWD, dict(train=2)), (FWD, dict(train=1, L=2, p=0.5)), (PREP, {}), (PROJ, {}),
                     (PREP, dict(L=2, bidir=1)), (PROJ, dict(L=2, bidir=1))):
        need = _need(libtt, fn, dict(BASE, **over))
        assert _call(libtt, fn, ws_short=1, **over) == WORKSPACE
        assert f"{fn}: workspace {need - 1} < {need} bytes (or not 256-B aligned)" in libtt.tt_last_error().decode(), (fn, over)
    for over, mode in (({}, 1), (dict(g_table=0xC000), 2), (dict(L=2, p=0.5, rnn=1), 1)):
        need = _need(libtt, BWD, dict(BASE, **over))
        assert _call(libtt, BWD, ws_short=1, **over) == WORKSPACE
        want = f"{BWD}: workspace {need - 1} < {need} bytes: pass the buffer the forward call (train={mode}) filled"
        assert want in libtt.tt_last_error().decode(), over
    # the same bytes under another address: the misaligned workspace gets the same message with need <= given
    need = _need(libtt, FWD, BASE)
    assert _call(libtt, FWD, ws=0x10000 + 128) == WORKSPACE
    assert f"workspace {need} < {need} bytes" in libtt.tt_last_error().decode()


# ---- tt_encoder_prepare_f32, tt_encoder_project_table_f32 ------------------------------------------------------------------
def _prepare(lib, E=300, H=256, L=1, bidir=0, rnn=0, weights=0x3000, prepared=0x4000, short=0):
    need = lib.tt_encoder_prepared_bytes(E, H, L, bidir, rnn)
    return lib.tt_encoder_prepare_f32(E, H, L, bidir, rnn, _p(weights), _p(prepared), max(need - short, 0), None)


BUFFER = "(or null / not 256-B aligned)"
PREPARE_CASES = [
    (dict(H=0), UNSUPPORTED, "HIDDEN_DIM=0"), (dict(H=100), UNSUPPORTED, "HIDDEN_DIM=100"), (dict(H=544), UNSUPPORTED, "HIDDEN_DIM=544"),
    (dict(E=0), UNSUPPORTED, "EMBED_DIM=0"), (dict(E=6), UNSUPPORTED, "EMBED_DIM=6"),
    (dict(L=0), UNSUPPORTED, "NUM_LAYERS=0"), (dict(L=5), UNSUPPORTED, "NUM_LAYERS=5"),
    (dict(rnn=-1), UNSUPPORTED, "rnn_type=-1 (0 GRU, 1 LSTM, 2 RNN)"), (dict(rnn=3), UNSUPPORTED, "rnn_type=3 (0 GRU, 1 LSTM, 2 RNN)"),
    (dict(weights=0), WORKSPACE, BUFFER), (dict(prepared=0), WORKSPACE, BUFFER), (dict(prepared=0x4000 + 128), WORKSPACE, BUFFER),
    (dict(short=1), WORKSPACE, BUFFER), (dict(short=1, L=4, bidir=1, rnn=1), WORKSPACE, BUFFER),
    # order: shape, rnn_type, buffers
    (dict(H=100, rnn=3), UNSUPPORTED, "HIDDEN_DIM=100"), (dict(rnn=3, weights=0), UNSUPPORTED, "rnn_type=3"),
    (dict(L=5, prepared=0), UNSUPPORTED, "NUM_LAYERS=5"),
]


@pytest.mark.parametrize("over,rc,msg", PREPARE_CASES, ids=[str(c[0]) for c in PREPARE_CASES])
def test_prepare_answers(libtt, over, rc, msg):  # noqa: F811
    assert _prepare(libtt, **over) == rc
    err = libtt.tt_last_error().decode()
    assert err.startswith("tt_encoder_prepare_f32: ") and msg in err, err


def test_prepare_names_the_need(libtt):  # noqa: F811
    need = libtt.tt_encoder_prepared_bytes(300, 256, 2, 1, 0)
    assert _prepare(libtt, L=2, bidir=1, short=1) == WORKSPACE
    assert f"buffer {need - 1} < {need} bytes" in libtt.tt_last_error().decode()


def _project(lib, table=0x2000, V=1000, E=300, H=256, L=1, bidir=0, rnn=0, weights=0x3000, prepared=0x4000, projected=0x5000, short=0):
    need = lib.tt_encoder_projected_bytes(V, E, H, bidir, rnn)
    return lib.tt_encoder_project_table_f32(_p(table), V, E, H, L, bidir, rnn, _p(weights), _p(prepared), _p(projected),
                                            max(need - short, 0), None)


NO_TABLE_FOR = "rnn_type=%d H=%d has no projected table (f16-split GRU: H = 128, 256)"
NULL_OR_PREPARED = "null pointer (or prepared not 256-B aligned)"
PROJECT_CASES = [
    (dict(H=0), UNSUPPORTED, "HIDDEN_DIM=0"), (dict(H=100), UNSUPPORTED, "HIDDEN_DIM=100"), (dict(E=6), UNSUPPORTED, "EMBED_DIM=6"),
    (dict(L=0), UNSUPPORTED, "NUM_LAYERS=0"), (dict(L=5), UNSUPPORTED, "NUM_LAYERS=5"),
    (dict(V=0), UNSUPPORTED, "B*T or V too large"), (dict(V=2**31 - 1), UNSUPPORTED, "B*T or V too large"),
    (dict(H=64), UNSUPPORTED, NO_TABLE_FOR % (0, 64)), (dict(H=512), UNSUPPORTED, NO_TABLE_FOR % (0, 512)),
    (dict(rnn=1), UNSUPPORTED, NO_TABLE_FOR % (1, 256)), (dict(rnn=2), UNSUPPORTED, NO_TABLE_FOR % (2, 256)),
    # (no "rnn_type=" refusal of its own: an unknown cell has no table either)
    (dict(rnn=-1), UNSUPPORTED, NO_TABLE_FOR % (-1, 256)), (dict(rnn=3), UNSUPPORTED, NO_TABLE_FOR % (3, 256)),
    (dict(table=0), BAD_SHAPE, NULL_OR_PREPARED), (dict(weights=0), BAD_SHAPE, NULL_OR_PREPARED),
    # (TT_ERR_BAD_SHAPE here, TT_ERR_WORKSPACE from the forward entries that read the same buffer)
    (dict(prepared=0), BAD_SHAPE, NULL_OR_PREPARED), (dict(prepared=0x4000 + 128), BAD_SHAPE, NULL_OR_PREPARED),
    (dict(projected=0), WORKSPACE, BUFFER), (dict(projected=0x5000 + 128), WORKSPACE, BUFFER), (dict(short=1), WORKSPACE, BUFFER),
    (dict(short=1, bidir=1, H=128, L=3), WORKSPACE, BUFFER),
    # order: shape, table support, pointers, buffer
    (dict(L=5, H=64), UNSUPPORTED, "NUM_LAYERS=5"), (dict(H=64, table=0), UNSUPPORTED, NO_TABLE_FOR % (0, 64)),
    (dict(table=0, projected=0), BAD_SHAPE, NULL_OR_PREPARED),
]


@pytest.mark.parametrize("over,rc,msg", PROJECT_CASES, ids=[str(c[0]) for c in PROJECT_CASES])
def test_project_table_answers(libtt, over, rc, msg):  # noqa: F811
    assert _project(libtt, **over) == rc
    err = libtt.tt_last_error().decode()
    assert err.startswith("tt_encoder_project_table_f32: ") and msg in err, err


def test_project_table_names_the_need(libtt):  # noqa: F811
    need = libtt.tt_encoder_projected_bytes(1000, 300, 256, 1, 0)
    assert need == 2 * 1000 * 768 * 4  # [V][3H] floats per direction (a multiple of 256 bytes here)
    assert _project(libtt, bidir=1, short=1) == WORKSPACE
    assert f"buffer {need - 1} < {need} bytes" in libtt.tt_last_error().decode()


# ---- tt_concat_ids_i64 --------------------------------------------------------------------------------------------------------
def _concat(lib, a=0x1000, Ba=2, Ta=5, b=0x2000, Bb=3, Tb=7, out=0x3000, T=7):
    return lib.tt_concat_ids_i64(_p(a), Ba, Ta, _p(b), Bb, Tb, _p(out), T, None)


CONCAT_CASES = [
    (dict(Ba=-1), BAD_SHAPE), (dict(Bb=-1), BAD_SHAPE), (dict(Ta=-1), BAD_SHAPE), (dict(Tb=-1), BAD_SHAPE),
    (dict(T=6), BAD_SHAPE), (dict(T=4), BAD_SHAPE), (dict(Ta=8), BAD_SHAPE), (dict(T=-1), BAD_SHAPE),
    (dict(a=0), BAD_SHAPE), (dict(b=0), BAD_SHAPE), (dict(out=0), BAD_SHAPE), (dict(out=0, Ba=0, Bb=0), BAD_SHAPE),
    # nothing to copy: TT_OK without a launch (a null source is fine when it has no rows or no columns)
    (dict(Ba=0, Bb=0), OK), (dict(Ba=0, Bb=0, a=0, b=0), OK), (dict(Ta=0, Tb=0, T=0), OK), (dict(Ta=0, Tb=0, T=0, a=0, b=0), OK),
]


@pytest.mark.parametrize("over,rc", CONCAT_CASES, ids=[str(c[0]) for c in CONCAT_CASES])
def test_concat_ids_answers(libtt, over, rc):  # noqa: F811
    a = dict(Ba=2, Ta=5, Bb=3, Tb=7, T=7)
    a.update({k: v for k, v in over.items() if k in a})
    assert _concat(libtt, **over) == rc
    if rc != OK:
        want = "tt_concat_ids_i64: Ba=%d Ta=%d Bb=%d Tb=%d T=%d (or null pointer)" % (a["Ba"], a["Ta"], a["Bb"], a["Tb"], a["T"])
        assert libtt.tt_last_error().decode() == want


# ---- the size queries ---------------------------------------------------------------------------------------------------------
def test_workspace_query(libtt):  # noqa: F811
    q = libtt.tt_encoder_workspace_bytes
    for B, T, L, rnn in ((0, 8, 1, 0), (-1, 8, 1, 0), (4, 0, 1, 0), (4, -1, 1, 0), (4, 8, 0, 0), (4, 8, 5, 0), (4, 8, 1, -1), (4, 8, 1, 3)):
        for train in (0, 1, 2, PROJECTED):
            assert q(B, T, 300, 256, L, 0, rnn, train, 0) == 0, (B, T, L, rnn, train)
    for rnn in (0, 1, 2):
        for bidir in (0, 1):
            for L in (1, 2, 4):
                def w(train, dropout=0):
                    return q(70, 40, 300, 256, L, bidir, rnn, train, dropout)
                assert 0 < w(0) < w(1) < w(2) and w(0) % 256 == 0
                assert w(2) - w(1) == 70 * 40 * 300 * 4  # the gradient w.r.t. the gathered vectors, last in the layout
                assert w(-1) == w(-2**31) == w(0)         # a negative word sizes an inference call
                assert w(3) == w(255) == w(2)             # modes above 2 size as 2
                for bits in (ONE_WG, BEGIN, FINISH, SEED_DEV, F32, ONE_WG | SEED_DEV | F32):
                    assert w(1 | bits) == w(1) and w(bits) == w(0) and w(2 | bits) == w(2)
                assert w(1 | PROJECTED) == w(1) and w(2 | PROJECTED) == w(2)  # (a projected table serves inference only)
                if L == 1:  # no [tokens][gate rows] projections at all
                    assert w(0) - w(PROJECTED) == (2 if bidir else 1) * 70 * 40 * (4 if rnn == 1 else 3 if rnn == 0 else 1) * 256 * 4
                else:
                    assert w(PROJECTED) == w(0)
                assert w(0, 1) == w(0)  # dropout buffers exist in training, between layers
                assert (w(1, 1) > w(1)) == (L > 1)
    # (H and E are the call's to refuse: the query answers)
    assert q(4, 8, 6, 100, 1, 0, 0, 0, 0) > 0


def test_prepared_and_projected_queries(libtt):  # noqa: F811
    q = libtt.tt_encoder_prepared_bytes
    for E, H, L, rnn in ((0, 256, 1, 0), (-4, 256, 1, 0), (300, 0, 1, 0), (300, -32, 1, 0), (300, 256, 0, 0), (300, 256, 5, 0),
                         (300, 256, 1, -1), (300, 256, 1, 3)):
        assert q(E, H, L, 0, rnn) == q(E, H, L, 1, rnn) == 0, (E, H, L, rnn)
    # header + per layer and direction the two fp16 images of W_ih (k padded to 32) and the packed W_hh
    assert q(300, 256, 1, 0, 0) == 256 + 2 * 2 * 768 * 320 + 4 * 768 * 256
    assert q(300, 256, 1, 1, 0) == 256 + 2 * (2 * 2 * 768 * 320 + 4 * 768 * 256)
    assert q(300, 256, 2, 0, 0) == q(300, 256, 1, 0, 0) + 2 * 2 * 768 * 256 + 4 * 768 * 256
    assert q(300, 256, 1, 0, 1) > q(300, 256, 1, 0, 0) > q(300, 256, 1, 0, 2) > 0
    q = libtt.tt_encoder_projected_bytes
    for V, E, H, rnn in ((0, 300, 256, 0), (-1, 300, 256, 0), (2**31 - 1, 300, 256, 0), (1000, 0, 256, 0), (1000, 6, 256, 0),
                         (1000, 300, 64, 0), (1000, 300, 512, 0), (1000, 300, 100, 0), (1000, 300, 256, 1), (1000, 300, 256, 2),
                         (1000, 300, 256, -1), (1000, 300, 256, 3)):
        assert q(V, E, H, 0, rnn) == q(V, E, H, 1, rnn) == 0, (V, E, H, rnn)
    assert q(1000, 300, 256, 0, 0) == 1000 * 768 * 4 and q(1000, 300, 128, 1, 0) == 2 * 1000 * 384 * 4
    assert q(1001, 300, 128, 0, 0) == (1001 * 384 * 4 + 255) // 256 * 256  # each direction's table starts on a 256-byte line
    assert q(2**31 - 2, 300, 256, 0, 0) == ((2**31 - 2) * 768 * 4 + 255) // 256 * 256


def test_split_workgroups_query(libtt):  # noqa: F811
    q = libtt.tt_encoder_split_workgroups
    # only the GRU at H = 256 has the column-split recurrence, for at most 1024 rows
    for B, H, rnn in ((0, 256, 0), (-1, 256, 0), (1025, 256, 0), (16, 128, 0), (16, 64, 0), (16, 512, 0), (16, 100, 0), (16, 256, 1),
                      (16, 256, 2), (16, 256, -1), (16, 256, 3)):
        assert q(B, H, 0, rnn) == q(B, H, 1, rnn) == 0, (B, H, rnn)
    # 32 workgroups per 8 row groups of 16 rows and launch (without a device 256 compute units are assumed: every B up to
    # 1024 fits one direction, and a device that cannot hold both directions at once runs them in two launches)
    for B, per_dir in ((1, 32), (16, 32), (128, 32), (129, 64), (1024, 256)):
        assert q(B, 256, 0, 0) == per_dir, B
        assert q(B, 256, 1, 0) in (per_dir, 2 * per_dir), B
