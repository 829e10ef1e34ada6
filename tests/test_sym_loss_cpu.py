"""The symmetric contrastive loss without a GPU: identities of the float64 helper (tests/sym_loss_ref.py); the new entry is
declared, bound and exported; the workspace query and every refusal work before any launch (the table of
tests/test_pool_loss_cpu.py plus alpha and the label pointers); the Python losses and the trainers refuse what they refuse
before anything is launched."""
import ctypes
import inspect
import re

import numpy as np
import pytest
import torch

import synth
from conftest import ROOT
from pool_loss_ref import pool_loss
from sym_loss_ref import bounds, sym_loss
from test_abi_cpu import libtt  # noqa: F401  (the fixture builds the library when it is missing)
from test_pool_loss_cpu import BASE, CASES
from twotowermlretrieval_amd._lib import TT_ERR_BAD_SHAPE as BAD_SHAPE

ENTRY = "tt_contrastive_loss_sym_f32"
QUERY = "tt_contrastive_loss_sym_workspace_bytes"
B, M, POS, H = 33, 70, 5, 20
TEMP = 0.05


def rows(seed, n, width, scale=1.0):
    return (synth.unit_rows(seed, n, width) * np.float32(scale)).astype(np.float32)


def test_alpha_0_is_the_pool_helper():
    q, d = rows(71, B, H, 3.0), rows(72, M, H, 3.0)
    want = pool_loss(q, d, POS, TEMP)
    got = sym_loss(q, d, POS, TEMP, 0.0)
    assert abs(got[0] - want[0]) <= 1e-15 and got[1] == got[0]
    assert np.abs(got[3] - want[1]).max() <= 1e-15 and np.abs(got[4] - want[2]).max() <= 1e-15
    mid = sym_loss(q, d, POS, TEMP, 0.25)
    assert abs(mid[0] - (0.75 * mid[1] + 0.25 * mid[2])) <= 1e-15 and abs(mid[1] - got[1]) <= 1e-15 and abs(mid[2] - got[2]) <= 1e-15


def test_alpha_1_is_the_plain_loss_with_the_roles_swapped():
    """The positives as queries, the queries as documents, pos_offset 0; the gradients change places with the roles, and no
    document off the positive columns receives any."""
    q, d = rows(73, B, H), rows(74, M, H, 2.0)
    got = sym_loss(q, d, POS, TEMP, 1.0)
    want = pool_loss(d[POS:POS + B], q, 0, TEMP)
    assert abs(got[0] - want[0]) <= 1e-15 and got[2] == got[0]
    assert np.abs(got[3] - want[2]).max() <= 1e-15 and np.abs(got[4][POS:POS + B] - want[1]).max() <= 1e-15
    assert not got[4][:POS].any() and not got[4][POS + B:].any() and got[4][POS:POS + B].any()


def test_on_a_square_symmetric_score_matrix_the_directions_agree():
    x = rows(75, B, H)
    got = sym_loss(x, x, 0, TEMP, 0.5)
    assert abs(got[1] - got[2]) <= 1e-15 and abs(got[0] - got[1]) <= 1e-15


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_with_one_label_everywhere_the_column_direction_is_exactly_zero(dtype):
    """All queries share one label and the positives carry it: every column keeps its own pair alone."""
    q, d = rows(76, B, H), rows(77, M, H)
    qg, dg = np.full(B, 4, dtype=np.int64), np.full(M, -1, dtype=np.int64)
    dg[POS:POS + B] = 4
    got = sym_loss(q, d, POS, TEMP, 0.5, qg, dg, dtype)
    assert got[2] == 0.0 and got[1] > 0.0
    zero = sym_loss(q, d, POS, TEMP, 0.0, qg, dg, dtype)
    # (L_dq adds nothing to any gradient: half the alpha = 0 gradients, to 64 roundings of the dtype at the largest entry --
    #  the two runs round their backward passes independently)
    eps = 64 * float(torch.finfo(dtype).eps)
    for k in (3, 4):
        assert np.abs(got[k] - 0.5 * zero[k]).max() <= eps * np.abs(zero[k]).max(), k
    want, tol = bounds(q, d, POS, TEMP, 0.5, qg, dg)
    assert want[2] == 0.0 and tol[2] == 0.0 and len(tol) == 5


def test_entries_are_declared_bound_and_exported(libtt):  # noqa: F811
    from twotowermlretrieval_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "tt.h").read_text(), flags=re.S)
    for name in (ENTRY, QUERY):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib.SIGNATURES and hasattr(libtt, name)
    res, args = _lib.SIGNATURES[ENTRY]
    old = _lib.SIGNATURES["tt_contrastive_loss_grouped_f32"]
    # (alpha behind temperature, loss_dirs behind loss)
    assert res is old[0] and args == old[1][:9] + [ctypes.c_float] + old[1][9:10] + [ctypes.c_void_p] + old[1][10:]
    import twotowermlretrieval_amd as tt
    assert tt.symmetric_contrastive_losses is tt.model.symmetric_contrastive_losses
    assert "symmetric_contrastive_losses" in tt.__all__ and "symmetric_contrastive_losses" in tt.model.__all__
    for fn in (tt.contrastive_softmax_loss, tt.in_batch_softmax_loss, tt.train_step, tt.DataParallelTrainer.__init__,
               tt.GraphedTrainStep.__init__):
        assert inspect.signature(fn).parameters["symmetric"].default == 0.0, fn
    assert "symmetric" not in inspect.signature(tt.soft_contrastive_loss).parameters
    # the step record: the seventh constructor argument, last and with a default; the six tuple fields stay what they were
    Spec = tt.trainer._StepSpec
    assert list(inspect.signature(Spec).parameters)[-1] == "symmetric" and Spec(0.2, "paired", 0.05, False, True, True).symmetric == 0.0
    half = Spec(0.2, "in_batch", 0.05, False, True, True, 0.5)
    assert half.symmetric == 0.5 and tuple(half) == (0.2, "in_batch", 0.05, False, True, True) and len(Spec._fields) == 6
    assert half != Spec(0.2, "in_batch", 0.05, False, True, True) and half == Spec(0.2, "in_batch", 0.05, False, True, True, 0.5)
    assert half._replace(margin=0.3).symmetric == 0.5 and half._replace(symmetric=1.0).symmetric == 1.0
    with pytest.raises(AttributeError):
        half.symmetric = 0.0


def test_workspace_query_needs_no_gpu_and_grows_over_the_plain_plan(libtt):  # noqa: F811
    q, plain = libtt.tt_contrastive_loss_sym_workspace_bytes, libtt.tt_contrastive_loss_workspace_bytes
    for shape in ((0, 4, 256), (-1, 4, 256), ((1 << 24) + 1, 1 << 25, 32), (4, 3, 256), (4, 0, 256), (4, (1 << 25) + 1, 32),
                  (4, 8, 0), (4, 8, -1), (4, 8, 513)):
        assert q(*shape) == 0, shape
    up = lambda x, m: (x + m - 1) // m * m  # noqa: E731
    for Bn, Mn, Hn, slices in ((1, 1, 1, 1), (33, 70, 20, 1), (130, 260, 32, 2), (512, 8192, 256, 4), (1025, 2060, 32, 5)):
        # the column partials [slices][Bq] twice, clse [Bq] and two row-loss arrays [Bq], f32
        assert q(Bn, Mn, Hn) - plain(Bn, Mn, Hn) == 4 * up(Bn, 128) * (2 * slices + 3), (Bn, Mn, Hn)
    assert q(1 << 24, 1 << 25, 512) > plain(1 << 24, 1 << 25, 512) > 0


def _p(addr):
    return ctypes.c_void_p(addr) if addr else None


SYM_BASE = dict(BASE, qg=8192, dg=8448, alpha=0.5, dirs=1280)
SYM_CASES = dict(CASES, **{"alpha=-0.1": (dict(alpha=-0.1), "alpha=-0.1"), "alpha=1.5": (dict(alpha=1.5), "alpha=1.5"),
                           "alpha=nan": (dict(alpha=float("nan")), "alpha="),
                           "null q_groups alone": (dict(qg=0), "both null or both non-null"),
                           "null doc_groups alone": (dict(dg=0), "both null or both non-null"),
                           "no labels, null workspace": (dict(qg=0, dg=0, ws=0), "null pointer"),
                           "no labels, misaligned workspace": (dict(qg=0, dg=0, ws=16384 + 8), "16-byte aligned"),
                           "no loss_dirs, workspace one byte short": (dict(dirs=0, ws_short=1), "workspace")})


@pytest.mark.parametrize("over,msg", list(SYM_CASES.values()), ids=list(SYM_CASES))
def test_bad_arguments_are_refused_before_any_launch(libtt, over, msg):  # noqa: F811
    """The pointers are never dereferenced: a call that got past its refusals would launch on a machine without a GPU and
    return another status than TT_ERR_BAD_SHAPE."""
    a = dict(SYM_BASE, **over)
    need = libtt.tt_contrastive_loss_sym_workspace_bytes(BASE["B"], BASE["M"], BASE["H"])
    assert need > 0
    nbytes = a["ws_bytes"] if "ws_bytes" in a else need - a["ws_short"]
    rc = libtt.tt_contrastive_loss_sym_f32(_p(a["q"]), a["B"], _p(a["docs"]), a["M"], a["H"], a["pos_offset"], _p(a["qg"]),
                                           _p(a["dg"]), a["temperature"], a["alpha"], _p(a["loss"]), _p(a["dirs"]), _p(a["dq"]),
                                           _p(a["ddocs"]), _p(a["ws"]), nbytes, None)
    assert rc == BAD_SHAPE
    err = libtt.tt_last_error().decode()
    assert err.startswith(ENTRY + ": ") and msg in err, err


def test_step_spec_refuses_what_no_step_can_run():
    from twotowermlretrieval_amd.trainer import _StepSpec
    ok = _StepSpec(0.2, "in_batch", 0.05, False, True, True, 0.5)
    assert ok.checked(graphs=False) is ok and ok.checked(graphs=True) is ok
    assert _StepSpec(0.2, "paired", 0.05, False, True, True, 0.0).checked(graphs=False).symmetric == 0.0
    for bad in (-0.1, 1.5, float("nan"), "0.5", None, True):
        with pytest.raises(ValueError, match="symmetric="):
            _StepSpec(0.2, "in_batch", 0.05, False, True, True, bad).checked(graphs=False)
    with pytest.raises(ValueError, match='needs negatives="in_batch"'):
        _StepSpec(0.2, "paired", 0.05, False, True, True, 0.5).checked(graphs=False)
    with pytest.raises(ValueError, match="gather_negatives=True.*queries of ALL ranks"):
        _StepSpec(0.2, "in_batch", 0.05, True, True, True, 0.5).checked(graphs=False)


def test_python_entries_refuse_before_any_launch_without_a_gpu():
    import twotowermlretrieval_amd as tt
    ids = torch.zeros((2, 3), dtype=torch.int64)
    x, d = torch.zeros(2, 4), torch.zeros(5, 4)
    for bad in (-0.1, 1.5, float("nan"), "0.5", None, True):
        with pytest.raises(ValueError, match="symmetric="):
            tt.contrastive_softmax_loss(x, d, symmetric=bad)
        with pytest.raises(ValueError, match="symmetric="):
            tt.in_batch_softmax_loss((x, x, x), symmetric=bad)
        with pytest.raises(ValueError, match="symmetric="):
            tt.train_step(None, None, ids, ids, ids, negatives="in_batch", symmetric=bad)
        with pytest.raises(ValueError, match="symmetric="):
            tt.DataParallelTrainer(None, negatives="in_batch", symmetric=bad)
        with pytest.raises(ValueError, match="symmetric="):
            tt.GraphedTrainStep(None, None, batch=2, q_width=16, doc_width=16, negatives="in_batch", symmetric=bad)
    with pytest.raises(ValueError, match='needs negatives="in_batch"'):
        tt.train_step(None, None, ids, ids, ids, symmetric=0.5)                                # (the default: "paired")
    with pytest.raises(ValueError, match="gather_negatives=True"):
        tt.train_step(None, None, ids, ids, ids, negatives="in_batch", gather_negatives=True, symmetric=0.5)
    with pytest.raises(ValueError, match="gather_negatives=True"):
        tt.DataParallelTrainer(None, negatives="in_batch", gather_negatives=True, symmetric=1.0)
    with pytest.raises(ValueError, match="soft=True and symmetric"):
        tt.GraphedTrainStep(None, None, batch=2, q_width=16, doc_width=16, negatives="in_batch", soft=True, symmetric=0.5)
    t = torch.zeros(2, 4)
    with pytest.raises(ValueError, match="targets and symmetric"):
        tt.train_step(None, None, ids, ids, ids, negatives="in_batch", targets=t, symmetric=0.5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):                                 # (the switch opens no CPU path)
        tt.contrastive_softmax_loss(x, d, symmetric=0.5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tt.symmetric_contrastive_losses(x, d)
    with pytest.raises(ValueError, match="both given or both None"):
        tt.symmetric_contrastive_losses(x, d, q_groups=torch.zeros(2, dtype=torch.int64))
