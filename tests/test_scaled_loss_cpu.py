"""The device-resident logit scale of K9 without a GPU: the identity the kernels take d_log_scale from, the clamp's mask, and
what tt_contrastive_loss_ls_f32 / tt_contrastive_loss_sym_ls_f32 refuse on the host (every refusal is in front of the first
launch, so the library answers on a machine with no device)."""
import ctypes
import math

import numpy as np
import pytest

from scaled_loss_ref import KINDS, bounds, clamp_passes, dot_route, scaled_loss
from test_grouped_loss_gpu import inputs, labels
from test_soft_loss_gpu import targets

LO, HI = 0.0, math.log(100.0)          # (temperatures 1 .. 0.01)
#          B     M   pos   H
SHAPES = [(33, 33, 0, 96), (17, 130, 113, 256), (65, 1040, 390, 96), (3, 1025, 1022, 32), (130, 260, 77, 32)]


def arguments(kind, B, M, pos, H):
    q, d = inputs(B, M, H, 1.0)
    kw = {}
    if kind == "grouped":
        kw["q_groups"], kw["doc_groups"] = labels("a", B, M, pos)
    if kind == "soft":
        kw["targets"] = targets("b", B, M, pos)
    return q, d, kw


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("B,M,pos,H", SHAPES)
def test_the_scale_gradient_is_the_sum_of_the_row_dots_in_float64(B, M, pos, H, kind):
    q, d, kw = arguments(kind, B, M, pos, H)
    for l in (-math.log(0.05), 0.0):
        auto = scaled_loss(kind, q, d, pos, l, LO, HI, **kw)[-1]
        dots, A = dot_route(kind, q, d, pos, l, LO, HI, **kw)
        assert A > 0.0 and abs(auto - dots) <= 1e-12 * A, (auto, dots, A)


@pytest.mark.parametrize("kind", KINDS)
def test_the_clamp_passes_gradient_on_its_edges_and_none_outside(kind):
    B, M, pos, H = 17, 130, 113, 256
    q, d, kw = arguments(kind, B, M, pos, H)
    lo, hi = 1.0, 3.0
    inside = {l: scaled_loss(kind, q, d, pos, l, lo, hi, **kw) for l in (lo, hi)}
    for l, edge in ((0.5, lo), (3.5, hi)):
        out = scaled_loss(kind, q, d, pos, l, lo, hi, **kw)
        assert not clamp_passes(l, lo, hi) and out[-1] == 0.0
        assert out[0] == inside[edge][0] and np.array_equal(out[-2], inside[edge][-2])    # (the loss and ddocs of T at the edge)
    for l in (lo, hi):
        assert clamp_passes(l, lo, hi) and inside[l][-1] != 0.0
        assert inside[l][-1] == pytest.approx(dot_route(kind, q, d, pos, l, lo, hi, **kw)[0], rel=1e-12)
    want, tol = bounds(kind, q, d, pos, 3.5, lo, hi, **kw)
    assert want[-1] == 0.0 and tol[-1] > 0.0       # (outside, the bound is the sum's own rounding: a leak of it would show)


@pytest.fixture(scope="module")
def libtt():
    from twotowermlretrieval_amd import build, _lib
    build.build()
    return _lib.lib()


def test_workspace_queries(libtt):
    plain = libtt.tt_contrastive_loss_workspace_bytes(65, 1040, 96)
    for soft in (0, 1):
        assert libtt.tt_contrastive_loss_ls_workspace_bytes(65, 1040, 96, soft) > \
            (libtt.tt_contrastive_loss_soft_workspace_bytes(65, 1040, 96) if soft else plain) > 0
    assert libtt.tt_contrastive_loss_sym_ls_workspace_bytes(65, 1040, 96) > libtt.tt_contrastive_loss_sym_workspace_bytes(65, 1040, 96)
    for B, M, H in ((0, 4, 32), (5, 4, 32), (4, 8, 0), (4, 8, 513), (4, (1 << 25) + 1, 32)):
        assert libtt.tt_contrastive_loss_ls_workspace_bytes(B, M, H, 0) == 0
        assert libtt.tt_contrastive_loss_ls_workspace_bytes(B, M, H, 1) == 0
        assert libtt.tt_contrastive_loss_sym_ls_workspace_bytes(B, M, H) == 0


def test_argument_validation_without_gpu(libtt):
    """Every pointer is the fake, aligned address 16: a call that passed its checks would launch on it, and none does."""
    from twotowermlretrieval_amd import _lib
    P = ctypes.c_void_p(16)
    B, M, H = 4, 8, 32
    big = 1 << 30

    def ls(B=B, M=M, H=H, pos=0, qg=None, dg=None, tg=None, l=P, lo=LO, hi=HI, loss=P, dls=P, dq=P, dd=P, ws=P, nbytes=big):
        return libtt.tt_contrastive_loss_ls_f32(P, B, P, M, H, pos, qg, dg, tg, l, lo, hi, loss, None, dls, dq, dd, ws, nbytes, None)

    def sym(B=B, M=M, H=H, pos=0, qg=None, dg=None, l=P, lo=LO, hi=HI, alpha=0.5, loss=P, dls=P, dq=P, dd=P, ws=P, nbytes=big):
        return libtt.tt_contrastive_loss_sym_ls_f32(P, B, P, M, H, pos, qg, dg, l, lo, hi, alpha, loss, None, None, dls, dq, dd, ws,
                                                    nbytes, None)

    nan = float("nan")
    for call in (ls, sym):
        for kw, said in ((dict(B=0), b"B=0"), (dict(M=3), b"M=3"), (dict(H=513), b"H=513"), (dict(pos=5), b"pos_offset"),
                         (dict(qg=P), b"q_groups"), (dict(dg=P), b"q_groups"),
                         (dict(l=None), b"log_scale"),
                         (dict(lo=nan), b"bounds"), (dict(hi=nan), b"bounds"), (dict(lo=2.0, hi=1.0), b"bounds"),
                         (dict(lo=-80.5), b"bounds"), (dict(hi=80.5), b"bounds"),
                         (dict(loss=None), b"null"), (dict(ws=None), b"null"),
                         (dict(dq=None), b"both"), (dict(dd=None), b"both"),
                         (dict(dq=None, dd=None), b"d_log_scale without dq"),
                         (dict(ws=ctypes.c_void_p(24)), b"aligned"),
                         (dict(nbytes=64), b"workspace 64 <")):
            assert call(**kw) == _lib.TT_ERR_BAD_SHAPE, kw
            assert said in libtt.tt_last_error(), (kw, libtt.tt_last_error())
    assert ls(qg=P, dg=P, tg=P) == _lib.TT_ERR_BAD_SHAPE and b"exclude" in libtt.tt_last_error()
    for alpha in (-0.1, 1.5, nan):
        assert sym(alpha=alpha) == _lib.TT_ERR_BAD_SHAPE and b"alpha" in libtt.tt_last_error()
    # one byte short of the plan is refused (the soft plan is the larger: targets change what is needed)
    for soft in (0, 1):
        need = libtt.tt_contrastive_loss_ls_workspace_bytes(B, M, H, soft)
        assert ls(tg=P if soft else None, nbytes=need - 1) == _lib.TT_ERR_BAD_SHAPE and b"workspace" in libtt.tt_last_error()
    assert sym(nbytes=libtt.tt_contrastive_loss_sym_ls_workspace_bytes(B, M, H) - 1) == _lib.TT_ERR_BAD_SHAPE
