"""The device-resident logit scale of K9 (tt_contrastive_loss_ls_f32, tt_contrastive_loss_sym_ls_f32) on the GPU, at the eight
shapes of tests/test_sym_loss_gpu.py and in the four kinds plain, grouped (label pattern a), soft (dense targets) and sym
(alpha 0.5):

  - the float entry, called at the temperature read back from temperature_out, writes the same bytes;
  - d_log_scale against float64 within scaled_loss_ref.bounds (each case prints measured / allowed);
  - the loss-only call and the call without d_log_scale write the same bits;
  - the clamp: T at the edge's bits and +0.0f outside, the gradient on the edges;
  - determinism over poisoned workspaces and outputs; a captured call replayed over a rewritten word; a NaN word."""
import functools
import math

import numpy as np
import pytest
import torch

from poison import CONTROL, poisoned_empty
from scaled_loss_ref import KINDS, bounds
from test_grouped_loss_gpu import call_abi as call_grouped, inputs, labels
from test_pool_loss_gpu import call_abi as call_plain, dev
from test_soft_loss_gpu import call_abi as call_soft, targets
from test_sym_loss_gpu import IDS, SHAPES, call_abi as call_sym

pytestmark = pytest.mark.gpu

ALPHA = 0.5
L = float(np.float32(-math.log(0.05)))       # the word of temperature 0.05, a float32 value
LO, HI = 0.0, float(np.float32(math.log(100.0)))
OUT = ("loss", "dirs", "T", "dl", "dq", "ddocs")
BIG = SHAPES[5]                              # several slices on every side


def arguments(kind, B, M, pos):
    """(q_groups, doc_groups, targets) of a kind at a shape (None where the kind has none)."""
    qg, dg = labels("a", B, M, pos) if kind == "grouped" else (None, None)
    return qg, dg, targets("b", B, M, pos) if kind == "soft" else None


class Call:
    """One *_ls call on device copies: outputs and workspace from torch.empty (poisoned_empty fills them), the word `l` on the
    device.  launch() enqueues it (again); result() reads everything back as numpy (None for what was not asked for)."""

    def __init__(self, kind, q, d, pos, l=L, lo=LO, hi=HI, grads=True, dls=True, t_out=True):
        from twotowermlretrieval_amd import _lib
        self.lib, self.L, self.kind, self.pos, self.lo, self.hi = _lib, _lib.lib(), kind, pos, lo, hi
        (self.B, self.H), self.M = q.shape, d.shape[0]
        qg, dg, tg = arguments(kind, self.B, self.M, pos)
        self.q, self.d = dev(q), dev(d)
        self.qg, self.dg = (None, None) if qg is None else (dev(np.asarray(qg, dtype=np.int64)), dev(np.asarray(dg, dtype=np.int64)))
        self.tg = None if tg is None else dev(tg)
        self.l = torch.tensor([l], dtype=torch.float32).cuda()
        new = lambda n: torch.empty(n, dtype=torch.float32, device="cuda")  # noqa: E731
        self.loss, self.dirs = new(1), new(2) if kind == "sym" else None
        self.T, self.dl = new(1) if t_out else None, new(1) if dls else None
        self.dq, self.dd = (torch.empty_like(self.q), torch.empty_like(self.d)) if grads else (None, None)
        self.need = self.L.tt_contrastive_loss_sym_ls_workspace_bytes(self.B, self.M, self.H) if kind == "sym" else \
            self.L.tt_contrastive_loss_ls_workspace_bytes(self.B, self.M, self.H, int(kind == "soft"))
        assert self.need > 0
        self.ws = torch.empty(self.need, dtype=torch.uint8, device="cuda")

    def launch(self):
        ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
        st = torch.cuda.current_stream().cuda_stream
        if self.kind == "sym":
            rc = self.L.tt_contrastive_loss_sym_ls_f32(self.q.data_ptr(), self.B, self.d.data_ptr(), self.M, self.H, self.pos,
                                                       ptr(self.qg), ptr(self.dg), self.l.data_ptr(), self.lo, self.hi, ALPHA,
                                                       self.loss.data_ptr(), ptr(self.dirs), ptr(self.T), ptr(self.dl), ptr(self.dq),
                                                       ptr(self.dd), self.ws.data_ptr(), self.need, st)
        else:
            rc = self.L.tt_contrastive_loss_ls_f32(self.q.data_ptr(), self.B, self.d.data_ptr(), self.M, self.H, self.pos,
                                                   ptr(self.qg), ptr(self.dg), ptr(self.tg), self.l.data_ptr(), self.lo, self.hi,
                                                   self.loss.data_ptr(), ptr(self.T), ptr(self.dl), ptr(self.dq), ptr(self.dd),
                                                   self.ws.data_ptr(), self.need, st)
        self.lib.check(rc)
        return self

    def result(self):
        torch.cuda.synchronize()
        got = (self.loss, self.dirs, self.T, self.dl, self.dq, self.dd)
        return {k: None if t is None else t.cpu().numpy() for k, t in zip(OUT, got)}


def call_ls(kind, q, d, pos, **kw):
    return Call(kind, q, d, pos, **kw).launch().result()


def call_float(kind, q, d, pos, temperature, grads=True):
    """The matching float entry -> the same dictionary (no T, no dl)."""
    B, M = q.shape[0], d.shape[0]
    qg, dg, tg = arguments(kind, B, M, pos)
    if kind == "sym":
        loss, dirs, dq, dd = call_sym(q, d, pos, ALPHA, temperature=temperature, grads=grads)
        return dict(loss=loss, dirs=dirs, dq=dq, ddocs=dd)
    loss, dq, dd = call_plain(q, d, pos, temperature, grads=grads) if kind == "plain" else \
        call_grouped(q, d, pos, qg, dg, temperature=temperature, grads=grads) if kind == "grouped" else \
        call_soft(q, d, tg, temperature=temperature, grads=grads)
    return dict(loss=loss, dirs=None, dq=dq, ddocs=dd)


def same(x, y, keys):
    for k in keys:
        if x[k] is None and y[k] is None:
            continue
        assert x[k].tobytes() == y[k].tobytes(), k


@functools.lru_cache(maxsize=None)
def reference(kind, B, M, pos, H, scale, l=L, lo=LO, hi=HI):
    """(want, tol) of a case, computed once and shared (no test writes to them)."""
    q, d = inputs(B, M, H, scale)
    qg, dg, tg = arguments(kind, B, M, pos)
    return bounds(kind, q, d, pos, l, lo, hi, q_groups=qg, doc_groups=dg, targets=tg, alpha=ALPHA)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("B,M,pos,H,scale,C", SHAPES, ids=IDS)
def test_the_float_entry_at_the_temperature_read_back_writes_the_same_bytes(B, M, pos, H, scale, C, kind):
    q, d = inputs(B, M, H, scale)
    new = call_ls(kind, q, d, pos)
    T = new["T"][0]
    assert abs(float(T) - math.exp(-L)) <= 4 * 2.0 ** -24 * math.exp(-L)          # (expf to a few ulp)
    old = call_float(kind, q, d, pos, T)
    assert all(np.isfinite(new[k]).all() for k in OUT if new[k] is not None)
    same(new, old, ("loss", "dirs", "dq", "ddocs"))
    # the loss alone: the same loss bits; without d_log_scale: the same gradients
    same(call_ls(kind, q, d, pos, grads=False, dls=False), new, ("loss", "dirs", "T"))
    same(call_ls(kind, q, d, pos, dls=False, t_out=False), new, ("loss", "dirs", "dq", "ddocs"))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("B,M,pos,H,scale,C", SHAPES, ids=IDS)
def test_the_scale_gradient_and_everything_else_vs_float64(B, M, pos, H, scale, C, kind):
    q, d = inputs(B, M, H, scale)
    want, tol = reference(kind, B, M, pos, H, scale)
    got = call_ls(kind, q, d, pos)
    dirs = (float(got["dirs"][0]), float(got["dirs"][1])) if kind == "sym" else ()
    flat = (float(got["loss"][0]),) + dirs + (got["dq"], got["ddocs"], float(got["dl"][0]))
    names = ("loss",) + (("L_qd", "L_dq") if kind == "sym" else ()) + ("dq", "ddocs", "d_log_scale")
    errs = [float(np.abs(np.asarray(g, dtype=np.float64) - np.asarray(w, dtype=np.float64)).max()) for g, w in zip(flat, want)]
    print("  ".join(f"{n} err {e:.3e} / allowed {t:.3e} (max|want| {np.abs(w).max():.3e})" for n, e, t, w in zip(names, errs, tol, want)))
    if tol[-1] > 0.0:          # (B = M = 1: G is exactly zero, and so are the sum and its bound)
        print(f"d_log_scale ratio {errs[-1] / tol[-1]:.4f}")
    for n, g, e, t in zip(names, flat, errs, tol):
        assert np.isfinite(g).all(), n
        assert e <= t, f"{n}: error {e:.3e} > {t:.3e}"


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("B,M,pos,H,scale,C", SHAPES, ids=IDS)
def test_the_clamp_holds_the_edge_temperature_and_passes_gradient_on_the_edges_alone(B, M, pos, H, scale, C, kind):
    q, d = inputs(B, M, H, scale)
    lo, hi = 1.0, 3.0
    zero = np.float32(0.0).tobytes()
    for edge, beyond in ((hi, 3.5), (lo, 0.5)):
        on, off = call_ls(kind, q, d, pos, l=edge, lo=lo, hi=hi), call_ls(kind, q, d, pos, l=beyond, lo=lo, hi=hi)
        assert abs(float(on["T"][0]) - math.exp(-edge)) <= 4 * 2.0 ** -24 * math.exp(-edge)
        same(on, off, ("T", "loss", "dirs", "dq", "ddocs"))          # (T has the bits of expf(-edge), so everything but dl has)
        assert off["dl"].tobytes() == zero                            # (bitwise +0.0f)
        want, tol = reference(kind, B, M, pos, H, scale, edge, lo, hi)
        e = abs(float(on["dl"][0]) - want[-1])
        print(f"l = {edge}: d_log_scale {float(on['dl'][0]):.6e} want {want[-1]:.6e} err {e:.3e} / allowed {tol[-1]:.3e}")
        assert e <= tol[-1]
        if B > 1 or M > 1:
            assert on["dl"].tobytes() != zero


@pytest.mark.parametrize("kind", KINDS)
def test_same_bits_whatever_workspace_and_outputs_held(kind):
    B, M, pos, H, scale, _ = BIG
    q, d = inputs(B, M, H, scale)
    out = {}
    for word in (0xFFFFFFFF, CONTROL):
        with poisoned_empty(word) as p:
            out[word] = call_ls(kind, q, d, pos)
            again = call_ls(kind, q, d, pos)
        assert p.tensors >= 12
        same(out[word], again, OUT)
    same(out[0xFFFFFFFF], out[CONTROL], OUT)
    assert all(np.isfinite(v).all() for v in out[CONTROL].values() if v is not None)


@pytest.mark.parametrize("kind", KINDS)
def test_a_replayed_graph_reads_the_word_as_it_is_at_replay(kind):
    """What a float argument cannot do: one capture, three words, each replay the bits of an eager call at that word."""
    B, M, pos, H, scale, _ = BIG
    q, d = inputs(B, M, H, scale)
    words = (float(np.float32(-math.log(0.07))), 0.0, L)
    eager = [call_ls(kind, q, d, pos, l=l) for l in words]
    assert len({e["loss"].tobytes() for e in eager}) == 3 and len({e["dl"].tobytes() for e in eager}) == 3
    call = Call(kind, q, d, pos, l=1.25)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call.launch()
    for l, want in zip(words, eager):
        call.l.fill_(l)
        for t in (call.loss, call.dirs, call.T, call.dl, call.dq, call.dd):
            if t is not None:
                t.fill_(float("nan"))
        call.ws.fill_(0xFF)
        graph.replay()
        same(call.result(), want, OUT)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("B,M,pos,H,scale,C", [SHAPES[2], BIG], ids=[IDS[2], IDS[5]])
def test_a_nan_word_gives_nan_and_the_call_returns(B, M, pos, H, scale, C, kind):
    q, d = inputs(B, M, H, scale)
    got = call_ls(kind, q, d, pos, l=float("nan"))
    assert np.isnan(got["T"][0]) and np.isnan(got["loss"][0]) and np.isnan(got["dl"][0])
    # the next call on the same stream is an ordinary one
    assert np.isfinite(call_ls(kind, q, d, pos)["dl"][0])
