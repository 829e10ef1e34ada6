"""The symmetric contrastive loss (tt_contrastive_loss_sym_f32, contrastive_softmax_loss(symmetric=)) against its float64
statement (tests/sym_loss_ref.py), bit for bit against tt_contrastive_loss_f32 / tt_contrastive_loss_grouped_f32 at alpha = 0,
and against the plain entry called with the roles swapped at alpha = 1.

The shapes are the six of tests/test_grouped_loss_gpu.py plus three; C = slices x chunks of the QUERIES a tile of positive
columns walks in the column statistics, ib_slices(B, B):

     B     M    pos    H    C       what it reaches
     1     2      1   32    1 x 1   one column, its own pair alone
    33    33      0   96    1 x 1   M = B, a ragged second column tile
    17   130    113  256    1 x 1   positive columns 113..129: aligned tiles 3 and 4, most of their lanes no column
    65  1040    390   96    1 x 1   columns off a 32-boundary over four aligned tiles
     3  1025   1022   32    1 x 1   three columns in the last document tile but one
  1025  2060      5   32    5 x 2   five column slices of two chunks; the last holds query 1024 alone
     1     1      0   20    1 x 1   only the positive: both directions 0
   130   260     77   32    2 x 1   two column slices of one chunk, the second nearly empty (queries 128, 129); the last
                                    query tile ragged; columns 77..206 start off a 32-boundary and straddle tiles

Bound per result (loss, L_qd, L_dq, dq, ddocs): sym_loss_ref.bounds, the rule of pool_loss_ref.bounds."""
import functools

import numpy as np
import pytest
import torch

import pool_loss_ref
from poison import CONTROL, poisoned_empty
from sym_loss_ref import bounds
from test_grouped_loss_gpu import SHAPES as GROUPED_SHAPES, call_abi as call_grouped, inputs, labels
from test_pool_loss_gpu import call_abi as call_plain, dev, ib_slices, rows

pytestmark = pytest.mark.gpu

TEMP = 0.05
NAMES = ("loss", "L_qd", "L_dq", "dq", "ddocs")

#          B     M   pos   H   scale  C (slices, chunks)
SHAPES = [s + (c,) for s, c in zip(GROUPED_SHAPES, ((1, 1), (1, 1), (1, 1), (1, 1), (1, 1), (5, 2)))] + \
         [(1, 1, 0, 20, 1.0, (1, 1)),
          (130, 260, 77, 32, 1.0, (2, 1))]
IDS = [f"{s[0]}x{s[1]}+{s[2]}-H{s[3]}" for s in SHAPES]


def call_abi(q, docs, pos_offset, alpha, qg=None, dg=None, temperature=TEMP, grads=True, dirs=True):
    """The symmetric C entry on device copies; loss, loss_dirs, gradients and workspace come from torch.empty (poisoned_empty
    fills them).  Returns (loss [1], loss_dirs [2], dq, ddocs) as numpy (None for what was not asked for)."""
    from twotowermlretrieval_amd import _lib
    L = _lib.lib()
    (B, H), M = q.shape, docs.shape[0]
    tq, td = dev(q), dev(docs)
    tqg = None if qg is None else dev(np.asarray(qg, dtype=np.int64))
    tdg = None if dg is None else dev(np.asarray(dg, dtype=np.int64))
    loss = torch.empty(1, dtype=torch.float32, device="cuda")
    both = torch.empty(2, dtype=torch.float32, device="cuda") if dirs else None
    g = [torch.empty_like(t) for t in (tq, td)] if grads else [None] * 2
    need = L.tt_contrastive_loss_sym_workspace_bytes(B, M, H)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
    _lib.check(L.tt_contrastive_loss_sym_f32(tq.data_ptr(), B, td.data_ptr(), M, H, pos_offset, ptr(tqg), ptr(tdg), float(temperature),
                                             float(alpha), loss.data_ptr(), ptr(both), ptr(g[0]), ptr(g[1]), ws.data_ptr(), need,
                                             torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() if t is not None else None for t in (loss, both, g[0], g[1]))


def flat(got):
    """(loss [1], dirs [2], dq, ddocs) -> (loss, L_qd, L_dq, dq, ddocs), the order of sym_loss_ref."""
    return (float(got[0][0]), float(got[1][0]), float(got[1][1]), got[2], got[3])


@functools.lru_cache(maxsize=None)
def reference(B, M, pos, H, scale, alpha, pattern=None):
    """(want, tol) of a shape, computed once and shared (no test writes to them)."""
    q, d = inputs(B, M, H, scale)
    qg, dg = labels(pattern, B, M, pos) if pattern else (None, None)
    return bounds(q, d, pos, TEMP, alpha, qg, dg)


def within(got, want, tol, names=NAMES):
    errs = [float(np.abs(np.asarray(g, dtype=np.float64) - np.asarray(w, dtype=np.float64)).max()) for g, w in zip(got, want)]
    print("  ".join(f"{name} err {e:.3e} / allowed {t:.3e} (max|want| {np.abs(w).max():.3e})"
                    for name, e, t, w in zip(names, errs, tol, want)))
    for name, g, e, t in zip(names, got, errs, tol):
        assert np.isfinite(g).all(), name
        assert e <= t, f"{name}: error {e:.3e} > {t:.3e}"


@pytest.mark.parametrize("alpha", [0.5, 1.0, 0.25])
@pytest.mark.parametrize("B,M,pos,H,scale,C", SHAPES, ids=IDS)
def test_loss_directions_and_gradients_vs_float64(B, M, pos, H, scale, C, alpha):
    per, n = ib_slices(B, B)
    assert (n, per) == C, (n, per)              # (the case reaches the class the table says it does)
    assert pos + B <= M
    q, d = inputs(B, M, H, scale)
    want, tol = reference(B, M, pos, H, scale, alpha)
    got = flat(call_abi(q, d, pos, alpha))
    within(got, want, tol)
    if alpha == 1.0:
        outside = np.delete(got[4], np.arange(pos, pos + B), axis=0)
        assert outside.tobytes() == bytes(outside.nbytes)            # (bitwise +0.0 off the positive columns)


@pytest.mark.parametrize("B,M,pos,H,scale,C", SHAPES, ids=IDS)
def test_alpha_0_gives_the_bits_of_the_one_directional_entries_and_still_both_directions(B, M, pos, H, scale, C):
    q, d = inputs(B, M, H, scale)
    new, old = call_abi(q, d, pos, 0.0), call_plain(q, d, pos, TEMP)
    for x, y in zip((new[0], new[2], new[3]), old):
        assert np.isfinite(x).all() and x.tobytes() == y.tobytes()
    alone = call_abi(q, d, pos, 0.0, grads=False)
    assert alone[0].tobytes() == old[0].tobytes() and alone[1].tobytes() == new[1].tobytes()
    assert new[1][0:1].tobytes() == old[0].tobytes()                 # (L_qd is that loss)
    # L_dq against float64: a dispatch to the one-directional kernels would not have it
    want, tol = reference(B, M, pos, H, scale, 0.5)
    within((float(new[1][1]),), want[2:3], tol[2:3], ("L_dq",))
    # with labels: the grouped entry's bits
    qg, dg = labels("a", B, M, pos)
    new, old = call_abi(q, d, pos, 0.0, qg, dg), call_grouped(q, d, pos, qg, dg)
    for x, y in zip((new[0], new[2], new[3]), old):
        assert np.isfinite(x).all() and x.tobytes() == y.tobytes()
    want, tol = reference(B, M, pos, H, scale, 0.5, "a")
    within((float(new[1][1]),), want[2:3], tol[2:3], ("L_dq, labels a",))


@pytest.mark.parametrize("B,M,pos,H,scale,C", SHAPES, ids=IDS)
def test_alpha_1_is_the_plain_entry_with_the_roles_swapped(B, M, pos, H, scale, C):
    """The positives as queries, the queries as documents, pos_offset 0.  Both are float32 results of one float64 value, so they
    differ by at most the sum of the two calls' own bounds."""
    q, d = inputs(B, M, H, scale)
    positives = np.ascontiguousarray(d[pos:pos + B])
    got = call_abi(q, d, pos, 1.0)
    swapped = call_plain(positives, q, 0, TEMP)
    _, tol = reference(B, M, pos, H, scale, 1.0)
    _, tol_swapped = pool_loss_ref.bounds(positives, q, 0, TEMP)
    pairs = (("loss", got[0], swapped[0], tol[0] + tol_swapped[0]),
             ("L_dq", got[1][1:2], swapped[0], tol[2] + tol_swapped[0]),
             ("dq", got[2], swapped[2], tol[3] + tol_swapped[2]),
             ("ddocs", got[3][pos:pos + B], swapped[1], tol[4] + tol_swapped[1]))
    for name, x, y, t in pairs:
        e = float(np.abs(x.astype(np.float64) - y.astype(np.float64)).max())
        print(f"{name}: differ by {e:.3e} / allowed {t:.3e}")
        assert np.isfinite(x).all() and e <= t, name
    outside = np.delete(got[3], np.arange(pos, pos + B), axis=0)
    assert outside.tobytes() == bytes(outside.nbytes)


@pytest.mark.parametrize("pattern", list("abcde"))
@pytest.mark.parametrize("B,M,pos,H,scale,C", SHAPES, ids=IDS)
def test_labels_leave_both_softmaxes(B, M, pos, H, scale, C, pattern):
    q, d = inputs(B, M, H, scale)
    qg, dg = labels(pattern, B, M, pos)
    want, tol = reference(B, M, pos, H, scale, 0.5, pattern)
    got = flat(call_abi(q, d, pos, 0.5, qg, dg))
    within(got, want, tol)
    if pattern == "c":          # (one label everywhere: every query and every column keeps its own pair alone)
        assert want[0] == 0.0 and got[0] == 0.0 and got[1] == 0.0 and got[2] == 0.0 and not got[3].any() and not got[4].any()
    if pattern == "e":          # (equal negative labels: nothing matches, the bits of the call without labels)
        for x, y in zip(call_abi(q, d, pos, 0.5, qg, dg), call_abi(q, d, pos, 0.5)):
            assert x.tobytes() == y.tobytes()


@pytest.mark.parametrize("B,M,pos,H,scale", [(65, 1040, 390, 96, 1.0e-3), (1025, 2060, 5, 32, 1.0e-3), (130, 260, 77, 32, 1.0)])
def test_columns_that_keep_their_own_pair_alone_cost_exactly_nothing(B, M, pos, H, scale):
    """All queries share one label and the positives carry it: L_dq is 0.0f exactly and adds nothing to any gradient, so the
    results are (1 - alpha) times those at alpha = 0.  Both sides are float32 results of one float64 value (the factor 0.5 is
    exact), so they differ by at most the bound at alpha = 0.5 plus half the bound at alpha = 0."""
    q, d = inputs(B, M, H, scale)
    qg, dg = np.full(B, 9, dtype=np.int64), np.full(M, -1, dtype=np.int64)
    dg[pos:pos + B] = 9
    want, tol = bounds(q, d, pos, TEMP, 0.5, qg, dg)
    _, tol0 = bounds(q, d, pos, TEMP, 0.0, qg, dg)
    half, zero = call_abi(q, d, pos, 0.5, qg, dg), call_abi(q, d, pos, 0.0, qg, dg)
    within(flat(half), want, tol)
    assert want[2] == 0.0 and half[1][1].tobytes() == np.float32(0.0).tobytes() and zero[1][1].tobytes() == np.float32(0.0).tobytes()
    for name, x, y, t in (("loss", half[0], zero[0], tol[0] + 0.5 * tol0[0]), ("dq", half[2], zero[2], tol[3] + 0.5 * tol0[3]),
                          ("ddocs", half[3], zero[3], tol[4] + 0.5 * tol0[4])):
        e = float(np.abs(x.astype(np.float64) - 0.5 * y.astype(np.float64)).max())
        print(f"{name}: differs from half the alpha = 0 result by {e:.3e} / allowed {t:.3e}")
        assert e <= t, name


def test_rows_shorter_than_eps_are_divided_by_eps_in_both_directions():
    """One all-zero query and one all-zero positive: their images are zero, every logit with them is 0 in the row and in the
    column softmax, and the gradient with respect to them is the image's gradient over eps."""
    B, M, pos, H = 5, 14, 6, 32
    q, d = rows(710, B, H).copy(), rows(711, M, H).copy()
    q[1] = 0.0
    d[pos + 3] = 0.0
    for alpha in (0.5, 1.0):
        want, tol = bounds(q, d, pos, TEMP, alpha)
        within(flat(call_abi(q, d, pos, alpha)), want, tol)
        assert np.abs(want[3][1]).max() > 1e6 and np.abs(want[4][pos + 3]).max() > 1e6     # (the case is what it claims to be)


def test_same_bits_whatever_workspace_and_outputs_held_and_in_a_replayed_graph():
    """Labels a at the shape with several slices on every side.  Workspace and outputs filled with NaN words or with zeros
    (tests/poison.py): the same bits; a second call: the same bits; the loss-only call: the same loss and loss_dirs bits; the
    call captured in a graph over other inputs and replayed after the inputs are rewritten: the same bits."""
    from twotowermlretrieval_amd import _lib
    B, M, pos, H = 1025, 2060, 5, 32
    assert ib_slices(B, B)[1] > 1 and ib_slices(M, B)[1] > 1 and ib_slices(B, M)[1] > 1
    q, d = inputs(B, M, H, 1.0)
    qg, dg = labels("a", B, M, pos)
    out = {}
    for word in (0xFFFFFFFF, CONTROL):
        with poisoned_empty(word) as p:
            out[word] = call_abi(q, d, pos, 0.5, qg, dg)
            again = call_abi(q, d, pos, 0.5, qg, dg)
            alone = call_abi(q, d, pos, 0.5, qg, dg, grads=False)
            no_dirs = call_abi(q, d, pos, 0.5, qg, dg, dirs=False)
        assert p.tensors >= 12
        assert all(x.tobytes() == y.tobytes() for x, y in zip(out[word], again))
        assert alone[0].tobytes() == out[word][0].tobytes() and alone[1].tobytes() == out[word][1].tobytes()
        assert all(no_dirs[k].tobytes() == out[word][k].tobytes() for k in (0, 2, 3))
    for x, y in zip(out[0xFFFFFFFF], out[CONTROL]):
        assert np.isfinite(x).all() and x.tobytes() == y.tobytes()
    # ---- captured over other inputs, replayed over these
    L = _lib.lib()
    tq, td = dev(inputs(B, M, H, 30.0)[0]), dev(inputs(B, M, H, 30.0)[1][::-1])
    tqg, tdg = torch.full((B,), -1, dtype=torch.int64, device="cuda"), torch.full((M,), -1, dtype=torch.int64, device="cuda")
    loss, both = torch.zeros(1, device="cuda"), torch.zeros(2, device="cuda")
    dq, dd = torch.zeros_like(tq), torch.zeros_like(td)
    need = L.tt_contrastive_loss_sym_workspace_bytes(B, M, H)
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")

    def launch():
        _lib.check(L.tt_contrastive_loss_sym_f32(tq.data_ptr(), B, td.data_ptr(), M, H, pos, tqg.data_ptr(), tdg.data_ptr(), TEMP, 0.5,
                                                 loss.data_ptr(), both.data_ptr(), dq.data_ptr(), dd.data_ptr(), ws.data_ptr(), need,
                                                 torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launch()
    graph.replay()
    torch.cuda.synchronize()
    assert loss.cpu().numpy().tobytes() != out[CONTROL][0].tobytes()
    for t, a in ((tq, q), (td, d), (tqg, qg), (tdg, dg)):
        t.copy_(dev(a))
    for fill in (0xFF, 0x00):
        for t in (loss, both, dq, dd):
            t.fill_(float("nan"))
        ws.fill_(fill)
        graph.replay()
        torch.cuda.synchronize()
        for x, y in zip((loss, both, dq, dd), out[CONTROL]):
            assert x.cpu().numpy().tobytes() == y.tobytes()


def test_python_losses_take_the_entry():
    import twotowermlretrieval_amd as tt
    B, M, pos, H = 33, 70, 30, 32
    q, d = inputs(B, M, H, 1.0)
    qg, dg = labels("a", B, M, pos)
    for lab in ((None, None), (qg, dg)):
        direct = call_abi(q, d, pos, 0.25, *lab)
        kw = {} if lab[0] is None else dict(q_groups=dev(lab[0]), doc_groups=dev(lab[1]))
        t = [dev(a).requires_grad_(True) for a in (q, d)]
        loss = tt.contrastive_softmax_loss(t[0], t[1], pos_offset=pos, temperature=TEMP, symmetric=0.25, **kw)
        assert loss.dim() == 0
        (3 * loss).backward()
        both = tt.symmetric_contrastive_losses(t[0], t[1], pos_offset=pos, temperature=TEMP, **kw)
        torch.cuda.synchronize()
        assert np.float32(loss.item()).tobytes() == direct[0].tobytes()
        for x, g in zip(t, direct[2:]):
            assert np.array_equal(x.grad.cpu().numpy(), np.float32(3.0) * g)
        assert not both[0].requires_grad and both[0].dim() == 0
        assert np.float32(both[0].item()).tobytes() == direct[1][0:1].tobytes()
        assert np.float32(both[1].item()).tobytes() == direct[1][1:2].tobytes()
    # symmetric=0.0 (and the integer 0) is the one-directional call
    plain = call_plain(q, d, pos, TEMP)
    for zero in (0.0, 0):
        assert np.float32(tt.contrastive_softmax_loss(dev(q), dev(d), pos_offset=pos, temperature=TEMP,
                                                      symmetric=zero).item()).tobytes() == plain[0].tobytes()
    # in_batch_softmax_loss: the pool form on [p; n], with and without labels
    p, n = inputs(B, B, H, 1.0)[1], inputs(B, B + 1, H, 1.0)[1][:B]
    g = qg.copy()
    for groups, doc_labels in ((None, None), (g, np.concatenate([g, np.full(B, -1)]))):
        want = call_abi(q, np.concatenate([p, n]), 0, 0.5, groups, doc_labels)
        tt3 = [dev(a).requires_grad_(True) for a in (q, p, n)]
        loss = tt.in_batch_softmax_loss(tt3, temperature=TEMP, groups=None if groups is None else dev(groups), symmetric=0.5)
        loss.backward()
        torch.cuda.synchronize()
        assert np.float32(loss.item()).tobytes() == want[0].tobytes()
        assert np.array_equal(tt3[0].grad.cpu().numpy(), want[2])
        assert np.array_equal(torch.cat((tt3[1].grad, tt3[2].grad)).cpu().numpy(), want[3])
    with pytest.raises(ValueError, match="symmetric="):
        tt.contrastive_softmax_loss(dev(q), dev(d), symmetric=1.5)
