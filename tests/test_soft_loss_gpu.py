"""Soft targets (tt_contrastive_loss_soft_f32, soft_contrastive_loss) against the float64 statement (tests/soft_loss_ref.py), bit
for bit against tt_contrastive_loss_f32 on one-hot targets, and exact zeros for all-zero target rows.

The shapes are those of tests/test_grouped_loss_gpu.py (ragged tiles, several query-side slices, several document-side slices)
plus (31, 4099): 7 slices of 5 chunks folded per query.  A slice is `per` chunks of 128 documents (ib_slices).  Target patterns:

    a  one-hot at pos + i: the bits of the pooled entry, with and without gradients
    b  dense: softmax(3 * randn) per row
    c  three weights of 1/3 per query: in column M - 1, in the ragged last tile, and in a slice other than the one of pos + i
       (where the shape has one slice or one tile they fall together and add up)
    d  sparse non-negative weights with row sums != 1; queries 0 and B - 1 all zero: exact zeros
    e  pattern b with one negative weight per row

Bound per result (loss, dq, ddocs) for b-e: soft_loss_ref.bounds, the rule of pool_loss_ref.bounds."""
import functools

import numpy as np
import pytest
import torch

from poison import CONTROL, poisoned_empty
from soft_loss_ref import bounds, soft_loss
from test_grouped_loss_gpu import SHAPES as GROUPED_SHAPES, inputs
from test_pool_loss_gpu import call_abi as call_plain, dev, ib_slices

pytestmark = pytest.mark.gpu

TEMP = 0.05
NAMES = ("loss", "dq", "ddocs")
#          B     M   pos   H   scale
SHAPES = GROUPED_SHAPES + [(31, 4099, 2000, 20, 1.0)]
IDS = [f"{s[0]}x{s[1]}+{s[2]}-H{s[3]}" for s in SHAPES]


def call_abi(q, docs, targets, temperature=TEMP, grads=True):
    """The soft C entry on device copies; loss, gradients and workspace come from torch.empty (poisoned_empty fills them).
    Returns (loss [1], dq, ddocs) as numpy (the gradients None without `grads`)."""
    from twotowermlretrieval_amd import _lib
    L = _lib.lib()
    (B, H), M = q.shape, docs.shape[0]
    tq, td, tt = dev(q), dev(docs), targets if isinstance(targets, torch.Tensor) else dev(np.asarray(targets, dtype=np.float32))
    assert tt.shape == (B, M) and tt.dtype == torch.float32 and tt.is_contiguous()
    loss = torch.empty(1, dtype=torch.float32, device="cuda")
    g = [torch.empty_like(t) for t in (tq, td)] if grads else [None] * 2
    need = L.tt_contrastive_loss_soft_workspace_bytes(B, M, H)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
    _lib.check(L.tt_contrastive_loss_soft_f32(tq.data_ptr(), B, td.data_ptr(), M, H, tt.data_ptr(), float(temperature),
                                              loss.data_ptr(), ptr(g[0]), ptr(g[1]), ws.data_ptr(), need,
                                              torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return (loss.cpu().numpy(),) + tuple(t.cpu().numpy() if t is not None else None for t in g)


def one_hot(B, M, pos):
    t = np.zeros((B, M), dtype=np.float32)
    t[np.arange(B), pos + np.arange(B)] = 1.0
    return t


def dense(seed, B, M):
    z = 3.0 * np.random.RandomState(seed).standard_normal((B, M))
    e = np.exp(z - z.max(axis=1, keepdims=True))
    return (e / e.sum(axis=1, keepdims=True)).astype(np.float32)


def other_slice_column(B, M, pos, i):
    """A column in a slice of the documents other than the one that holds pos + i (column 0 of the next slice, cyclically); with
    one slice, column 0."""
    per, n = ib_slices(M, B)
    width = per * 128
    return ((pos + i) // width + 1) % n * width


@functools.lru_cache(maxsize=None)
def targets(pattern, B, M, pos):
    """The targets of a (pattern, shape), made once and shared (no test writes to them)."""
    rs = np.random.RandomState(1000 + 7 * B + M + ord(pattern))
    i = np.arange(B)
    if pattern == "a":
        t = one_hot(B, M, pos)
    elif pattern == "b":
        t = dense(5 * B + M, B, M)
    elif pattern == "c":
        t = np.zeros((B, M), dtype=np.float32)
        third = np.float32(1.0) / np.float32(3.0)
        ragged = (M - 1) // 32 * 32 + (i % ((M - 1) % 32 + 1))          # (a column of the last, ragged document tile)
        for cols in (np.full(B, M - 1), ragged, np.array([other_slice_column(B, M, pos, k) for k in i])):
            np.add.at(t, (i, cols), third)
    elif pattern == "d":
        t = (rs.random_sample((B, M)) * 2.5).astype(np.float32) * (rs.random_sample((B, M)) < 0.05)
        t[i, rs.randint(0, M, B)] += np.float32(0.75)                    # (no row empty by chance)
        t[0] = 0.0
        t[B - 1] = 0.0
        t = t.astype(np.float32)
    else:
        t = dense(5 * B + M, B, M)
        t[i, rs.randint(0, M, B)] = np.float32(-0.2)
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def reference(pattern, B, M, pos, H, scale):
    q, d = inputs(B, M, H, scale)
    return bounds(q, d, targets(pattern, B, M, pos), TEMP)


def check(got, want, tol):
    got = (float(got[0][0]),) + tuple(got[1:])
    errs = [float(np.abs(np.asarray(g, dtype=np.float64) - np.asarray(w, dtype=np.float64)).max()) for g, w in zip(got, want)]
    print("  ".join(f"{name} err {e:.3e} / allowed {t:.3e} (max|want| {np.abs(w).max():.3e})"
                    for name, e, t, w in zip(NAMES, errs, tol, want)))
    for name, g, e, t in zip(NAMES, got, errs, tol):
        assert np.isfinite(g).all(), name
        assert e <= t, f"{name}: error {e:.3e} > {t:.3e}"
    return got


@pytest.mark.parametrize("B,M,pos,H,scale", SHAPES, ids=IDS)
def test_one_hot_targets_give_the_bits_of_the_pooled_entry(B, M, pos, H, scale):
    q, d = inputs(B, M, H, scale)
    t = targets("a", B, M, pos)
    new, old = call_abi(q, d, t), call_plain(q, d, pos, TEMP)
    for name, x, y in zip(NAMES, new, old):
        assert np.isfinite(x).all() and x.tobytes() == y.tobytes(), name
    alone, old_alone = call_abi(q, d, t, grads=False), call_plain(q, d, pos, TEMP, grads=False)
    assert alone[0].tobytes() == old[0].tobytes() == old_alone[0].tobytes()


@pytest.mark.parametrize("pattern", list("bcde"))
@pytest.mark.parametrize("B,M,pos,H,scale", SHAPES, ids=IDS)
def test_loss_and_gradients_vs_float64(B, M, pos, H, scale, pattern):
    q, d = inputs(B, M, H, scale)
    t = targets(pattern, B, M, pos)
    want, tol = reference(pattern, B, M, pos, H, scale)
    got = check(call_abi(q, d, t), want, tol)
    alone = call_abi(q, d, t, grads=False)
    assert alone[0].tobytes() == np.float32(got[0]).tobytes()
    if pattern == "c":
        assert np.allclose(t.sum(axis=1), 1.0, atol=1e-6) and (t[:, M - 1] > 0).all()
        if ib_slices(M, B)[1] > 1:
            width = ib_slices(M, B)[0] * 128
            assert all((np.flatnonzero(t[k]) // width != (pos + k) // width).any() for k in range(B))
    if pattern == "d":
        # property 2: an all-zero target row has no loss and no gradient; with B = 1 that is the whole call
        assert not got[1][0].any() and not got[1][B - 1].any() and not want[1][0].any()
        if B == 1:
            assert got[0] == 0.0 and want[0] == 0.0 and not got[2].any()
        else:
            assert got[1][1:B - 1].any()
    if pattern == "e":
        assert (t < 0).sum(axis=1).tolist() == [1] * B


def test_all_zero_targets_cost_exactly_nothing():
    B, M, pos, H, scale = SHAPES[3]
    q, d = inputs(B, M, H, 1.0)
    got = call_abi(q, d, np.zeros((B, M), dtype=np.float32))
    assert got[0][0] == 0.0 and not got[1].any() and not got[2].any()
    # queries 0 and 40 carry no weight beside ordinary ones: zero dq rows there and nowhere else
    t = np.zeros((B, M), dtype=np.float32)
    t[1:40, 7] = 0.5
    t[41:, 9] = 2.0
    a = call_abi(q, d, t)
    assert not a[1][0].any() and not a[1][40].any() and (np.abs(np.delete(a[1], [0, 40], axis=0)).max(axis=1) > 0.0).all()
    want, tol = bounds(q, d, t, TEMP)
    assert not want[1][0].any() and not want[1][40].any()
    check(a, want, tol)


def test_same_bits_whatever_workspace_and_outputs_held_and_nothing_else_is_written():
    """Dense targets at the shape with several slices on both sides.  Workspace, loss and gradient outputs filled with NaN words
    or with zeros (tests/poison.py): the same bits; a second call: the same bits; the loss-only call: the same loss bits.  The
    inputs and the bytes behind the workspace's end are what they were."""
    from twotowermlretrieval_amd import _lib
    B, M, pos, H, scale = SHAPES[5]
    q, d = inputs(B, M, H, 1.0)
    t = targets("b", B, M, pos)
    out = {}
    for word in (0xFFFFFFFF, CONTROL):
        with poisoned_empty(word) as p:
            out[word] = call_abi(q, d, t)
            again = call_abi(q, d, t)
            alone = call_abi(q, d, t, grads=False)
        assert p.tensors >= 10
        assert all(x.tobytes() == y.tobytes() for x, y in zip(out[word], again)) and alone[0].tobytes() == out[word][0].tobytes()
    for x, y in zip(out[0xFFFFFFFF], out[CONTROL]):
        assert np.isfinite(x).all() and x.tobytes() == y.tobytes()
    # ---- guard bytes around every buffer the call writes, and the inputs afterwards
    L = _lib.lib()
    need = L.tt_contrastive_loss_soft_workspace_bytes(B, M, H)
    tq, td, tt = dev(q), dev(d), dev(t)
    G = 256

    def guarded(nbytes):
        raw = torch.full((G + nbytes + G,), 0xA5, dtype=torch.uint8, device="cuda")
        return raw, raw[G:G + nbytes]
    bufs = {name: guarded(n) for name, n in (("loss", 4), ("dq", 4 * B * H), ("ddocs", 4 * M * H), ("ws", need))}
    _lib.check(L.tt_contrastive_loss_soft_f32(tq.data_ptr(), B, td.data_ptr(), M, H, tt.data_ptr(), TEMP, bufs["loss"][1].data_ptr(),
                                              bufs["dq"][1].data_ptr(), bufs["ddocs"][1].data_ptr(), bufs["ws"][1].data_ptr(), need,
                                              torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    for name, (raw, _) in bufs.items():
        assert (raw[:G] == 0xA5).all() and (raw[-G:] == 0xA5).all(), name
    for name, x in zip(NAMES, out[CONTROL]):
        assert bufs[name][1].cpu().numpy().tobytes() == x.tobytes(), name
    assert np.array_equal(tq.cpu().numpy(), q) and np.array_equal(td.cpu().numpy(), d) and np.array_equal(tt.cpu().numpy(), t)


def test_captured_in_a_graph_and_replayed_over_rewritten_targets():
    from twotowermlretrieval_amd import _lib
    B, M, pos, H, scale = SHAPES[5]
    q, d = inputs(B, M, H, 1.0)
    L = _lib.lib()
    tq, td = dev(q), dev(d)
    tt = torch.zeros((B, M), dtype=torch.float32, device="cuda")
    loss = torch.zeros(1, device="cuda")
    dq, dd = torch.zeros_like(tq), torch.zeros_like(td)
    need = L.tt_contrastive_loss_soft_workspace_bytes(B, M, H)
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")

    def launch():
        _lib.check(L.tt_contrastive_loss_soft_f32(tq.data_ptr(), B, td.data_ptr(), M, H, tt.data_ptr(), TEMP, loss.data_ptr(),
                                                  dq.data_ptr(), dd.data_ptr(), ws.data_ptr(), need,
                                                  torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launch()
    for pattern, fill in (("b", 0xFF), ("d", 0x00), ("a", 0xFF)):
        t = targets(pattern, B, M, pos)
        want = call_abi(q, d, t) if pattern != "a" else call_plain(q, d, pos, TEMP)
        tt.copy_(dev(t))
        for x in (loss, dq, dd):
            x.fill_(float("nan"))
        ws.fill_(fill)
        graph.replay()
        torch.cuda.synchronize()
        for name, x, y in zip(NAMES, (loss, dq, dd), want):
            assert x.cpu().numpy().tobytes() == y.tobytes(), (pattern, name)


def test_autograd_gives_the_entrys_gradients_and_targets_get_none():
    import twotowermlretrieval_amd as tt
    B, M, pos, H = 33, 70, 30, 32
    q, d = inputs(B, M, H, 1.0)
    t = targets("e", B, M, pos)
    direct = call_abi(q, d, t)
    x = [dev(a).requires_grad_(True) for a in (q, d)]
    tg = dev(t).requires_grad_(True)
    loss = tt.soft_contrastive_loss(x[0], x[1], tg, temperature=TEMP)
    assert loss.dim() == 0
    (3 * loss).backward()
    torch.cuda.synchronize()
    assert np.float32(loss.item()).tobytes() == direct[0].tobytes() and tg.grad is None
    for a, g in zip(x, direct[1:]):
        assert np.array_equal(a.grad.cpu().numpy(), np.float32(3.0) * g)
    # the builders' targets go straight in: one-hot from labels that match nothing is the pooled loss, bit for bit
    none = torch.full((B,), -1, dtype=torch.int64, device="cuda"), torch.full((M,), -1, dtype=torch.int64, device="cuda")
    a = tt.soft_contrastive_loss(x[0], x[1], tt.multi_positive_targets(*none, pos), temperature=TEMP)
    b = tt.contrastive_softmax_loss(x[0], x[1], pos_offset=pos, temperature=TEMP)
    assert np.float32(a.item()).tobytes() == np.float32(b.item()).tobytes()
    teacher = torch.randn((B, M), generator=torch.Generator().manual_seed(3)).cuda()
    c = tt.soft_contrastive_loss(x[0], x[1], tt.distillation_targets(teacher, 0.5), temperature=TEMP)
    want = soft_loss(q, d, tt.distillation_targets(teacher, 0.5).cpu().numpy(), TEMP)[0]
    assert abs(c.item() - want) <= 1e-5 * abs(want)


def test_python_entry_names_the_argument_it_refuses():
    import twotowermlretrieval_amd as tt
    q, d, t = torch.ones((4, 32), device="cuda"), torch.ones((9, 32), device="cuda"), torch.zeros((4, 9), device="cuda")
    for bad in (t.double(), t[:3], t[:, :8], t[None], t.cpu(), t.long(), [[0.0] * 9] * 4, None):
        with pytest.raises(ValueError, match=r"targets must be a float32 tensor \[4, 9\]"):
            tt.soft_contrastive_loss(q, d, bad)
    with pytest.raises(ValueError, match="temperature"):
        tt.soft_contrastive_loss(q, d, t, temperature=0.0)
    with pytest.raises(ValueError, match="M=3 documents for B=4"):
        tt.soft_contrastive_loss(q, d[:3], t[:, :3])
    assert tt.soft_contrastive_loss(q, d, t).item() == 0.0
    assert tt.soft_contrastive_loss(q, d, t.t().contiguous().t()).item() == 0.0           # (a strided view is made contiguous)


def test_past_2_to_32_target_elements():
    """B = M = 65 600: element i * M + j passes 2^31 at row 32 737 and 2^32 at row 65 473.  The targets are zeros but for six
    planted rows -- the first, the two on either side of each boundary, the last -- with weights in columns 0, M - 1 and three
    more.  Every other row is all zeros: exactly nothing (property 2), so the float64 statement over the planted rows alone,
    scaled by planted / B, is the whole result; every other dq row is asserted all-zero.  An index formed in 32 bits would
    read the zeros (or other rows' weights) of a wrapped offset."""
    B = M = 65600
    H = 32
    q, d = inputs(B, M, H, 1.0)
    up = lambda n: -(-n // M)  # noqa: E731
    planted = [0, up(2 ** 31) - 1, up(2 ** 31), up(2 ** 32) - 1, up(2 ** 32), B - 1]
    assert planted == sorted(set(planted)) and (planted[2] * M >= 2 ** 31 > planted[1] * M) and (planted[4] * M >= 2 ** 32 > planted[3] * M)
    rs = np.random.RandomState(9)
    small = np.zeros((len(planted), M), dtype=np.float32)
    for k, i in enumerate(planted):
        cols = np.unique(np.concatenate([[0, M - 1, i], rs.randint(1, M - 1, 2)]))
        small[k, cols] = (0.25 + rs.random_sample(cols.size)).astype(np.float32)
    tt = torch.zeros((B, M), dtype=torch.float32, device="cuda")
    tt[torch.tensor(planted, device="cuda")] = dev(small)
    got = call_abi(q, d, tt)
    del tt
    want, tol = bounds(q[planted], d, small, TEMP)
    k = len(planted) / B
    want, tol = tuple(np.asarray(w) * k for w in want), [t * k for t in tol]
    others = np.setdiff1d(np.arange(B), planted)
    assert not got[1][others].any()
    check((got[0], got[1][planted], got[2]), (float(want[0]), want[1], want[2]), tol)
    assert all(np.abs(got[1][i]).max() > 0.0 for i in planted)
