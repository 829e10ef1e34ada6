"""Grouped negatives (tt_contrastive_loss_grouped_f32, contrastive_softmax_loss(q_groups=, doc_groups=)) against the float64
statement (tests/grouped_loss_ref.py), and bit for bit against tt_contrastive_loss_f32 where no label matches.

The shapes are the classes of tests/test_pool_loss_gpu.py that reach ragged tiles, several query-side slices and several
document-side slices (the table there); a slice is `per` chunks of 128 documents (ib_slices).  Label patterns:

    a  groups of 3 consecutive queries share a label, and all their positives carry it
    b  every row of one whole slice carries query 0's label: that slice holds no kept document for query 0
    c  one label on every query and every row: every query keeps its positive alone -- loss rows 0.0, all gradients zero
    d  labels 2^40 + i; rows that carry the low 32 bits alone must not match
    e  equal NEGATIVE labels on both sides: no group, nothing matches

Bound per result (loss, dq, ddocs): grouped_loss_ref.bounds, the rule of pool_loss_ref.bounds."""
import functools

import numpy as np
import pytest
import torch

import pool_loss_ref
from grouped_loss_ref import bounds
from poison import CONTROL, poisoned_empty
from test_pool_loss_gpu import call_abi as call_plain, dev, ib_slices, rows

pytestmark = pytest.mark.gpu

TEMP = 0.05
NAMES = ("loss", "dq", "ddocs")


def call_abi(q, docs, pos_offset, qg, dg, temperature=TEMP, grads=True):
    """The grouped C entry on device copies; loss, gradients and workspace come from torch.empty (poisoned_empty fills them).
    Returns (loss [1], dq, ddocs) as numpy (the gradients None without `grads`)."""
    from twotowermlretrieval_amd import _lib
    L = _lib.lib()
    (B, H), M = q.shape, docs.shape[0]
    tq, td, tqg, tdg = dev(q), dev(docs), dev(np.asarray(qg, dtype=np.int64)), dev(np.asarray(dg, dtype=np.int64))
    assert tqg.shape == (B,) and tdg.shape == (M,)
    loss = torch.empty(1, dtype=torch.float32, device="cuda")
    g = [torch.empty_like(t) for t in (tq, td)] if grads else [None] * 2
    need = L.tt_contrastive_loss_workspace_bytes(B, M, H)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
    _lib.check(L.tt_contrastive_loss_grouped_f32(tq.data_ptr(), B, td.data_ptr(), M, H, pos_offset, tqg.data_ptr(), tdg.data_ptr(),
                                                 float(temperature), loss.data_ptr(), ptr(g[0]), ptr(g[1]), ws.data_ptr(), need,
                                                 torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return (loss.cpu().numpy(),) + tuple(t.cpu().numpy() if t is not None else None for t in g)


#          B     M   pos   H   scale
SHAPES = [(1, 2, 1, 32, 30.0),
          (33, 33, 0, 96, 1.0e-3),
          (17, 130, 113, 256, 30.0),
          (65, 1040, 390, 96, 1.0e-3),
          (3, 1025, 1022, 32, 1.0),
          (1025, 2060, 5, 32, 1.0e-3)]


@functools.lru_cache(maxsize=None)
def inputs(B, M, H, scale):
    """The rows of a shape, made once and shared (no test writes to them)."""
    return rows(17 * B + M, B, H, scale), rows(17 * B + M + 1, M, H, scale)


def empty_slice(B, M, pos):
    """(first row, rows) of a slice of the documents that does not hold query 0's positive; the only slice when there is one."""
    per, n = ib_slices(M, B)
    width = per * 128
    s = 0 if (n == 1 or pos // width != 0) else 1
    return s * width, min(width, M - s * width), n


def labels(pattern, B, M, pos):
    i, j = np.arange(B, dtype=np.int64), np.arange(M, dtype=np.int64)
    if pattern == "a":
        qg, dg = i // 3, np.full(M, -1, dtype=np.int64)
        dg[pos:pos + B] = qg
    elif pattern == "b":
        qg, dg = 1000 + i, np.full(M, -1, dtype=np.int64)
        dg[pos:pos + B] = qg
        lo, n_rows, _ = empty_slice(B, M, pos)
        dg[lo:lo + n_rows] = qg[0]
    elif pattern == "c":
        qg, dg = np.full(B, 5, dtype=np.int64), np.full(M, 5, dtype=np.int64)
    elif pattern == "d":
        qg = (1 << 40) + i
        dg = np.where(j % 2 == 1, (1 << 40) + j % B, j % B)           # odd rows: a real match; even rows: the low bits alone
        dg[pos:pos + B] = qg
    else:
        qg, dg = np.full(B, -2, dtype=np.int64), np.full(M, -2, dtype=np.int64)
    return qg, dg


def check(q, d, pos, qg, dg, temperature=TEMP):
    want, tol = bounds(q, d, pos, temperature, qg, dg)
    got = call_abi(q, d, pos, qg, dg, temperature)
    got = (float(got[0][0]),) + got[1:]
    errs = [float(np.abs(np.asarray(g, dtype=np.float64) - np.asarray(w, dtype=np.float64)).max()) for g, w in zip(got, want)]
    print("  ".join(f"{name} err {e:.3e} / allowed {t:.3e} (max|want| {np.abs(w).max():.3e})"
                    for name, e, t, w in zip(NAMES, errs, tol, want)))
    for name, g, e, t in zip(NAMES, got, errs, tol):
        assert np.isfinite(g).all(), name
        assert e <= t, f"{name}: error {e:.3e} > {t:.3e}"
    return got, want


@pytest.mark.parametrize("pattern", list("abcde"))
@pytest.mark.parametrize("B,M,pos,H,scale", SHAPES, ids=[f"{s[0]}x{s[1]}+{s[2]}-H{s[3]}" for s in SHAPES])
def test_loss_and_gradients_vs_float64(B, M, pos, H, scale, pattern):
    q, d = inputs(B, M, H, scale)
    qg, dg = labels(pattern, B, M, pos)
    if pattern == "b":
        lo, n_rows, n = empty_slice(B, M, pos)
        assert n_rows > 0 and (n == 1 or not lo <= pos < lo + n_rows)       # (with several slices, one is empty for query 0)
    got, want = check(q, d, pos, qg, dg)
    if pattern == "c":
        assert want[0] == 0.0 and got[0] == 0.0 and not got[1].any() and not got[2].any()
    if pattern == "d" and M > B + 1:
        plain = pool_loss_ref.pool_loss(q, d, pos, TEMP)
        assert abs(plain[0] - want[0]) > 1e-6                                # (the labels of the case do mask something)
    if pattern == "e":
        plain = call_plain(q, d, pos, TEMP)
        assert plain[0].tobytes() == np.float32(got[0]).tobytes() and plain[1].tobytes() == got[1].tobytes()
        assert plain[2].tobytes() == got[2].tobytes()


@pytest.mark.parametrize("which", ["all_negative", "all_distinct"])
@pytest.mark.parametrize("B,M,pos,H", [(33, 66, 0, 96), (1025, 2060, 5, 32)])
def test_without_a_match_it_returns_the_bits_of_the_ungrouped_entry(B, M, pos, H, which):
    q, d = inputs(B, M, H, 1.0)
    if which == "all_negative":
        qg, dg = -1 - np.arange(B, dtype=np.int64) % 3, -1 - np.arange(M, dtype=np.int64) % 3      # (equal negatives abound)
    else:
        qg, dg = np.arange(B, dtype=np.int64), 10 ** 6 + np.arange(M, dtype=np.int64)
        dg[pos:pos + B] = qg                                                                    # (matches on the positives only)
    new, old = call_abi(q, d, pos, qg, dg), call_plain(q, d, pos, TEMP)
    for x, y in zip(new, old):
        assert np.isfinite(x).all() and x.tobytes() == y.tobytes()
    alone = call_abi(q, d, pos, qg, dg, grads=False)
    assert alone[0].tobytes() == old[0].tobytes()


def test_a_fully_masked_query_costs_nothing_beside_ordinary_ones():
    """Queries 0 and 40 see their label on every other row: row loss 0.0 (the mean is the other queries' alone) and an all-zero
    gradient row; a document ignored by them still receives the gradient of the others."""
    B, M, pos, H = 65, 1040, 390, 96
    q, d = inputs(B, M, H, 1.0)
    qg, dg = np.full(B, -1, dtype=np.int64), np.full(M, 7, dtype=np.int64)
    qg[[0, 40]] = 7
    got, want = check(q, d, pos, qg, dg)
    assert not got[1][0].any() and not got[1][40].any() and got[1][1].any()
    assert not want[1][0].any() and not want[1][40].any()
    assert (np.abs(got[2]).max(axis=1) > 0.0).all()          # (every document, the two queries' positives included)


def test_ignoring_rows_is_removing_them_from_the_pool():
    """One query tile (B = 32) whose queries share one mask: a whole document tile, a ragged run across a chunk boundary and
    single rows in front of and behind the positives.  The grouped result is the loss over the pool without those rows: checked
    against that pool's float64 statement within its bounds; the removed rows' gradients are exactly zero."""
    B, M, pos, H = 32, 300, 40, 96
    q, d = inputs(B, M, H, 1.0)
    gone = np.concatenate([[3, 17], np.arange(96, 128), np.arange(250, 263), [299]])
    assert not np.intersect1d(gone, np.arange(pos, pos + B)).size
    qg, dg = np.full(B, 3, dtype=np.int64), np.full(M, -1, dtype=np.int64)
    dg[gone] = 3
    keep = np.setdiff1d(np.arange(M), gone)
    pos_kept = pos - int((gone < pos).sum())
    want, tol = pool_loss_ref.bounds(q, d[keep], pos_kept, TEMP)
    got = call_abi(q, d, pos, qg, dg)
    plain = call_plain(q, np.ascontiguousarray(d[keep]), pos_kept, TEMP)
    assert not got[2][gone].any()
    for name, g, p, w, t in zip(NAMES, (float(got[0][0]), got[1], got[2][keep]), (float(plain[0][0]),) + plain[1:], want, tol):
        e = float(np.abs(np.asarray(g, dtype=np.float64) - w).max())
        ep = float(np.abs(np.asarray(p, dtype=np.float64) - w).max())
        print(f"{name}: grouped err {e:.3e}, ungrouped on the reduced pool err {ep:.3e} / allowed {t:.3e}")
        assert e <= t and ep <= t, name


def test_same_bits_whatever_workspace_and_outputs_held_and_in_a_replayed_graph():
    """Pattern a and an empty slice for query 0 together, at the shape with several slices on both sides.  Workspace, loss
    and gradient outputs filled with NaN words or with zeros (tests/poison.py): the same bits; a second call: the same bits;
    the loss-only call: the same loss bits; the call captured in a graph and replayed twice over poisoned buffers: the same bits."""
    from twotowermlretrieval_amd import _lib
    B, M, pos, H = 1025, 2060, 5, 32
    q, d = inputs(B, M, H, 1.0)
    qg, dg = labels("a", B, M, pos)
    lo, n_rows, n = empty_slice(B, M, pos)
    assert n > 1
    dg[lo:lo + n_rows] = qg[0]
    out = {}
    for word in (0xFFFFFFFF, CONTROL):
        with poisoned_empty(word) as p:
            out[word] = call_abi(q, d, pos, qg, dg)
            again = call_abi(q, d, pos, qg, dg)
            alone = call_abi(q, d, pos, qg, dg, grads=False)
        assert p.tensors >= 10
        assert all(x.tobytes() == y.tobytes() for x, y in zip(out[word], again)) and alone[0].tobytes() == out[word][0].tobytes()
    for x, y in zip(out[0xFFFFFFFF], out[CONTROL]):
        assert np.isfinite(x).all() and x.tobytes() == y.tobytes()
    # ---- captured and replayed
    L = _lib.lib()
    tq, td, tqg, tdg = dev(q), dev(d), dev(qg), dev(dg)
    loss = torch.zeros(1, device="cuda")
    dq, dd = torch.zeros_like(tq), torch.zeros_like(td)
    need = L.tt_contrastive_loss_workspace_bytes(B, M, H)
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")

    def launch():
        _lib.check(L.tt_contrastive_loss_grouped_f32(tq.data_ptr(), B, td.data_ptr(), M, H, pos, tqg.data_ptr(), tdg.data_ptr(), TEMP,
                                                     loss.data_ptr(), dq.data_ptr(), dd.data_ptr(), ws.data_ptr(), need,
                                                     torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launch()
    for fill in (0xFF, 0x00):
        for t in (loss, dq, dd):
            t.fill_(float("nan"))
        ws.fill_(fill)
        graph.replay()
        torch.cuda.synchronize()
        for x, y in zip((loss, dq, dd), out[CONTROL]):
            assert x.cpu().numpy().tobytes() == y.tobytes()


def test_autograd_gives_the_entrys_gradients_and_in_batch_takes_the_pool_entry():
    import twotowermlretrieval_amd as tt
    B, M, pos, H = 33, 70, 30, 32
    q, d = inputs(B, M, H, 1.0)
    qg, dg = labels("a", B, M, pos)
    direct = call_abi(q, d, pos, qg, dg)
    assert direct[0].tobytes() != call_plain(q, d, pos, TEMP)[0].tobytes()
    t = [dev(a).requires_grad_(True) for a in (q, d)]
    loss = tt.contrastive_softmax_loss(t[0], t[1], pos_offset=pos, temperature=TEMP, q_groups=dev(qg), doc_groups=dev(dg))
    assert loss.dim() == 0
    (3 * loss).backward()
    torch.cuda.synchronize()
    assert np.float32(loss.item()).tobytes() == direct[0].tobytes()
    for x, g in zip(t, direct[1:]):
        assert np.array_equal(x.grad.cpu().numpy(), np.float32(3.0) * g)
    # in_batch_softmax_loss: positives carry `groups`, negatives `neg_groups` (None: -1), over the pool [p; n]
    p, n = inputs(B, B, H, 1.0)[1], inputs(B, B + 1, H, 1.0)[1][:B]
    g, ng = qg.copy(), np.where(np.arange(B) % 4 == 0, qg, -1)
    for neg, doc_labels in ((None, np.concatenate([g, np.full(B, -1)])), (ng, np.concatenate([g, ng]))):
        want = call_abi(q, np.concatenate([p, n]), 0, g, doc_labels)
        tt3 = [dev(a).requires_grad_(True) for a in (q, p, n)]
        loss = tt.in_batch_softmax_loss(tt3, temperature=TEMP, groups=dev(g), neg_groups=None if neg is None else dev(neg))
        loss.backward()
        torch.cuda.synchronize()
        assert np.float32(loss.item()).tobytes() == want[0].tobytes()
        assert np.array_equal(tt3[0].grad.cpu().numpy(), want[1])
        assert np.array_equal(torch.cat((tt3[1].grad, tt3[2].grad)).cpu().numpy(), want[2])


def test_python_entries_name_the_label_argument_they_refuse():
    import twotowermlretrieval_amd as tt
    q, d = torch.ones((4, 32), device="cuda"), torch.ones((9, 32), device="cuda")
    qg, dg = torch.zeros(4, dtype=torch.int64, device="cuda"), torch.zeros(9, dtype=torch.int64, device="cuda")
    for kw in (dict(q_groups=qg), dict(doc_groups=dg)):
        with pytest.raises(ValueError, match="both given or both None"):
            tt.contrastive_softmax_loss(q, d, **kw)
    for bad in (qg.int(), qg[:3], qg[None], qg.cpu(), qg.double(), [0, 0, 0, 0]):
        with pytest.raises(ValueError, match="q_groups must be"):
            tt.contrastive_softmax_loss(q, d, q_groups=bad, doc_groups=dg)
    for bad in (dg.int(), dg[:4], dg.cpu()):
        with pytest.raises(ValueError, match="doc_groups must be"):
            tt.contrastive_softmax_loss(q, d, q_groups=qg, doc_groups=bad)
    with pytest.raises(ValueError, match="neg_groups must be"):
        tt.in_batch_softmax_loss((q, q, q), groups=qg, neg_groups=qg.int())
    with pytest.raises(ValueError, match="groups must be"):
        tt.in_batch_softmax_loss((q, q, q), groups=dg)
    assert tt.contrastive_softmax_loss(q, d, pos_offset=5, q_groups=qg, doc_groups=dg).item() == 0.0      # (all rows share the label)
