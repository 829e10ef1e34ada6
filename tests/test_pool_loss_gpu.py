"""Softmax contrastive loss over a pool of documents (tt_contrastive_loss_f32, contrastive_softmax_loss) against its float64
statement (tests/pool_loss_ref.py), and bit for bit against tt_in_batch_loss_f32 where the two meet (docs = [p; n]).

The kernels are K9's (tests/test_in_batch_loss_gpu.py): a workgroup owns 32 queries or 32 documents and walks the other side in
chunks of 128 rows, cut into at most 8 slices of whole chunks (ib_slices, restated below).  Q = slices x chunks of the documents
a query tile walks, D = the same of the queries a document tile walks:

     B     M   pos_offset    H    Q       D       what it reaches
     1     1        0       20    1 x 1   1 x 1   only the positive
     1     2        1       32    1 x 1   1 x 1   positive in the last column
    33    33        0       96    1 x 1   1 x 1   M = B, no explicit negatives, one row past a tile
    32    96       64      512    1 x 1   1 x 1   positive block = exactly the last document tile
    17   130      113      256    2 x 1   1 x 1   positive block ends in the ragged tile past a 128-row chunk
    65  1040      390       96    5 x 2   1 x 1   world 8 x 2 * 65, rank 3: positives outside slice 0
     3  1025     1022       32    5 x 2   1 x 1   few queries, 33 document tiles, positives at the pool's end
    31  4099     2000       20    7 x 5   1 x 1   35 chunk places folded by the online softmax
  1025  2060        5       32    6 x 3   3 x 3   the only class with several document-side slices
   512  8192     3072      256    8 x 8   1 x 4   the 8-rank product shape

Bound per result (loss, dq, ddocs): 4 x the error of the helper itself evaluated in float32 at that very shape, plus
4 * 2^-24 * max|want| (pool_loss_ref.bounds, the rule of in_batch_ref.bounds)."""
import copy

import numpy as np
import pytest
import torch

import synth
from poison import CONTROL, poisoned_empty
from pool_loss_ref import bounds

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def ib_slices(walked_rows, owner_rows):
    """(chunks per slice, slices): the rule of csrc/in_batch_loss.hip, restated."""
    chunks, tiles = -(-walked_rows // 128), -(-owner_rows // 32)
    want = min(max(256 // tiles, 1), 8, chunks)
    per = -(-chunks // want)
    return per, -(-chunks // per)


def call_abi(q, docs, pos_offset, temperature, grads=True, fill=None):
    """The C entry on device copies.  fill: byte the workspace holds on entry (None: whatever the allocator gave).
    Returns (loss [1], dq, ddocs) as numpy (the gradients None without `grads`)."""
    from twotowermlretrieval_amd import _lib
    L = _lib.lib()
    (B, H), M = q.shape, docs.shape[0]
    tq, td = dev(q), dev(docs)
    loss = torch.full((1,), float("nan"), device="cuda")
    g = [torch.full_like(t, float("nan")) for t in (tq, td)] if grads else [None] * 2
    need = L.tt_contrastive_loss_workspace_bytes(B, M, H)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    if fill is not None:
        ws.fill_(fill)
    ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
    _lib.check(L.tt_contrastive_loss_f32(tq.data_ptr(), B, td.data_ptr(), M, H, pos_offset, float(temperature), loss.data_ptr(),
                                         ptr(g[0]), ptr(g[1]), ws.data_ptr(), need, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return (loss.cpu().numpy(),) + tuple(t.cpu().numpy() if t is not None else None for t in g)


NAMES = ("loss", "dq", "ddocs")


def check(q, docs, pos_offset, temperature):
    want, tol = bounds(q, docs, pos_offset, temperature)
    got = call_abi(q, docs, pos_offset, temperature)
    got = (float(got[0][0]),) + got[1:]
    errs = [float(np.abs(np.asarray(g, dtype=np.float64) - np.asarray(w, dtype=np.float64)).max()) for g, w in zip(got, want)]
    print("  ".join(f"{name} err {e:.3e} / allowed {t:.3e} (max|want| {np.abs(w).max():.3e})"
                    for name, e, t, w in zip(NAMES, errs, tol, want)))
    for name, g, e, t in zip(NAMES, got, errs, tol):
        assert np.isfinite(g).all(), name
        assert e <= t, f"{name}: error {e:.3e} > {t:.3e}"
    return got, want


def rows(seed, n, H, scale=1.0):
    return (synth.unit_rows(seed, n, H) * np.float32(scale)).astype(np.float32)


#         B     M   pos   H   scale   Q (slices, chunks)  D
SHAPES = [(1, 1, 0, 20, 1.0, (1, 1), (1, 1)),
          (1, 2, 1, 32, 30.0, (1, 1), (1, 1)),
          (33, 33, 0, 96, 1.0e-3, (1, 1), (1, 1)),
          (32, 96, 64, 512, 1.0, (1, 1), (1, 1)),
          (17, 130, 113, 256, 30.0, (2, 1), (1, 1)),
          (65, 1040, 390, 96, 1.0e-3, (5, 2), (1, 1)),
          (3, 1025, 1022, 32, 1.0, (5, 2), (1, 1)),
          (31, 4099, 2000, 20, 30.0, (7, 5), (1, 1)),
          (1025, 2060, 5, 32, 1.0e-3, (6, 3), (3, 3)),
          (512, 8192, 3072, 256, 1.0, (8, 8), (1, 4))]


@pytest.mark.parametrize("B,M,pos_offset,H,scale,Q,D", SHAPES, ids=[f"{s[0]}x{s[1]}+{s[2]}-H{s[3]}" for s in SHAPES])
def test_loss_and_gradients_vs_float64(B, M, pos_offset, H, scale, Q, D):
    per, n = ib_slices(M, B)
    assert (n, per) == Q, (n, per)              # (the case reaches the class the table says it does)
    per, n = ib_slices(B, M)
    assert (n, per) == D, (n, per)
    assert pos_offset + B <= M
    check(rows(13 * B + M, B, H, scale), rows(13 * B + M + 1, M, H, scale), pos_offset, 0.05)


@pytest.mark.parametrize("B,H", [(33, 96), (65, 20), (1025, 256)])
def test_on_p_n_it_returns_the_bits_of_the_in_batch_entry(B, H):
    from test_in_batch_loss_gpu import call_abi as call_old
    q, p, n = (rows(500 + B + s, B, H) for s in range(3))
    old = call_old(q, p, n, 0.05)
    new = call_abi(q, np.concatenate([p, n]), 0, 0.05)
    assert np.isfinite(new[0]).all()
    assert new[0].tobytes() == old[0].tobytes() and new[1].tobytes() == old[1].tobytes()
    assert new[2][:B].tobytes() == old[2].tobytes() and new[2][B:].tobytes() == old[3].tobytes()


def test_logits_of_100_across_slices_do_not_overflow():
    """temperature = 0.01 and docs[pos_offset + i] = q_i on every third row: the logit is 100 and exp(100) is not a float32.  At
    (65, 1040, 390) the positives lie in slice 1 of 5 (documents 256..511): the maximum of such a row sits in another slice than
    slice 0, and ib_lse_kernel rescales across slices."""
    B, M, pos, H = 65, 1040, 390, 96
    assert ib_slices(M, B) == (2, 5) and pos // 256 >= 1
    q, d = rows(600, B, H).copy(), rows(601, M, H).copy()
    d[pos:pos + B:3] = q[::3]
    got, _ = check(q, d, pos, 0.01)
    assert np.isfinite(got[0])


def test_rows_shorter_than_eps_are_divided_by_eps():
    """One all-zero query and one all-zero document (a positive): their images are zero, every logit with them is 0, and the
    gradient with respect to them is the image's gradient over eps (the helper defines it)."""
    B, M, pos, H = 5, 14, 6, 32
    q, d = rows(610, B, H).copy(), rows(611, M, H).copy()
    q[1] = 0.0
    d[pos + 3] = 0.0
    got, want = check(q, d, pos, 0.05)
    assert np.abs(want[1][1]).max() > 1e6 and np.abs(want[2][pos + 3]).max() > 1e6     # (the case is what it claims to be)


def test_loss_alone_is_the_loss_of_the_full_call():
    B, M, pos, H = 33, 140, 100, 96
    q, d = rows(620, B, H), rows(621, M, H)
    full = call_abi(q, d, pos, 0.05)
    alone = call_abi(q, d, pos, 0.05, grads=False)
    assert alone[1] is None and alone[2] is None and np.isfinite(alone[0]).all()
    assert alone[0].tobytes() == full[0].tobytes()


def test_same_bits_whatever_the_workspace_held():
    B, M, pos, H = 65, 1040, 390, 96
    q, d = rows(630, B, H, 2.0), rows(631, M, H, 2.0)
    a = call_abi(q, d, pos, 0.05, fill=0xFF)
    b = call_abi(q, d, pos, 0.05, fill=0x00)
    for x, y in zip(a, b):
        assert np.isfinite(x).all() and x.tobytes() == y.tobytes()


def test_autograd_scales_the_kernel_gradients_by_the_incoming_scalar():
    import twotowermlretrieval_amd as tt
    B, M, pos, H = 33, 70, 30, 32
    q, d = rows(640, B, H), rows(641, M, H)
    direct = call_abi(q, d, pos, 0.05)
    t = [dev(a).requires_grad_(True) for a in (q, d)]
    loss = tt.contrastive_softmax_loss(t[0], t[1], pos_offset=pos, temperature=0.05)
    assert loss.dim() == 0
    (3 * loss).backward()
    torch.cuda.synchronize()
    assert np.float32(loss.item()).tobytes() == direct[0].tobytes()
    for x, g in zip(t, direct[1:]):
        assert np.array_equal(x.grad.cpu().numpy(), np.float32(3.0) * g)


def test_python_entry_validates_its_arguments():
    import twotowermlretrieval_amd as tt
    q, d = torch.zeros((4, 32), device="cuda"), torch.zeros((9, 32), device="cuda")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tt.contrastive_softmax_loss(q.cpu(), d)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tt.contrastive_softmax_loss(q, d.cpu())
    for bad in ((q.double(), d), (q, d.half()), (q[0], d), (q, d[None])):                # dtype, rank
        with pytest.raises(ValueError, match="float32"):
            tt.contrastive_softmax_loss(*bad)
    with pytest.raises(ValueError, match="H="):
        tt.contrastive_softmax_loss(q, d[:, :16])
    with pytest.raises(ValueError, match="M=3"):
        tt.contrastive_softmax_loss(q, d[:3])
    for pos in (-1, 6):
        with pytest.raises(ValueError, match="pos_offset"):
            tt.contrastive_softmax_loss(q, d, pos_offset=pos)
    for temp in (0.0, -0.05, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="temperature"):
            tt.contrastive_softmax_loss(q, d, temperature=temp)
    assert tt.contrastive_softmax_loss(q + 1.0, d + 1.0, pos_offset=5).dim() == 0         # (the last offset allowed)


# ---- whatever torch.empty returned ------------------------------------------------------------------------------------------
V, E, HM, BT = 80, 20, 32, 24
TEMP = 0.1


def small_model(seed=3):
    import twotowermlretrieval_amd as tt
    torch.manual_seed(seed)
    return tt.TwoTowerModel({"VOCAB_SIZE": V, "EMBED_DIM": E, "HIDDEN_DIM": HM, "NUM_LAYERS": 1, "BIDIRECTIONAL": False, "DROPOUT": 0.0},
                            synth.make_table(4, V, E)).cuda().train()


def test_poisoned_buffers_change_no_bit_of_the_loss_or_of_the_gathered_step():
    """One call of contrastive_softmax_loss (with its backward) and one train_step(negatives="in_batch", gather_negatives=True)
    with every torch.empty / empty_like filled with NaN words: workspace, gradient outputs, the pool and its gradient.  The
    same bits as on zero-filled buffers."""
    import twotowermlretrieval_amd as tt
    B, M, pos, H = 65, 300, 130, 96
    q, d = rows(650, B, H), rows(651, M, H)
    ids = [torch.from_numpy(synth.make_ids(90 + s, BT, T, V)).cuda() for s, T in enumerate((6, 11, 9))]
    base = small_model()
    out = {}
    for word in (0xFFFFFFFF, CONTROL):
        t = [dev(a).requires_grad_(True) for a in (q, d)]
        m = copy.deepcopy(base)
        opt = tt.FusedClipAdam(m.parameters(), lr=1e-2, max_norm=1.0)
        with poisoned_empty(word) as p:
            loss = tt.contrastive_softmax_loss(t[0], t[1], pos_offset=pos, temperature=0.05)
            loss.backward()
            step_loss = tt.train_step(m, opt, *ids, negatives="in_batch", temperature=TEMP, gather_negatives=True)
        torch.cuda.synchronize()
        assert p.tensors >= 6
        out[word] = [x.detach().cpu().numpy() for x in (loss, t[0].grad, t[1].grad, step_loss, opt.flat_params, opt.exp_avg_sq)]
    for x, y in zip(out[0xFFFFFFFF], out[CONTROL]):
        assert np.isfinite(x).all() and x.tobytes() == y.tobytes()
