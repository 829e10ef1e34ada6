"""K9 in-batch softmax loss (tt_in_batch_loss_f32, in_batch_softmax_loss) against its float64 statement (tests/in_batch_ref.py).

The kernels work in tiles: a workgroup owns 32 queries (query-tile height) or 32 documents (document-tile width), and walks the
other side in chunks of 128 rows, one 32-row MFMA tile per wave; images are zero-padded to H rounded up to 32 columns.  Shapes:
B = 1 (two candidates) and 3; B = 31, 32, 33 around the query-tile height; B = 17 (2B = 34, one document past a document
tile) and B = 65 (2B = 130, one pair past a 128-row chunk of documents, one query past two query tiles); B = 1025 (several
tiles and chunks both ways, ragged); H = 20 (< 32, not a multiple of 4), 32, 96, 256, 512 (four 32-column slices per wave).
The walked side is cut into slices of whole chunks, one workgroup each, whose partial results are added in ascending order:
one slice up to B = 64, two (of the documents) at B = 65, six uneven ones of the documents and three of the queries at B = 1025.

The slice classes (ib_slices: up to IB_MAX_SLICES = 8 partial results per side, combined in fixed order by ib_lse_kernel and
ib_project_kernel).  Q = slices x chunks each of the documents a query tile walks, D = the same of the queries a document tile
walks:
     B     H    Q                      D
   129    20    3 x 1                  2 x 1     the first multi-slice document side
   257    96    5 x 1                  3 x 1
   449    32    8 x 1                  4 x 1     the smallest B with all 8 slices, ragged last chunk
   512   256    8 x 1                  4 x 1     the product's train batch
   513    32    5 x 2 (last: 1 chunk)  5 x 1     uneven last slice
   641    20    6 x 2 (last: 1 chunk)  6 x 1     the most document-side slices any B gives
  1024    32    8 x 2                  4 x 2     all 8 slices, two chunks each
  4096    32    2 x 32                 1 x 32    32 chunks folded by one workgroup through the online softmax

Bound per result (loss, dq, dp, dn): 4 x the error of the helper itself evaluated in float32 at that very shape, plus
4 * 2^-24 * max|want| -- room for another summation order over 2B * H terms, none for a half-precision product."""
import numpy as np
import pytest
import torch

import synth
from in_batch_ref import bounds

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def call_abi(q, p, n, temperature, grads=True, fill=None):
    """The C entry on device copies of q, p, n.  fill: byte the workspace holds on entry (None: whatever the allocator gave).
    Returns (loss [1], dq, dp, dn) as numpy (the gradients None without `grads`)."""
    from twotowermlretrieval_amd import _lib
    L = _lib.lib()
    B, H = q.shape
    tq, tp, tn = dev(q), dev(p), dev(n)
    loss = torch.full((1,), float("nan"), device="cuda")
    g = [torch.full_like(t, float("nan")) for t in (tq, tp, tn)] if grads else [None] * 3
    need = L.tt_in_batch_loss_workspace_bytes(B, H)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    if fill is not None:
        ws.fill_(fill)
    ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
    _lib.check(L.tt_in_batch_loss_f32(tq.data_ptr(), tp.data_ptr(), tn.data_ptr(), B, H, float(temperature), loss.data_ptr(),
                                      ptr(g[0]), ptr(g[1]), ptr(g[2]), ws.data_ptr(), need, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return (loss.cpu().numpy(),) + tuple(t.cpu().numpy() if t is not None else None for t in g)


def check(q, p, n, temperature):
    want, tol = bounds(q, p, n, temperature)
    got = call_abi(q, p, n, temperature)
    got = (float(got[0][0]),) + got[1:]
    errs = [float(np.abs(np.asarray(g, dtype=np.float64) - np.asarray(w, dtype=np.float64)).max()) for g, w in zip(got, want)]
    print("  ".join(f"{name} err {e:.3e} / allowed {t:.3e} (max|want| {np.abs(w).max():.3e})"
                    for name, e, t, w in zip(("loss", "dq", "dp", "dn"), errs, tol, want)))
    for name, g, e, t in zip(("loss", "dq", "dp", "dn"), got, errs, tol):
        assert np.isfinite(g).all(), name
        assert e <= t, f"{name}: error {e:.3e} > {t:.3e}"
    return got, want


# every B once, every H at least once; scale: rows of non-unit norm (the cosine divides it out, the gradients do not)
@pytest.mark.parametrize("B,H,temperature,scale", [(1, 20, 1.0, 1.0), (3, 32, 0.05, 1.0), (17, 96, 1.0, 30.0), (31, 256, 0.05, 1.0),
                                                   (32, 512, 1.0, 1.0e-3), (33, 20, 0.05, 30.0), (65, 96, 0.05, 1.0e-3),
                                                   (1025, 256, 0.05, 1.0),
                                                   # the slice classes of the module docstring
                                                   (129, 20, 0.05, 1.0), (257, 96, 0.05, 30.0), (449, 32, 0.05, 1.0e-3),
                                                   (512, 256, 0.05, 1.0), (513, 32, 0.05, 30.0), (641, 20, 0.05, 1.0e-3),
                                                   (1024, 32, 0.05, 1.0), (4096, 32, 0.05, 30.0)])
def test_loss_and_gradients_vs_float64(B, H, temperature, scale):
    q, p, n = ((synth.unit_rows(11 * B + s, B, H) * np.float32(scale)).astype(np.float32) for s in range(3))
    check(q, p, n, temperature)


def test_logits_of_100_do_not_overflow():
    """temperature = 0.01 and p_i = q_i on every third row: cos = 1, the logit is 100 and exp(100) is not a float32.  Only a
    running maximum inside the softmax keeps the sums finite."""
    B, H = 33, 96
    q, p, n = (synth.unit_rows(70 + s, B, H).copy() for s in range(3))
    p[::3] = q[::3]
    got, _ = check(q, p, n, 0.01)
    assert np.isfinite(got[0])


@pytest.mark.parametrize("B", [449, 4096])
def test_logits_of_100_across_slices_and_chunks(B):
    """The same construction at B = 449 (8 slices of one chunk: the maximum of 100 sits in another slice than most of a row's
    logits, and ib_lse_kernel rescales across slices) and B = 4096 (one workgroup folds 32 chunks: the running maximum jumps
    to 100 in whichever chunk holds p_i)."""
    H = 32
    q, p, n = (synth.unit_rows(170 + B + s, B, H).copy() for s in range(3))
    p[::3] = q[::3]
    got, _ = check(q, p, n, 0.01)
    assert np.isfinite(got[0])


def test_rows_shorter_than_eps_are_divided_by_eps():
    """One all-zero query and one all-zero passage: their images are zero, every logit with them is 0, and the gradient with
    respect to them is the image's gradient over eps (the helper defines it)."""
    B, H = 5, 32
    q, p, n = (synth.unit_rows(80 + s, B, H).copy() for s in range(3))
    q[1] = 0.0
    p[3] = 0.0
    got, want = check(q, p, n, 0.05)
    assert np.abs(want[1][1]).max() > 1e6 and np.abs(want[2][3]).max() > 1e6     # (the case is what it claims to be)


def test_loss_alone_is_the_loss_of_the_full_call():
    B, H = 33, 96
    q, p, n = (synth.unit_rows(90 + s, B, H) for s in range(3))
    full = call_abi(q, p, n, 0.05)
    alone = call_abi(q, p, n, 0.05, grads=False)
    assert alone[1] is None and np.isfinite(alone[0]).all()
    assert alone[0].tobytes() == full[0].tobytes()


def test_same_bits_twice_whatever_the_workspace_held():
    B, H = 65, 96
    q, p, n = (synth.unit_rows(95 + s, B, H) * np.float32(2.0) for s in range(3))
    a = call_abi(q, p, n, 0.05, fill=0xFF)
    b = call_abi(q, p, n, 0.05, fill=0x00)
    for x, y in zip(a, b):
        assert np.isfinite(x).all() and x.tobytes() == y.tobytes()


def test_autograd_scales_the_kernel_gradients_by_the_incoming_scalar():
    import twotowermlretrieval_amd as tt
    B, H = 33, 32
    q, p, n = (synth.unit_rows(99 + s, B, H) for s in range(3))
    direct = call_abi(q, p, n, 0.05)
    t = [dev(a).requires_grad_(True) for a in (q, p, n)]
    loss = tt.in_batch_softmax_loss(tuple(t), temperature=0.05)
    assert loss.dim() == 0
    (3 * loss).backward()
    torch.cuda.synchronize()
    assert np.float32(loss.item()).tobytes() == direct[0].tobytes()
    for x, d in zip(t, direct[1:]):
        assert np.array_equal(x.grad.cpu().numpy(), np.float32(3.0) * d)


def test_python_entry_validates_like_the_triplet_loss():
    import twotowermlretrieval_amd as tt
    a = torch.zeros((4, 32), device="cuda")
    with pytest.raises(ValueError):
        tt.in_batch_softmax_loss((a, a, a[:3]))
    with pytest.raises(ValueError):
        tt.in_batch_softmax_loss((a, a.double(), a))
    with pytest.raises(ValueError):
        tt.in_batch_softmax_loss((a, a, a), temperature=0.0)
    with pytest.raises(RuntimeError):
        tt.in_batch_softmax_loss((a.cpu(), a, a))
