"""K6 triplet loss (triplet_loss_cosine) and K8 clip + Adam (FusedClipAdam) against the same torch calls in float64
(tests/f64_ref.py: F.cosine_similarity + clamp + mean with autograd; clip_grad_norm_ + torch.optim.Adam), at the batch and
buffer sizes where the launches change shape: K6 runs four rows per 256-thread block and sums the rows in one 1024-thread
block (B = 1, 3, 4, 5; 1023, 1025; 4099), 64 lanes stride a row (H = 32 < 64, 96, 256, 512); K8 runs at most 512 blocks of 256
(n = 131072 is the last size with one element per thread).  Bounds are those tests/test_train_gpu.py holds these kernels to."""
import numpy as np
import pytest
import torch

import synth
from f64_ref import clip_adam_f64, triplet_f64

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def triplet_on_gpu(q, p, n, margin):
    from twotowermlretrieval_amd.model import triplet_loss_cosine
    t = [dev(a).requires_grad_(True) for a in (q, p, n)]
    loss = triplet_loss_cosine(tuple(t), margin=margin)
    loss.backward()
    torch.cuda.synchronize()
    assert loss.dim() == 0
    return (float(loss.item()),) + tuple(x.grad.cpu().numpy() for x in t)


def hinge_args(q, p, n, margin):
    """cos(q,n) - cos(q,p) + margin per row, in float64 (what decides which rows carry a gradient)."""
    q, p, n = (np.asarray(a, dtype=np.float64) for a in (q, p, n))
    cos = lambda a, b: (a * b).sum(1) / (np.maximum(np.linalg.norm(a, axis=1), 1e-8) * np.maximum(np.linalg.norm(b, axis=1), 1e-8))
    return cos(q, n) - cos(q, p) + margin


def check_triplet(q, p, n, margin):
    got = triplet_on_gpu(q, p, n, margin)
    want = triplet_f64(q, p, n, margin)
    print(f"loss err {abs(got[0] - want[0]):.3e}", [f"{np.abs(g - w).max():.3e}/{np.abs(w).max():.3e}" for g, w in zip(got[1:], want[1:])])
    assert abs(got[0] - want[0]) < 1e-6
    for g, w in zip(got[1:], want[1:]):
        np.testing.assert_allclose(g, w, atol=2e-7, rtol=1e-4)
    return got, want


# every B once, every H once; scale: rows of non-unit norm (the cosine divides them out, the gradients do not)
@pytest.mark.parametrize("B,H,margin,scale", [(1, 32, 0.5, 1.0), (3, 96, 0.2, 1.0), (4, 256, 0.5, 1.0), (5, 512, 0.2, 1.0),
                                              (1023, 96, 0.5, 1.0e-3), (1025, 256, 0.2, 30.0), (4099, 32, 0.5, 1.0)])
def test_triplet_loss_and_embedding_gradients_vs_float64(B, H, margin, scale):
    q, p, n = ((synth.unit_rows(7 * B + s, B, H) * np.float32(scale)).astype(np.float32) for s in range(3))
    v = hinge_args(q, p, n, margin)
    assert np.abs(v).min() > 1e-5            # (no row sits on the hinge: fp32 and float64 see the same active set)
    check_triplet(q, p, n, margin)


def test_triplet_rows_under_the_hinge_get_exactly_zero_gradients():
    """p = q on every third row: cos(q,p) = 1, so cos(q,n) - 1 + margin < 0 there; the other rows are active."""
    B, H, margin = 1023, 512, 0.2
    q, p, n = (synth.unit_rows(50 + s, B, H) for s in range(3))
    off = np.arange(B) % 3 == 0
    p[off] = q[off]
    v = hinge_args(q, p, n, margin)
    assert (v[off] < -1e-3).all() and (v[~off] > 1e-3).all()
    got, want = check_triplet(q, p, n, margin)
    for g, w in zip(got[1:], want[1:]):
        assert not g[off].any() and not w[off].any()
        assert np.abs(g[~off]).max(axis=1).min() > 0


def test_triplet_hinge_argument_exactly_zero_passes_the_gradient():
    """margin = 0 and p = n row by row: cos(q,n) - cos(q,p) is exactly 0 in any precision, and clamp(min=0) passes the
    gradient where its argument is >= 0 (ATen's mask): dq cancels to zero, dp = -dn are not zero."""
    B, H = 5, 96
    q, p = synth.unit_rows(60, B, H), synth.unit_rows(61, B, H)
    n = p.copy()
    got, want = check_triplet(q, p, n, 0.0)
    assert got[0] == 0.0 and want[0] == 0.0
    for res in (got, want):
        assert np.abs(res[2]).max(axis=1).min() > 1e-4 and np.abs(res[3]).max(axis=1).min() > 1e-4


@pytest.mark.parametrize("n", [1, 255, 256, 257, 131072, 131073, 300001])
def test_fused_clip_adam_three_steps_vs_float64(n):
    """Step 1 clips (pre-clip norm 10 against max_norm 1), step 2 does not (0.01), step 3 clips again."""
    from twotowermlretrieval_amd.trainer import FusedClipAdam
    rs = np.random.RandomState(n % 1000 + 3)
    p0 = rs.standard_normal(n).astype(np.float32)
    grads = []
    for target in (10.0, 0.01, 10.0):
        z = rs.standard_normal(n)
        grads.append((z / np.linalg.norm(z) * target).astype(np.float32))
    want = clip_adam_f64(p0, grads, lr=1e-3, max_norm=1.0)
    prm = torch.nn.Parameter(dev(p0))
    opt = FusedClipAdam([prm], lr=1e-3, max_norm=1.0)
    for step, g in enumerate(grads):
        opt.zero_grad()
        prm.grad.copy_(dev(g))
        tn = float(opt.step().item())
        wp, wn = want[step]
        assert (wn > 1.0) == (step != 1)
        got = prm.detach().cpu().numpy()
        print(f"step {step}: norm rel err {abs(tn - wn) / wn:.3e}, max param err {np.abs(got - wp).max():.3e}")
        assert abs(tn - wn) / wn < 1e-6
        np.testing.assert_allclose(got, wp, atol=1e-8, rtol=2e-6)
