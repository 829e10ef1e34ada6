"""The in-batch softmax contrastive loss stated with stock torch ops on the CPU (tests only): the truth in float64, and the
same code in float32 as the yardstick for what float32 arithmetic can deliver at a shape.

    qh_i = q_i / max(||q_i||, eps)        Dh_j = D_j / max(||D_j||, eps)        D = [p; n], eps = 1e-8
    s_ij = (qh_i . Dh_j) / temperature    loss = mean_i (logsumexp_j s_ij - s_ii)

Never imports the package: every input is numpy, every result numpy (loss a Python float)."""
from __future__ import annotations

import numpy as np
import torch

EPS = 1e-8


def normalised(x: torch.Tensor) -> torch.Tensor:
    """Rows divided by their clamped norm.  (vector_norm's gradient at an all-zero row is zero, and clamp_min passes no
    gradient below eps: a row shorter than eps is simply divided by eps.)"""
    return x / torch.linalg.vector_norm(x, dim=1, keepdim=True).clamp_min(EPS)


def cosines(q, d, dtype=torch.float64) -> np.ndarray:
    """[Bq, Bd] matrix qh . Dh^T."""
    q, d = (torch.from_numpy(np.asarray(a)).to(dtype) for a in (q, d))
    return (normalised(q) @ normalised(d).T).numpy()


def in_batch_loss(q, p, n, temperature, dtype=torch.float64):
    """(loss, dq, dp, dn) by autograd in `dtype`."""
    t = [torch.from_numpy(np.asarray(a)).to(dtype).requires_grad_(True) for a in (q, p, n)]
    qh, dh = normalised(t[0]), normalised(torch.cat([t[1], t[2]], dim=0))
    s = (qh @ dh.T) / temperature
    loss = (torch.logsumexp(s, dim=1) - torch.diagonal(s)).mean()   # (diagonal of [B,2B]: s_ii, the positive p_i)
    loss.backward()
    return (float(loss.item()),) + tuple(x.grad.numpy().copy() for x in t)


def bounds(q, p, n, temperature):
    """(want, tol): the float64 results and, per result, the error allowed to a float32 implementation at this shape:
    4 x the error of this very code run in float32, plus 4 * 2^-24 * max|want| (for shapes where torch's float32 happens to
    be exact)."""
    want = in_batch_loss(q, p, n, temperature, torch.float64)
    f32 = in_batch_loss(q, p, n, temperature, torch.float32)
    tol = []
    for w, f in zip(want, f32):
        w, f = np.asarray(w, dtype=np.float64), np.asarray(f, dtype=np.float64)
        tol.append(4.0 * float(np.abs(f - w).max()) + 4.0 * 2.0 ** -24 * float(np.abs(w).max()))
    return want, tol
