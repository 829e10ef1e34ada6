"""The softmax loss over a pool against SOFT TARGETS stated with stock torch ops on the CPU (tests only): the truth in float64,
and the same code in float32 as the yardstick for what float32 arithmetic can deliver at a shape.

    s_ij as tests/pool_loss_ref.py.  t [B, M] any finite weights:
        w_i  = sum_j t_ij          lse_i = logsumexp_{j<M} s_ij
        loss = mean_{i<B} (w_i lse_i - sum_j t_ij s_ij)
        d loss / d s_ij = G_ij = (w_i exp(s_ij - lse_i) - t_ij) / B

Written in that algebraic form (w lse - sum t s, not sum t (lse - s)): it is the form whose float32 run the bound is taken from.
Never imports the package: every input is numpy, every result numpy (loss a Python float)."""
from __future__ import annotations

import numpy as np
import torch

from in_batch_ref import normalised


def scores(q, docs, temperature, dtype=torch.float64):
    q, docs = (torch.from_numpy(np.asarray(a)).to(dtype) for a in (q, docs))
    return (normalised(q) @ normalised(docs).T) / temperature


def soft_loss(q, docs, targets, temperature, dtype=torch.float64):
    """(loss, dq, ddocs) by autograd in `dtype`."""
    t = [torch.from_numpy(np.asarray(a)).to(dtype).requires_grad_(True) for a in (q, docs)]
    tg = torch.from_numpy(np.asarray(targets)).to(dtype)
    B, M = t[0].shape[0], t[1].shape[0]
    assert 1 <= B <= M and tuple(tg.shape) == (B, M)
    s = (normalised(t[0]) @ normalised(t[1]).T) / temperature
    loss = (tg.sum(dim=1) * torch.logsumexp(s, dim=1) - (tg * s).sum(dim=1)).mean()
    loss.backward()
    return (float(loss.item()),) + tuple(x.grad.numpy().copy() for x in t)


def closed_form_G(q, docs, targets, temperature, dtype=torch.float64):
    """G [B, M] = d loss / d s by the formula."""
    s = scores(q, docs, temperature, dtype)
    tg = torch.from_numpy(np.asarray(targets)).to(dtype)
    lse = torch.logsumexp(s, dim=1, keepdim=True)
    return ((tg.sum(dim=1, keepdim=True) * torch.exp(s - lse) - tg) / s.shape[0]).numpy()


def bounds(q, docs, targets, temperature):
    """(want, tol): the float64 results and, per result (loss, dq, ddocs), the error allowed to a float32 implementation at
    this shape: 4 x the error of this very code run in float32, plus 4 * 2^-24 * max|want| (the rule of pool_loss_ref.bounds)."""
    want = soft_loss(q, docs, targets, temperature, torch.float64)
    f32 = soft_loss(q, docs, targets, temperature, torch.float32)
    tol = []
    for w, f in zip(want, f32):
        w, f = np.asarray(w, dtype=np.float64), np.asarray(f, dtype=np.float64)
        tol.append(4.0 * float(np.abs(f - w).max()) + 4.0 * 2.0 ** -24 * float(np.abs(w).max()))
    return want, tol
