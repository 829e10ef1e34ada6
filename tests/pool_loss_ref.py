"""The softmax contrastive loss over a pool of documents stated with stock torch ops on the CPU (tests only): the truth in
float64, and the same code in float32 as the yardstick for what float32 arithmetic can deliver at a shape.

    qh_i = q_i / max(||q_i||, eps)        Dh_j = docs_j / max(||docs_j||, eps)        eps = 1e-8
    s_ij = (qh_i . Dh_j) / temperature    loss = mean_{i<B} (logsumexp_{j<M} s_ij - s_{i, pos_offset+i})

The rectangular form of tests/in_batch_ref.py (whose loss is the case docs = [p; n], pos_offset = 0).
Never imports the package: every input is numpy, every result numpy (loss a Python float)."""
from __future__ import annotations

import numpy as np
import torch

from in_batch_ref import normalised


def pool_loss(q, docs, pos_offset, temperature, dtype=torch.float64):
    """(loss, dq, ddocs) by autograd in `dtype`."""
    t = [torch.from_numpy(np.asarray(a)).to(dtype).requires_grad_(True) for a in (q, docs)]
    B, M = t[0].shape[0], t[1].shape[0]
    assert 1 <= B <= M and 0 <= pos_offset <= M - B
    s = (normalised(t[0]) @ normalised(t[1]).T) / temperature
    loss = (torch.logsumexp(s, dim=1) - torch.diagonal(s, offset=pos_offset)).mean()   # (s_{i, pos_offset+i}, i < B)
    loss.backward()
    return (float(loss.item()),) + tuple(x.grad.numpy().copy() for x in t)


def bounds(q, docs, pos_offset, temperature):
    """(want, tol): the float64 results and, per result (loss, dq, ddocs), the error allowed to a float32 implementation at
    this shape: 4 x the error of this very code run in float32, plus 4 * 2^-24 * max|want| (the rule of in_batch_ref.bounds)."""
    want = pool_loss(q, docs, pos_offset, temperature, torch.float64)
    f32 = pool_loss(q, docs, pos_offset, temperature, torch.float32)
    tol = []
    for w, f in zip(want, f32):
        w, f = np.asarray(w, dtype=np.float64), np.asarray(f, dtype=np.float64)
        tol.append(4.0 * float(np.abs(f - w).max()) + 4.0 * 2.0 ** -24 * float(np.abs(w).max()))
    return want, tol
