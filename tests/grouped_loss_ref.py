"""The softmax contrastive loss over a pool with GROUPED NEGATIVES stated with stock torch ops on the CPU (tests only): the truth
in float64, and the same code in float32 as the yardstick for what float32 arithmetic can deliver at a shape.

    s_ij as tests/pool_loss_ref.py.  int64 labels qg [B], dg [M]; the pair (i, j) is IGNORED iff
        j != pos_offset + i   and   qg[i] >= 0   and   dg[j] == qg[i]
    loss = mean_{i<B} (logsumexp_{j kept for i} s_ij - s_{i, pos_offset+i})

The ignored logits are set to -inf before logsumexp: they add exp(-inf) = 0 to the sum and receive no gradient.
Never imports the package: every input is numpy, every result numpy (loss a Python float)."""
from __future__ import annotations

import numpy as np
import torch

from in_batch_ref import normalised


def ignored(q_groups, doc_groups, pos_offset) -> np.ndarray:
    """The [B, M] boolean matrix of ignored pairs."""
    qg, dg = np.asarray(q_groups, dtype=np.int64), np.asarray(doc_groups, dtype=np.int64)
    m = (qg[:, None] >= 0) & (dg[None, :] == qg[:, None])
    i = np.arange(qg.shape[0])
    m[i, pos_offset + i] = False                                   # (a query's own positive is always kept)
    return m


def grouped_loss(q, docs, pos_offset, temperature, q_groups, doc_groups, dtype=torch.float64):
    """(loss, dq, ddocs) by autograd in `dtype`."""
    t = [torch.from_numpy(np.asarray(a)).to(dtype).requires_grad_(True) for a in (q, docs)]
    B, M = t[0].shape[0], t[1].shape[0]
    assert 1 <= B <= M and 0 <= pos_offset <= M - B
    assert np.asarray(q_groups).shape == (B,) and np.asarray(doc_groups).shape == (M,)
    s = (normalised(t[0]) @ normalised(t[1]).T) / temperature
    kept = s.masked_fill(torch.from_numpy(ignored(q_groups, doc_groups, pos_offset)), float("-inf"))
    loss = (torch.logsumexp(kept, dim=1) - torch.diagonal(s, offset=pos_offset)).mean()
    loss.backward()
    return (float(loss.item()),) + tuple(x.grad.numpy().copy() for x in t)


def bounds(q, docs, pos_offset, temperature, q_groups, doc_groups):
    """(want, tol): the float64 results and, per result (loss, dq, ddocs), the error allowed to a float32 implementation at
    this shape: 4 x the error of this very code run in float32, plus 4 * 2^-24 * max|want| (the rule of pool_loss_ref.bounds)."""
    want = grouped_loss(q, docs, pos_offset, temperature, q_groups, doc_groups, torch.float64)
    f32 = grouped_loss(q, docs, pos_offset, temperature, q_groups, doc_groups, torch.float32)
    tol = []
    for w, f in zip(want, f32):
        w, f = np.asarray(w, dtype=np.float64), np.asarray(f, dtype=np.float64)
        tol.append(4.0 * float(np.abs(f - w).max()) + 4.0 * 2.0 ** -24 * float(np.abs(w).max()))
    return want, tol
