"""The SYMMETRIC softmax contrastive loss over a pool stated with stock torch ops on the CPU (tests only): the truth in float64,
and the same code in float32 as the yardstick for what float32 arithmetic can deliver at a shape.

    s_ij as tests/pool_loss_ref.py;  P_i = pos_offset + i
    L_qd = mean_{i<B} (logsumexp_{j<M}  s_ij       - s_{i,P_i})
    L_dq = mean_{i<B} (logsumexp_{i'<B} s_{i',P_i} - s_{i,P_i})          (column P_i, over the B queries)
    loss = (1 - alpha) L_qd + alpha L_dq

Labels (both or neither): the ignored pairs of tests/grouped_loss_ref.py are -inf logits in BOTH softmaxes.
Never imports the package: every input is numpy, every result numpy (the losses Python floats)."""
from __future__ import annotations

import numpy as np
import torch

from grouped_loss_ref import ignored
from in_batch_ref import normalised


def sym_loss(q, docs, pos_offset, temperature, alpha, q_groups=None, doc_groups=None, dtype=torch.float64):
    """(loss, L_qd, L_dq, dq, ddocs) by autograd in `dtype`."""
    t = [torch.from_numpy(np.asarray(a)).to(dtype).requires_grad_(True) for a in (q, docs)]
    B, M = t[0].shape[0], t[1].shape[0]
    assert 1 <= B <= M and 0 <= pos_offset <= M - B and 0.0 <= alpha <= 1.0
    assert (q_groups is None) == (doc_groups is None)
    s = (normalised(t[0]) @ normalised(t[1]).T) / temperature
    kept = s
    if q_groups is not None:
        assert np.asarray(q_groups).shape == (B,) and np.asarray(doc_groups).shape == (M,)
        kept = s.masked_fill(torch.from_numpy(ignored(q_groups, doc_groups, pos_offset)), float("-inf"))
    pos = torch.diagonal(s, offset=pos_offset)                                # (s_{i, P_i}, i < B)
    l_qd = (torch.logsumexp(kept, dim=1) - pos).mean()
    l_dq = (torch.logsumexp(kept[:, pos_offset:pos_offset + B], dim=0) - pos).mean()
    loss = (1.0 - alpha) * l_qd + alpha * l_dq
    loss.backward()
    return (float(loss.item()), float(l_qd.item()), float(l_dq.item())) + tuple(x.grad.numpy().copy() for x in t)


def bounds(q, docs, pos_offset, temperature, alpha, q_groups=None, doc_groups=None):
    """(want, tol): the float64 results and, per result (loss, L_qd, L_dq, dq, ddocs), the error allowed to a float32
    implementation at this shape: 4 x the error of this very code run in float32, plus 4 * 2^-24 * max|want| (the rule of
    pool_loss_ref.bounds)."""
    want = sym_loss(q, docs, pos_offset, temperature, alpha, q_groups, doc_groups, torch.float64)
    f32 = sym_loss(q, docs, pos_offset, temperature, alpha, q_groups, doc_groups, torch.float32)
    tol = []
    for w, f in zip(want, f32):
        w, f = np.asarray(w, dtype=np.float64), np.asarray(f, dtype=np.float64)
        tol.append(4.0 * float(np.abs(f - w).max()) + 4.0 * 2.0 ** -24 * float(np.abs(w).max()))
    return want, tol
