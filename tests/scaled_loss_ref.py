"""The four softmax contrastive losses with a LEARNABLE, CLAMPED logit scale, stated with stock torch ops on the CPU (tests
only): the truth in float64, and the same code in float32 as the yardstick for what float32 arithmetic can deliver at a shape.

    l a leaf [1];   T = exp(-clamp(l, lo, hi));   s_ij = (qh_i . Dh_j) / T
    kind "plain"    tests/pool_loss_ref.py        kind "grouped"   tests/grouped_loss_ref.py (labels)
    kind "soft"     tests/soft_loss_ref.py (targets)       kind "sym"   tests/sym_loss_ref.py (alpha, labels optional)

Those files take the temperature as it comes, so they are used as they are with the 0-d tensor T; their backward() also fills
l.grad = d loss / d l.  The second route to that scalar is the one the kernels take: with c = qh Dh^T a leaf and s = c / T,
G = d loss / d c, and
    d loss / d l = sum_ij G_ij c_ij = sum_i qh_i . dqh_i,   dqh = G Dh          (inside the clamp; 0 outside)
for which the losses are restated once as functions of the score matrix (loss_of_scores).
Never imports the package: every input is numpy, every result numpy (the scalars Python floats)."""
from __future__ import annotations

import numpy as np
import torch

import grouped_loss_ref
import pool_loss_ref
import soft_loss_ref
import sym_loss_ref
from in_batch_ref import normalised

KINDS = ("plain", "grouped", "soft", "sym")


def temperature_of(l, lo, hi, dtype=torch.float64):
    """(the leaf l [1], T 0-d) in `dtype`."""
    leaf = torch.tensor([float(l)], dtype=dtype, requires_grad=True)
    return leaf, torch.exp(-torch.clamp(leaf, float(lo), float(hi)))[0]


def scaled_loss(kind, q, docs, pos_offset, l, lo, hi, q_groups=None, doc_groups=None, targets=None, alpha=0.5,
                dtype=torch.float64):
    """(loss, dq, ddocs, d_log_scale), or (loss, L_qd, L_dq, dq, ddocs, d_log_scale) for "sym", by autograd in `dtype`."""
    leaf, T = temperature_of(l, lo, hi, dtype)
    if kind == "plain":
        out = pool_loss_ref.pool_loss(q, docs, pos_offset, T, dtype)
    elif kind == "grouped":
        out = grouped_loss_ref.grouped_loss(q, docs, pos_offset, T, q_groups, doc_groups, dtype)
    elif kind == "soft":
        out = soft_loss_ref.soft_loss(q, docs, targets, T, dtype)
    else:
        assert kind == "sym"
        out = sym_loss_ref.sym_loss(q, docs, pos_offset, T, alpha, q_groups, doc_groups, dtype)
    return out + (float(leaf.grad[0]),)


def loss_of_scores(kind, s, pos_offset, q_groups=None, doc_groups=None, targets=None, alpha=0.5):
    """The loss as a function of the score matrix s [B, M] (a torch tensor), the statements of the four files above."""
    B = s.shape[0]
    if kind == "soft":
        tg = torch.from_numpy(np.asarray(targets)).to(s.dtype)
        return (tg.sum(dim=1) * torch.logsumexp(s, dim=1) - (tg * s).sum(dim=1)).mean()
    kept = s
    if q_groups is not None:
        kept = s.masked_fill(torch.from_numpy(grouped_loss_ref.ignored(q_groups, doc_groups, pos_offset)), float("-inf"))
    pos = torch.diagonal(s, offset=pos_offset)
    l_qd = (torch.logsumexp(kept, dim=1) - pos).mean()
    if kind != "sym":
        return l_qd
    l_dq = (torch.logsumexp(kept[:, pos_offset:pos_offset + B], dim=0) - pos).mean()
    return (1.0 - alpha) * l_qd + alpha * l_dq


def dot_route(kind, q, docs, pos_offset, l, lo, hi, q_groups=None, doc_groups=None, targets=None, alpha=0.5,
              dtype=torch.float64):
    """(sum_i qh_i . dqh_i, A = sum_ij |G_ij c_ij|) in `dtype`, before the clamp's mask: G = d loss / d c with c = qh Dh^T."""
    qh, dh = (normalised(torch.from_numpy(np.asarray(a)).to(dtype)) for a in (q, docs))
    with torch.no_grad():
        T = float(temperature_of(l, lo, hi, dtype)[1])
    c = (qh @ dh.T).requires_grad_(True)
    loss_of_scores(kind, c / T, pos_offset, q_groups, doc_groups, targets, alpha).backward()
    G = c.grad
    dqh = G @ dh
    return float((qh * dqh).sum(dim=1).sum()), float((G * c.detach()).abs().sum())


def clamp_passes(l, lo, hi) -> bool:
    """torch.clamp's derivative: 1 where lo <= l <= hi."""
    return bool(float(lo) <= float(l) <= float(hi))


def bounds(kind, q, docs, pos_offset, l, lo, hi, q_groups=None, doc_groups=None, targets=None, alpha=0.5):
    """(want, tol): the float64 results in scaled_loss's order and, per result, the error allowed to a float32 implementation.
    loss, L_qd, L_dq, dq, ddocs: 4 x the error of this very code run in float32, plus 4 * 2^-24 * max|want| (the rule of
    pool_loss_ref.bounds).  The scalar d_log_scale has no maximum over elements to steady a one-sample yardstick, so:
        4 x max(error of the float32 autograd route, error of the float32 sum_i qh_i . dqh_i route) + 32 * 2^-24 * A,
    A = sum_ij |G_ij c_ij| in float64: the magnitude the sum is made of (|want| when nothing cancels); 32 covers the longest
    addition chain of the kernels' fixed order (8 lane steps, 6 xor steps, 8 slices, the row sum)."""
    kw = dict(q_groups=q_groups, doc_groups=doc_groups, targets=targets, alpha=alpha)
    want = scaled_loss(kind, q, docs, pos_offset, l, lo, hi, dtype=torch.float64, **kw)
    f32 = scaled_loss(kind, q, docs, pos_offset, l, lo, hi, dtype=torch.float32, **kw)
    tol = []
    for w, f in zip(want[:-1], f32[:-1]):
        w, f = np.asarray(w, dtype=np.float64), np.asarray(f, dtype=np.float64)
        tol.append(4.0 * float(np.abs(f - w).max()) + 4.0 * 2.0 ** -24 * float(np.abs(w).max()))
    _, A = dot_route(kind, q, docs, pos_offset, l, lo, hi, dtype=torch.float64, **kw)
    dots32 = dot_route(kind, q, docs, pos_offset, l, lo, hi, dtype=torch.float32, **kw)[0] if clamp_passes(l, lo, hi) else 0.0
    tol.append(4.0 * max(abs(f32[-1] - want[-1]), abs(dots32 - want[-1])) + 32.0 * 2.0 ** -24 * A)
    return want, tol
