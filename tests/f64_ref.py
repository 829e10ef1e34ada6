"""float64 statements of the encoder, the triplet loss and clip + Adam with stock torch modules on the CPU (tests only).

The fp32 C oracle (oracle/tt_oracle.c) is this project's own code; nn.GRU / nn.LSTM / nn.RNN in double precision is an
independent, higher-precision statement of the same operations (backend/model.py:48-75, :109-114; backend/main.py:257-259).
Never imports the package: every input is numpy, every result numpy float64."""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F


def encoder_f64(cell, ids, table, sd, E, H, layers=1, bi=False, d_out=None, table_grad=False):
    """RNNEncoder.forward (+ backward with the output cotangent d_out) in float64, dropout = 0, normalised output.
    sd: synth.make_encoder_state's dict (keys rnn.<name>, projection.weight / .bias).
    Returns (out [B,H], grads {<torch's name>: array, "projection.weight" / "projection.bias" when bi}, table gradient
    [V,E] or None).  Row 0 of the table is a real row in the lookup (interior id-0 tokens are looked up) and gets no
    gradient (padding_idx = 0)."""
    rnn = getattr(torch.nn, cell.upper())(E, H, num_layers=layers, batch_first=True, bidirectional=bi).double()
    with torch.no_grad():
        for name, prm in rnn.named_parameters():
            src = torch.from_numpy(np.asarray(sd[f"rnn.{name}"])).double()
            assert src.shape == prm.shape, (name, src.shape, prm.shape)
            prm.copy_(src)
    proj = None
    if bi:
        proj = [torch.from_numpy(np.asarray(sd[f"projection.{n}"])).double().requires_grad_(True) for n in ("weight", "bias")]
    ids_t = torch.from_numpy(np.ascontiguousarray(ids, dtype=np.int64))
    table64 = torch.from_numpy(np.asarray(table)).double().requires_grad_(bool(table_grad))
    emb = table64[ids_t]
    lengths = (ids_t != 0).sum(1)
    packed = torch.nn.utils.rnn.pack_padded_sequence(emb, lengths, batch_first=True, enforce_sorted=False)
    _, h = rnn(packed)
    if cell.upper() == "LSTM":
        h = h[0]
    hidden = torch.cat([h[-2], h[-1]], dim=1) @ proj[0].T + proj[1] if bi else h[-1]
    out = F.normalize(hidden, p=2, dim=1)
    grads, gt = {}, None
    if d_out is not None:
        out.backward(torch.from_numpy(np.asarray(d_out)).double())
        grads = {name: prm.grad.numpy().copy() for name, prm in rnn.named_parameters()}
        if bi:
            grads["projection.weight"], grads["projection.bias"] = (x.grad.numpy().copy() for x in proj)
        if table_grad:
            gt = table64.grad.numpy().copy()
            gt[0] = 0.0
    return out.detach().numpy().copy(), grads, gt


def triplet_f64(q, p, n, margin):
    """clamp(cs(q,n) - cs(q,p) + margin, min=0).mean() in float64 with autograd: (loss, dq, dp, dn)."""
    t = [torch.from_numpy(np.asarray(a)).double().requires_grad_(True) for a in (q, p, n)]
    cs = F.cosine_similarity
    loss = torch.clamp(cs(t[0], t[2]) - cs(t[0], t[1]) + margin, min=0).mean()
    loss.backward()
    return (float(loss.item()),) + tuple(x.grad.numpy().copy() for x in t)


def clip_adam_f64(p0, grads_per_step, lr, max_norm):
    """clip_grad_norm_(max_norm) then torch.optim.Adam(lr).step(), per step, in float64.
    Returns [(parameters after the step, pre-clip total norm)] per step."""
    prm = torch.nn.Parameter(torch.from_numpy(np.asarray(p0)).double().clone())
    opt = torch.optim.Adam([prm], lr=lr)
    out = []
    for g in grads_per_step:
        prm.grad = torch.from_numpy(np.asarray(g)).double().clone()
        total = torch.nn.utils.clip_grad_norm_([prm], max_norm=max_norm)
        opt.step()
        out.append((prm.detach().numpy().copy(), float(total)))
    return out
