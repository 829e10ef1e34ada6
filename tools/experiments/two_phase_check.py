#!/usr/bin/env python3
"""Is the document tower's forward in two halves (TT_ENC_PHASE_BEGIN / _FINISH around the query tower's call) the same bits as the
one-call form?  Gradients of one direct train step, three ways."""
import sys, copy
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parent.parent.parent))
sys.path.insert(0, str(Path(__file__).resolve().parent.parent.parent / "tests" / "golden"))
import numpy as np, torch
import synth
import twotowermlretrieval_amd as tt
from twotowermlretrieval_amd import trainer as T
V, E, H, B = 500, 300, 256, 512
torch.manual_seed(5)
m0 = tt.TwoTowerModel({"VOCAB_SIZE": V, "EMBED_DIM": E, "HIDDEN_DIM": H}, synth.make_table(4, V, E)).cuda().train()
ids = [torch.from_numpy(synth.make_ids(60 + s, B, Tn, V)).cuda() for s, Tn in enumerate((9, 60, 70))]
res = {}
for name, order, direct in (("two_phase", "query_first", True), ("query_first", "query_first_whole", True),
                            ("autograd", "query_first", False), ("two_phase_again", "query_first", True)):
    T._FWD_ORDER = order   # ("query_first": the document tower's call in two halves; "query_first_whole": whole calls)
    m = copy.deepcopy(m0)
    o = tt.FusedClipAdam(m.parameters(), lr=1e-5, max_norm=1.0)
    loss = tt.train_step(m, o, *ids, margin=0.5, direct=direct)
    torch.cuda.synchronize()
    res[name] = (float(loss), o.flat_grads.clone(), o.flat_params.clone(), [p.numel() for p in o.params])
base = res["two_phase"]
for name, r in res.items():
    dg = (r[1] - base[1]).abs()
    off, parts = 0, []
    for n in r[3]:
        parts.append(float(dg[off:off + n].max())); off += n
    print(name, "loss", r[0], "grads differ at", int((dg > 0).sum()), "max", float(dg.max()), "per tensor max", parts,
          "params differ at", int((r[2] != base[2]).sum()), flush=True)
# what did the optimizer do in each?
T._FWD_ORDER = "query_first"
for name, direct in (("direct", True), ("autograd", False)):
    m = copy.deepcopy(m0)
    o = tt.FusedClipAdam(m.parameters(), lr=1e-5, max_norm=1.0)
    before = o.flat_params.clone()
    loss = tt.train_step(m, o, *ids, margin=0.5, direct=direct)
    torch.cuda.synchronize()
    d = (o.flat_params - before)
    print(name, "gate", o.gate.tolist(), "step_count", o.step_count, "total_norm", float(o.total_norm), "update absmax", float(d.abs().max()),
          "nonzero updates", int((d != 0).sum()), "exp_avg absmax", float(o.exp_avg.abs().max()), flush=True)
