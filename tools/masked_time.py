#!/usr/bin/env python3
"""Masked exact search vs the unmasked call of the SAME build, event timing with interleaved rounds on one GPU: over
10M x 256 rows (fp32 and bf16), B = 32 and B = 1024, k = 10, the unmasked call against the masked call with an all-ones mask,
a random 50 % mask and a 1 %-kept mask.  The mask adds 1/(8 d bytes-per-element) of traffic (0.05 % fp32, 0.1 % bf16 at
d = 256), so an all-ones slowdown beyond the spread of the unmasked call's own repeats means a wait was added to the tile loop.
With --parent PATH (a libtt.so built from the parent commit) it also times that library's tt_score_topk_f32 against this
build's, to record that the unmasked instantiations did not move.
One JSON line per measurement (times in ms: median, and min..max over the rounds).
Usage: masked_time.py [docs] [--parent PATH]"""
import ctypes as C
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch

import bench
import twotowermlretrieval_amd as tt
from twotowermlretrieval_amd import _lib

args = sys.argv[1:]
parent = None
if "--parent" in args:
    at = args.index("--parent")
    parent = args[at + 1]
    del args[at:at + 2]
n = int(args[0]) if args else bench.N_DOCS
dev = torch.device("cuda:0")
K, ROUNDS = 10, 5


def timeit(fn, iters):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def interleaved(fns, iters, rounds=ROUNDS):
    """rounds x (every fn in turn): per fn (median, min, max) in ms."""
    ts = {name: [] for name in fns}
    for _ in range(rounds):
        for name, fn in fns.items():
            ts[name].append(timeit(fn, iters))
    return {name: (sorted(t)[len(t) // 2], min(t), max(t)) for name, t in ts.items()}


def emit(**kw):
    print(json.dumps(kw), flush=True)


g = torch.Generator(device=dev).manual_seed(0)
masks = {"ones": torch.ones(n, dtype=torch.bool, device=dev),
         "half": torch.rand(n, device=dev, generator=g) < 0.5,
         "one_percent": torch.rand(n, device=dev, generator=g) < 0.01}
keeps = {name: tt.pack_keep_mask(m) for name, m in masks.items()}
docs32 = bench.gen_rows(0, n, dev)
for dtype in (torch.float32, torch.bfloat16):
    docs = docs32 if dtype == torch.float32 else docs32.to(torch.bfloat16)
    for B in (32, 1024):
        q = bench.gen_queries(B, dev, seed=B)
        ws = torch.empty(_lib.lib().tt_score_topk_masked_workspace_bytes(B, n, 256, K, int(dtype == torch.bfloat16)),
                         dtype=torch.uint8, device=dev)
        plain = tt.score_topk(q, docs, K, 0, ws)
        ones = tt.score_topk(q, docs, K, 0, ws, keep=keeps["ones"])
        same = bool(torch.equal(plain[0], ones[0]) and torch.equal(plain[1], ones[1]))
        fns = {"unmasked": lambda: tt.score_topk(q, docs, K, 0, ws)}
        for name, keep in keeps.items():
            fns[name] = (lambda keep: lambda: tt.score_topk(q, docs, K, 0, ws, keep=keep))(keep)
        t = interleaved(fns, iters=3 if B > 64 else 20)
        base = t["unmasked"][0]
        emit(leg="masked", dtype=str(dtype).split(".")[1], B=B, docs=n, all_ones_identical=same,
             **{f"{name}_ms": [round(x, 4) for x in v] for name, v in t.items()},
             unmasked_spread=round((t["unmasked"][2] - t["unmasked"][1]) / base, 4),
             **{f"{name}_over_unmasked": round(t[name][0] / base, 4) for name in keeps})
    del docs

if parent:
    old = C.CDLL(parent)
    sig = _lib.SIGNATURES["tt_score_topk_f32"]
    old.tt_score_topk_f32.restype, old.tt_score_topk_f32.argtypes = sig
    new = _lib.lib()
    st = torch.cuda.current_stream().cuda_stream
    for B in (32, 1024):
        q = bench.gen_queries(B, dev, seed=B)
        ws = torch.empty(new.tt_score_topk_workspace_bytes(B, n, 256, K), dtype=torch.uint8, device=dev)
        outs = {}

        def call(lib, tag):
            v, i = outs.setdefault(tag, (torch.empty((B, K), device=dev), torch.empty((B, K), dtype=torch.int64, device=dev)))
            _lib.check(lib.tt_score_topk_f32(q.data_ptr(), B, 256, docs32.data_ptr(), n, K, 0, v.data_ptr(), i.data_ptr(),
                                             ws.data_ptr(), ws.numel(), st))

        t = interleaved({"parent": lambda: call(old, "parent"), "this": lambda: call(new, "this")}, iters=3 if B > 64 else 20)
        torch.cuda.synchronize()
        same = bool(torch.equal(outs["parent"][0], outs["this"][0]) and torch.equal(outs["parent"][1], outs["this"][1]))
        emit(leg="unmasked_vs_parent", B=B, docs=n, identical=same, parent_ms=[round(x, 4) for x in t["parent"]],
             this_ms=[round(x, 4) for x in t["this"]], this_over_parent=round(t["this"][0] / t["parent"][0], 4))
