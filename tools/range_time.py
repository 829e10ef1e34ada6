#!/usr/bin/env python3
"""Threshold search against the exact search of the SAME build, event timing with interleaved rounds on one GPU: over
10M x 256 rows (fp32 and bf16), B = 32 and B = 1024, the counting pass alone (tt_score_count_*: unmasked and under a random
50 % mask, thresholds = each query's 10th best score) against tt_score_topk_f32 / _bf16 for k = 10; then range_search(q, t, 10)
against search(q, 10) on a screen=True index.  The counting pass multiplies what the k = 10 search multiplies and selects
nothing, so the yardstick is that search and the margin its own round-to-round spread, printed next to the medians.
With --parent PATH (a libtt.so built from the parent commit) it also times that library's tt_score_topk_f32 against this
build's, to record that the existing instantiations did not move; with --ab PATH (the comparison build, -DTT_AB) the counting
pass with and without the pacing gate (TT_SCORE_PACE=0) at B = 1024.
One JSON line per measurement (times in ms: median, and min..max over the rounds).
Usage: range_time.py [docs] [--parent PATH] [--ab PATH]"""
import ctypes as C
import json
import os
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch

import bench
import twotowermlretrieval_amd as tt
from twotowermlretrieval_amd import _lib

args = sys.argv[1:]


def option(name):
    if name not in args:
        return None
    at = args.index(name)
    val = args[at + 1]
    del args[at:at + 2]
    return val


parent, ab = option("--parent"), option("--ab")
n = int(args[0]) if args else bench.N_DOCS
dev = torch.device("cuda:0")
K, ROUNDS, D_ = 10, 5, 256


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


def ms(v):
    return [round(x, 4) for x in v]


def bind(lib, name):
    fn = getattr(lib, name)
    fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    return fn


def count_call(lib, bf16, q, docs, keep, thr, out, ws):
    fn = bind(lib, "tt_score_count_bf16" if bf16 else "tt_score_count_f32")
    st = torch.cuda.current_stream().cuda_stream
    B = q.shape[0]
    return lambda: _lib.check(fn(q.data_ptr(), B, D_, docs.data_ptr(), docs.shape[0], None if keep is None else keep.data_ptr(),
                                 thr.data_ptr(), out.data_ptr(), 0, ws.data_ptr(), ws.numel(), st))


g = torch.Generator(device=dev).manual_seed(0)
keep_half = tt.pack_keep_mask(torch.rand(n, device=dev, generator=g) < 0.5)
docs32 = bench.gen_rows(0, n, dev)
L = _lib.lib()
for dtype in (torch.float32, torch.bfloat16):
    bf16 = dtype == torch.bfloat16
    docs = docs32.to(torch.bfloat16) if bf16 else docs32
    for B in (32, 1024):
        q = bench.gen_queries(B, dev, seed=B)
        ws = torch.empty(getattr(L, "tt_score_topk_bf16_workspace_bytes" if bf16 else "tt_score_topk_workspace_bytes")(B, n, D_, K),
                         dtype=torch.uint8, device=dev)
        cws = torch.empty(L.tt_score_count_workspace_bytes(B, n, D_, int(bf16)), dtype=torch.uint8, device=dev)
        vals, _ = tt.score_topk(q, docs, K, 0, ws)
        thr = vals[:, K - 1].contiguous()                 # each query's 10th best score: the count is 10 (plus ties)
        out = torch.empty(B, dtype=torch.int64, device=dev)
        fns = {"topk": lambda: tt.score_topk(q, docs, K, 0, ws),
               "count": count_call(L, bf16, q, docs, None, thr, out, cws),
               "count_half": count_call(L, bf16, q, docs, keep_half, thr, out, cws)}
        fns["count"]()
        torch.cuda.synchronize()
        counted = out.tolist()
        t = interleaved(fns, iters=3 if B > 64 else 20)
        base = t["topk"][0]
        emit(leg="count", dtype=str(dtype).split(".")[1], B=B, docs=n, counts_min_max=[min(counted), max(counted)],
             **{f"{name}_ms": ms(v) for name, v in t.items()},
             topk_spread=round((t["topk"][2] - t["topk"][1]) / base, 4),
             count_over_topk=round(t["count"][0] / base, 4), count_half_over_topk=round(t["count_half"][0] / base, 4))
        if ab and B == 1024:                              # what the pacing gate buys the counting pass
            lab = C.CDLL(ab)
            paced = count_call(lab, bf16, q, docs, None, thr, out, cws)

            def unpaced():
                os.environ["TT_SCORE_PACE"] = "0"
                try:
                    paced()
                finally:
                    del os.environ["TT_SCORE_PACE"]

            t = interleaved({"paced": paced, "unpaced": unpaced}, iters=3)
            emit(leg="count_pacing", dtype=str(dtype).split(".")[1], B=B, docs=n, paced_ms=ms(t["paced"]), unpaced_ms=ms(t["unpaced"]),
                 unpaced_over_paced=round(t["unpaced"][0] / t["paced"][0], 4))
    del docs

ix = tt.BruteForceIndex(docs32, screen=True)
for B in (32, 1024):
    q = bench.gen_queries(B, dev, seed=B)
    thr = ix.search(q, K)[0][:, K - 1].contiguous()
    t = interleaved({"search": lambda: ix.search(q, K), "range_search": lambda: ix.range_search(q, thr, K),
                     "count": lambda: ix.count(q, thr)}, iters=3 if B > 64 else 20)
    emit(leg="screened_index", B=B, docs=n, **{f"{name}_ms": ms(v) for name, v in t.items()},
         search_spread=round((t["search"][2] - t["search"][1]) / t["search"][0], 4),
         range_over_search=round(t["range_search"][0] / t["search"][0], 4))
del ix

if parent:
    old = C.CDLL(parent)
    f_old, f_new = bind(old, "tt_score_topk_f32"), L.tt_score_topk_f32
    st = torch.cuda.current_stream().cuda_stream
    for B in (32, 1024):
        q = bench.gen_queries(B, dev, seed=B)
        ws = torch.empty(L.tt_score_topk_workspace_bytes(B, n, D_, K), dtype=torch.uint8, device=dev)
        outs = {}

        def call(fn, tag):
            v, i = outs.setdefault(tag, (torch.empty((B, K), device=dev), torch.empty((B, K), dtype=torch.int64, device=dev)))
            _lib.check(fn(q.data_ptr(), B, D_, docs32.data_ptr(), n, K, 0, v.data_ptr(), i.data_ptr(), ws.data_ptr(), ws.numel(), st))

        t = interleaved({"parent": lambda: call(f_old, "parent"), "this": lambda: call(f_new, "this")}, iters=3 if B > 64 else 20)
        torch.cuda.synchronize()
        same = bool(torch.equal(outs["parent"][0], outs["this"][0]) and torch.equal(outs["parent"][1], outs["this"][1]))
        emit(leg="topk_vs_parent", B=B, docs=n, identical=same, parent_ms=ms(t["parent"]), this_ms=ms(t["this"]),
             this_over_parent=round(t["this"][0] / t["parent"][0], 4))
