#!/usr/bin/env python3
"""Per-query exclusion, event timing with interleaved rounds on one build and one GPU.
  leg "filter"  tt_topk_exclude_ids alone at B = 1024: (M, E, k) = (15, 5, 10), the direct compare, and (1024, 1000, 24), the
                sorted list; every list is the head of its row (the worst case: the whole row is read).
  leg "search"  [docs] x 256 rows (default 10M), screen=True, B = 1024: search(q, 10, exclude=[B,5]) against search(q, 15) on
                the same index -- the call the exclusion search makes first, and what the parent commit runs for k = 15 (no
                search kernel changed) -- so the difference is the filter launch and one scratch allocation.
One JSON line per measurement (times in ms: median, and min..max over the rounds); "spread" = (max - min) / median of the
baseline's own rounds.  Usage: exclude_time.py [docs] > profiles/exclude_time.log"""
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch

import bench
import twotowermlretrieval_amd as tt

n = int(sys.argv[1]) if len(sys.argv) > 1 else bench.N_DOCS
dev = torch.device("cuda:0")
B, ROUNDS = 1024, 7


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


def spread(t):
    return round((t[2] - t[1]) / t[0], 4)


def emit(**kw):
    print(json.dumps(kw), flush=True)


g = torch.Generator(device=dev).manual_seed(0)
for M, E, k in ((15, 5, 10), (1024, 1000, 24)):
    vals = torch.sort(torch.rand((B, M), device=dev, generator=g), dim=1, descending=True).values
    idx = torch.stack([torch.randperm(4 * M, device=dev, generator=g)[:M] for _ in range(B)])
    ex = idx[:, :E].contiguous()
    out = (torch.empty((B, k), device=dev), torch.empty((B, k), dtype=torch.int64, device=dev))
    tt.topk_exclude(vals, idx, ex, k, out=out)
    torch.cuda.synchronize()
    ok = bool(torch.equal(out[1], idx[:, E:E + k]) and torch.equal(out[0], vals[:, E:E + k]))
    t = interleaved({"filter": lambda: tt.topk_exclude(vals, idx, ex, k, out=out)}, iters=200)["filter"]
    emit(leg="filter", B=B, M=M, E=E, k=k, result_is_the_row_behind_the_list=ok, filter_ms=[round(x, 5) for x in t],
         filter_spread=spread(t))

K, E = 10, 5
ix = tt.BruteForceIndex(bench.gen_rows(0, n, dev), screen=True)
q = bench.gen_queries(B, dev, seed=B)
assert ix._screens(B, K + E)
wide = ix.search(q, K + E)
ex = wide[1][:, :E].contiguous()                                 # every query's own top five
got = ix.search(q, K, exclude=ex)
torch.cuda.synchronize()
ok = bool(torch.equal(got[1], wide[1][:, E:]) and torch.equal(got[0], wide[0][:, E:]))
t = interleaved({"search_k15": lambda: ix.search(q, K + E), "search_k10_exclude5": lambda: ix.search(q, K, exclude=ex)}, iters=5)
emit(leg="search", B=B, docs=n, k=K, E=E, result_is_the_k15_row_behind_the_list=ok,
     **{f"{name}_ms": [round(x, 4) for x in v] for name, v in t.items()}, search_k15_spread=spread(t["search_k15"]),
     exclude_over_k15=round(t["search_k10_exclude5"][0] / t["search_k15"][0], 4),
     difference_ms=round(t["search_k10_exclude5"][0] - t["search_k15"][0], 4))
