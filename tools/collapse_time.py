#!/usr/bin/env python3
"""Collapsed search, event timing with interleaved rounds on one build and one GPU.
  leg "filter"  tt_topk_collapse_gids alone at B = 1024 for (M, k, m) = (64, 10, 1), (1024, 100, 1) and (1024, 256, 3), against
                the same rule written with stock torch ops on the device (a [B,M,M] equality under a strict lower triangle,
                a row sum, a cumulative sum and a scatter).  The rows draw their group ids from M / 4 groups, one in eight
                ungrouped: the whole row is staged, and the k-th kept entry falls into the first 256-entry chunk for the first
                two shapes and into a later one for the third.  A fourth line is the worst case of the third shape: every entry
                of one group, so that all four chunks are counted and compacted.  The launches are enqueued back to back from
                Python, so a figure of some 10 us is the host's enqueue rate as much as the kernel's time.
  leg "search"  [docs] x 256 rows (default 10M), screen=True, B = 1024: collapsed_search(q, 10, fetch_k=64, exact=False)
                against search(q, 64) on the same index -- the call the collapsed search makes first (64 is the widest fetch on
                this side of the routing cliff; the default for k = 10 is 40, timed as well), and what the parent commit runs
                for that fetch (no search kernel changed) -- so the difference is the filter launch and its four outputs.
One JSON line per measurement (times in ms: median, and min..max over the rounds); "spread" = (max - min) / median of the
baseline's own rounds.  Usage: collapse_time.py [docs] > profiles/collapse_time.log"""
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


def torch_rule(vals, idx, gids, k, m):
    """The rule with stock torch ops: (vals [B,k], idx [B,k], gids [B,k]), tail (-inf, -1, -1)."""
    Bq, M = vals.shape
    g = torch.where(idx >= 0, gids, torch.full_like(gids, -1))
    earlier = ((g[:, :, None] == g[:, None, :]) & torch.ones((M, M), dtype=torch.bool, device=g.device).tril(-1)).sum(-1)
    keep = (idx >= 0) & ((g < 0) | (earlier < m))
    pos = torch.cumsum(keep, 1) - 1
    pos = torch.where(keep & (pos < k), pos, torch.full_like(pos, k))        # everything else lands in a spare column
    ov = torch.full((Bq, k + 1), float("-inf"), device=vals.device).scatter_(1, pos, vals)
    oi = torch.full((Bq, k + 1), -1, dtype=torch.int64, device=vals.device).scatter_(1, pos, idx)
    og = torch.full((Bq, k + 1), -1, dtype=torch.int64, device=vals.device).scatter_(1, pos, g)
    return ov[:, :k], oi[:, :k], og[:, :k]


g_ = torch.Generator(device=dev).manual_seed(0)
for M, k, m, one_group in ((64, 10, 1, False), (1024, 100, 1, False), (1024, 256, 3, False), (1024, 256, 3, True)):
    vals = torch.sort(torch.rand((B, M), device=dev, generator=g_), dim=1, descending=True).values
    idx = torch.stack([torch.randperm(4 * M, device=dev, generator=g_)[:M] for _ in range(B)])
    gids = torch.randint(0, max(M // 4, 2), (B, M), device=dev, generator=g_)
    gids[torch.rand((B, M), device=dev, generator=g_) < 0.125] = -1
    if one_group:
        gids.fill_(7)
    out = (torch.empty((B, k), device=dev), torch.empty((B, k), dtype=torch.int64, device=dev),
           torch.empty((B, k), dtype=torch.int64, device=dev), torch.empty((B, 2), dtype=torch.int32, device=dev))
    tt.topk_collapse(vals, idx, k, gids=gids, max_per_group=m, out=out)
    want = torch_rule(vals, idx, gids, k, m)
    torch.cuda.synchronize()
    ok = all(bool(torch.equal(a, b)) for a, b in zip(out[:3], want))
    t = interleaved({"filter": lambda: tt.topk_collapse(vals, idx, k, gids=gids, max_per_group=m, out=out),
                     "torch": lambda: torch_rule(vals, idx, gids, k, m)}, iters=50)
    emit(leg="filter", B=B, M=M, k=k, m=m, one_group=one_group, equals_the_torch_rule=ok, mean_kept=round(float(out[3][:, 0].float().mean()), 1),
         filter_ms=[round(x, 5) for x in t["filter"]], torch_ms=[round(x, 5) for x in t["torch"]],
         filter_spread=spread(t["filter"]), torch_over_filter=round(t["torch"][0] / t["filter"][0], 2))

K, FETCH = 10, 64
ix = tt.BruteForceIndex(bench.gen_rows(0, n, dev), screen=True)
ix.set_groups(torch.arange(n, device=dev) // 4)                  # pages of four consecutive passages
q = bench.gen_queries(B, dev, seed=B)
assert ix._screens(B, FETCH)
got = ix.collapsed_search(q, K, exact=False)
torch.cuda.synchronize()
t = interleaved({"search_k64": lambda: ix.search(q, FETCH),
                 "collapsed_k10_fetch64": lambda: ix.collapsed_search(q, K, fetch_k=FETCH, exact=False),
                 "collapsed_k10_default": lambda: ix.collapsed_search(q, K, exact=False)}, iters=5)
emit(leg="search", B=B, docs=n, k=K, default_fetch_k=tt.index._collapse_fetch_k(K, n), complete_at_default=int(got[3].sum()),
     **{f"{name}_ms": [round(x, 4) for x in v] for name, v in t.items()}, search_k64_spread=spread(t["search_k64"]),
     collapsed_over_k64=round(t["collapsed_k10_fetch64"][0] / t["search_k64"][0], 4),
     difference_ms=round(t["collapsed_k10_fetch64"][0] - t["search_k64"][0], 4))
