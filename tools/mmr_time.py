#!/usr/bin/env python3
"""Diversified selection, event timing with interleaved rounds on one build and one GPU, over [docs] x 256 rows (default 10M),
uniformly random candidate ids (the method of tools/score_ids_time.py).
  leg "kernel"      tt_mmr_select_f32 / _bf16 alone (mmr_select on ready lists) at (B, C, k) = (1, 64, 10), (1024, 128, 10) and
                    (1024, 128, 64), beside the stock-torch composition a caller writes without it: gather the candidates'
                    rows, bmm them into the Gram, then k greedy steps of a few launches each (it is not the project's defined
                    score -- bmm's summation order is its own -- so its picks may differ; only its time is compared).
                    Per leg: both times, the ratio, the algorithmic bytes of the gather and the Gram's flop.
  leg "end_to_end"  BruteForceIndex.diverse_search(q, 10) (fetch_k = 40) against search(q, 40) on the same screened index, at
                    B = 1 and B = 1024: what the selection adds to the search that feeds it.
The tool exits with status 1 (and a FAILED line) when a B = 1 kernel leg is not faster than the torch composition.  That is the
only condition; every other figure is recorded.  One JSON line per measurement (times in ms: median, and min..max over the rounds).
Usage: mmr_time.py [docs] > profiles/mmr_time.log"""
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch

import bench
import twotowermlretrieval_amd as tt

n = int(sys.argv[1]) if len(sys.argv) > 1 else bench.N_DOCS
dev = torch.device("cuda:0")
D_, ROUNDS, LAM = bench.DIM, 7, 0.5


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


def ms(t, nd=5):
    return [round(x, nd) for x in t]


def torch_mmr(vals, idx, docs, k, lam):
    """The composition from stock torch ops: gather, bmm, k steps of (penalised score, mask, argmax, scatter, gather, max)."""
    B, C = vals.shape
    X = docs[idx].to(torch.float32)
    G = torch.bmm(X, X.transpose(1, 2))
    a = lam * vals
    pen = torch.full_like(vals, float("-inf"))
    taken = torch.zeros_like(vals, dtype=torch.bool)
    pos = torch.empty((B, k), dtype=torch.int64, device=vals.device)
    rows = torch.arange(B, device=vals.device)
    for t in range(k):
        m = a if t == 0 else a - (1.0 - lam) * pen
        s = m.masked_fill(taken, float("-inf")).argmax(1)
        pos[:, t] = s
        taken[rows, s] = True
        pen = torch.maximum(pen, G[rows, s])
    return vals.gather(1, pos), idx.gather(1, pos)


g = torch.Generator(device=dev).manual_seed(0)
docs32 = bench.gen_rows(0, n, dev)
docs16 = docs32.to(torch.bfloat16)
failed = []

# ---- the kernel alone, against the torch composition
for docs in (docs32, docs16):
    s = docs.element_size()
    name = "bf16" if s == 2 else "f32"
    for B, C, k in ((1, 64, 10), (1024, 128, 10), (1024, 128, 64)):
        idx = torch.randint(0, n, (B, C), device=dev, generator=g)
        vals = torch.rand((B, C), device=dev, generator=g).sort(1, descending=True).values.contiguous()
        t = interleaved({"kernel": lambda: tt.mmr_select(vals, idx, docs, k, LAM),
                         "torch": lambda: torch_mmr(vals, idx, docs, k, LAM)}, iters=20 if B == 1 else 5)
        faster = bool(t["kernel"][2] < t["torch"][1])
        emit(leg="kernel", rows=name, docs=n, d=D_, B=B, C=C, k=k, kernel_ms=ms(t["kernel"]), torch_composition_ms=ms(t["torch"]),
             torch_over_kernel=round(t["torch"][0] / t["kernel"][0], 1), kernel_is_faster=faster,
             gather_bytes=B * C * D_ * s, gather_GBps=round(B * C * D_ * s / t["kernel"][0] / 1e6, 1),
             gram_flop=2 * B * C * C * D_, gram_GFLOPs_full_square=round(2 * B * C * C * D_ / t["kernel"][0] / 1e6, 1))
        if B == 1 and not faster:
            failed.append(f"kernel {name} B=1: tt_mmr_select is not faster than the torch composition")

# ---- end to end: what the selection adds to the search that feeds it
ix = tt.BruteForceIndex(docs32, screen=True)
for B in (1, 1024):
    q = bench.gen_queries(B, dev, seed=B)
    t = interleaved({"diverse": lambda: ix.diverse_search(q, 10, LAM), "search": lambda: ix.search(q, 40)}, iters=5)
    emit(leg="end_to_end", docs=n, B=B, k=10, fetch_k=40, screened=bool(ix._screens(B, 40)), diverse_search_ms=ms(t["diverse"]),
         search_fetch_k_ms=ms(t["search"]), selection_adds_ms=round(t["diverse"][0] - t["search"][0], 5),
         diverse_over_search=round(t["diverse"][0] / t["search"][0], 3))

if failed:
    for f in failed:
        print("FAILED: " + f, file=sys.stderr, flush=True)
        emit(leg="FAILED", what=f)
    sys.exit(1)
