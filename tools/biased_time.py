#!/usr/bin/env python3
"""Biased search against the masked call of the SAME build, event timing with interleaved rounds on one GPU, over 10M x 256
rows (fp32 and bf16), k = 10.

 * ratio: B = 32 and B = 1024, the biased call with a bias of zeros against the masked call with an all-ones keep-bitmask --
   the yardstick, whose code the biased feature does not touch.  The biases add 4 bytes per document to d * 4 (or d * 2) of
   row: 0.4 % fp32, 0.8 % bf16 at d = 256.  Both results are compared for equality first.
 * use case: one biased call against score_all + add + topk -- the [B, N] matrix the call exists to avoid -- at B = 32 over
   the first `dense_docs` rows (default 4M: 512 MB of scores, and torch.topk's workspace on top).

One JSON line per measurement (times in ms: median, and min..max over the rounds; spread = (max - min) / median of each
side's own repeats).
Usage: biased_time.py [docs [dense_docs]]"""
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch

import bench
import twotowermlretrieval_amd as tt

args = sys.argv[1:]
n = int(args[0]) if args else bench.N_DOCS
n_dense = min(int(args[1]) if len(args) > 1 else 4_000_000, n)
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


def same(a, b):
    return bool(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]))


ones = tt.pack_keep_mask(torch.ones(n, dtype=torch.bool, device=dev))
zero_bias = torch.zeros(32 * ((n + 31) // 32), dtype=torch.float32, device=dev)
docs32 = bench.gen_rows(0, n, dev)
for dtype in (torch.float32, torch.bfloat16):
    docs = docs32 if dtype == torch.float32 else docs32.to(torch.bfloat16)
    name = str(dtype).split(".")[1]
    for B in (32, 1024):
        q = bench.gen_queries(B, dev, seed=B)
        fns = {"masked_all_ones": lambda: tt.score_topk(q, docs, K, keep=ones),
               "biased_zero": lambda: tt.score_topk_biased(q, docs, zero_bias, K)}
        identical = same(fns["masked_all_ones"](), fns["biased_zero"]())
        t = interleaved(fns, iters=3 if B > 64 else 20)
        base, mine = t["masked_all_ones"], t["biased_zero"]
        emit(leg="ratio", dtype=name, B=B, docs=n, identical=identical,
             **{f"{k}_ms": [round(x, 4) for x in v] for k, v in t.items()},
             masked_spread=round((base[2] - base[1]) / base[0], 4), biased_spread=round((mine[2] - mine[1]) / mine[0], 4),
             biased_over_masked=round(mine[0] / base[0], 4))
    del docs

# the use case, fp32 rows: the dense idiom materialises [B, n_dense] floats
B = 32
q = bench.gen_queries(B, dev, seed=B)
sub = docs32[:n_dense]
g = torch.Generator(device=dev).manual_seed(7)
prior = torch.randn(n_dense, device=dev, generator=g).mul_(0.05)


def dense():
    v, i = torch.topk(tt.score_all(q, sub).add_(prior[None, :]), K, dim=1)
    return v, i


def fused():
    return tt.score_topk_biased(q, sub, prior, K)


a, b = dense(), fused()
t = interleaved({"score_all_add_topk": dense, "one_biased_call": fused}, iters=3, rounds=3)
emit(leg="use_case", dtype="float32", B=B, docs=n_dense, values_identical=bool(torch.equal(a[0], b[0])),
     indices_identical=bool(torch.equal(a[1], b[1])), dense_matrix_mb=round(B * n_dense * 4 / 2 ** 20, 1),
     **{f"{k}_ms": [round(x, 4) for x in v] for k, v in t.items()},
     dense_over_biased=round(t["score_all_add_topk"][0] / t["one_biased_call"][0], 3))
