#!/usr/bin/env python3
"""Cursor search against the masked call of the SAME build, event timing with interleaved rounds on one GPU, over 10M x 256
rows (fp32 and bf16), k = 10.

 * open: B = 32 and B = 1024, the cursor call under the open cursor (+inf, -1) against the masked call with an all-ones
   keep-bitmask -- the yardstick, whose code the cursor feature does not touch.  Both results are compared for equality first.
 * deep: the cursor at each query's 640th result (from one search(k = 1024)) against the open cursor.  A tile whose only scores
   above the threshold were returned by earlier pages must not enter the append pass, so the ratio should be about 1.
 * use case: results 1025..1088 through one search_after (the cursor is the 1024th result) against score_all + topk(1088)
   -- the [B, N] matrix a deep page otherwise costs -- at B = 32 over the first `dense_docs` rows (default 4M).

One JSON line per measurement (times in ms: median, and min..max over the rounds; spread = (max - min) / median of each
side's own repeats).
Usage: cursor_time.py [docs [dense_docs]]"""
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
K, ROUNDS, DEEP = 10, 5, 640
INF = float("inf")


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


def spread(t):
    return round((t[2] - t[1]) / t[0], 4)


ones = tt.pack_keep_mask(torch.ones(n, dtype=torch.bool, device=dev))
docs32 = bench.gen_rows(0, n, dev)
for dtype in (torch.float32, torch.bfloat16):
    docs = docs32 if dtype == torch.float32 else docs32.to(torch.bfloat16)
    name = str(dtype).split(".")[1]
    for B in (32, 1024):
        q = bench.gen_queries(B, dev, seed=B)
        open_v = torch.full((B,), INF, dtype=torch.float32, device=dev)
        open_i = torch.full((B,), -1, dtype=torch.int64, device=dev)
        pv, pi = tt.score_topk(q, docs, 1024)                # the first 1024 results: the deep cursor, and its expected page
        deep_v, deep_i = pv[:, DEEP - 1].contiguous(), pi[:, DEEP - 1].contiguous()
        fns = {"masked_all_ones": lambda: tt.score_topk(q, docs, K, keep=ones),
               "cursor_open": lambda: tt.score_topk_after(q, docs, open_v, open_i, K),
               "cursor_deep": lambda: tt.score_topk_after(q, docs, deep_v, deep_i, K)}
        identical = same(fns["masked_all_ones"](), fns["cursor_open"]())
        deep_identical = same(fns["cursor_deep"](), (pv[:, DEEP:DEEP + K], pi[:, DEEP:DEEP + K]))
        t = interleaved(fns, iters=3 if B > 64 else 20)
        base, mine, deep = t["masked_all_ones"], t["cursor_open"], t["cursor_deep"]
        emit(leg="open_and_deep", dtype=name, B=B, docs=n, identical=identical, deep_page_identical=deep_identical,
             **{f"{k}_ms": [round(x, 4) for x in v] for k, v in t.items()},
             masked_spread=spread(base), open_spread=spread(mine), deep_spread=spread(deep),
             open_over_masked=round(mine[0] / base[0], 4), deep_over_open=round(deep[0] / mine[0], 4))
        del pv, pi
    del docs

# the use case, fp32 rows: the dense idiom materialises [B, n_dense] floats
B = 32
q = bench.gen_queries(B, dev, seed=B)
sub = docs32[:n_dense]
ix = tt.BruteForceIndex(sub)
pv, pi = ix.search(q, 1024)
after = (pv[:, -1].contiguous(), pi[:, -1].contiguous())


def dense():
    v, i = torch.topk(tt.score_all(q, sub), 1088, dim=1)
    return v[:, 1024:], i[:, 1024:]


def fused():
    return ix.search_after(q, 64, after)


a, b = dense(), fused()
t = interleaved({"score_all_topk_1088": dense, "one_search_after": fused}, iters=3, rounds=3)
emit(leg="use_case", dtype="float32", B=B, docs=n_dense, results="1025..1088", values_identical=bool(torch.equal(a[0], b[0])),
     indices_identical=bool(torch.equal(a[1], b[1])), dense_matrix_mb=round(B * n_dense * 4 / 2 ** 20, 1),
     **{f"{k}_ms": [round(x, 4) for x in v] for k, v in t.items()},
     dense_over_cursor=round(t["score_all_topk_1088"][0] / t["one_search_after"][0], 3))
