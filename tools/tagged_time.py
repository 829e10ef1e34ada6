#!/usr/bin/env python3
"""Tagged search against the masked call of the SAME build, event timing with interleaved rounds on one GPU, over 10M x 256
rows (fp32 and bf16), k = 10.

 * ratio: B = 32 and B = 1024, the tagged call with every document eligible (mask 0, value 0) against the masked call with an
   all-ones keep-bitmask -- the yardstick, whose code the tagged feature does not touch.  The tags add 4 bytes per document to
   d * 4 (or d * 2) of row: 0.4 % fp32, 0.8 % bf16 at d = 256.  Both results are compared for equality first.
 * use case: B = 1024 over 8 tenants (tags = n % 8, query b wants b % 8) as ONE tagged call, against the 8 masked calls of 128
   queries each that the same batch takes without tags (the keep-bitmasks are built beforehand and not timed); and the same
   over 128 tenants, 8 queries each, where every masked call is a corpus scan of its own.

One JSON line per measurement (times in ms: median, and min..max over the rounds; spread = (max - min) / median of the
yardstick's own repeats).
Usage: tagged_time.py [docs]"""
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch

import bench
import twotowermlretrieval_amd as tt

args = sys.argv[1:]
n = int(args[0]) if args else bench.N_DOCS
dev = torch.device("cuda:0")
K, ROUNDS, MANY = 10, 5, (8, 128)


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
pad = 32 * ((n + 31) // 32)
tenant = torch.zeros(pad, dtype=torch.int32, device=dev)
docs32 = bench.gen_rows(0, n, dev)
for dtype in (torch.float32, torch.bfloat16):
    docs = docs32 if dtype == torch.float32 else docs32.to(torch.bfloat16)
    name = str(dtype).split(".")[1]
    for B in (32, 1024):
        q = bench.gen_queries(B, dev, seed=B)
        zero = torch.zeros(B, dtype=torch.int32, device=dev)
        fns = {"masked_all_ones": lambda: tt.score_topk(q, docs, K, keep=ones),
               "tagged_all_eligible": lambda: tt.score_topk_tagged(q, docs, tenant, zero, zero, K)}
        identical = same(fns["masked_all_ones"](), fns["tagged_all_eligible"]())
        t = interleaved(fns, iters=3 if B > 64 else 20)
        base = t["masked_all_ones"]
        emit(leg="ratio", dtype=name, B=B, docs=n, identical=identical,
             **{f"{k}_ms": [round(x, 4) for x in v] for k, v in t.items()},
             masked_spread=round((base[2] - base[1]) / base[0], 4),
             tagged_spread=round((t["tagged_all_eligible"][2] - t["tagged_all_eligible"][1]) / t["tagged_all_eligible"][0], 4),
             tagged_over_masked=round(t["tagged_all_eligible"][0] / base[0], 4))
    # the use case: 1024 queries over 8 tenants (128 queries per filter: the masked calls are MFMA-bound like the one tagged
    # call), and over 128 tenants (8 queries per filter: every masked call is a scan of its own)
    B = 1024
    q = bench.gen_queries(B, dev, seed=B)
    full = torch.full((B,), -1, dtype=torch.int32, device=dev)
    for tenants in MANY:
        tenant[:n] = torch.arange(n, device=dev, dtype=torch.int32) % tenants
        keeps = [tt.pack_keep_mask(tenant[:n] == t) for t in range(tenants)]
        want = torch.arange(B, device=dev, dtype=torch.int32) % tenants
        groups = [torch.nonzero(want == t).flatten() for t in range(tenants)]
        subq = [q[g].contiguous() for g in groups]

        def one_tagged():
            return tt.score_topk_tagged(q, docs, tenant, full, want, K)

        def masked_per_tenant():
            return [tt.score_topk(subq[t], docs, K, keep=keeps[t]) for t in range(tenants)]

        got, parts = one_tagged(), masked_per_tenant()
        identical = all(same((got[0][g], got[1][g]), p) for g, p in zip(groups, parts))
        t = interleaved({"one_tagged_call": one_tagged, "masked_call_per_tenant": masked_per_tenant}, iters=3, rounds=3)
        emit(leg="use_case", dtype=name, B=B, tenants=tenants, queries_per_tenant=B // tenants, docs=n, identical=identical,
             **{f"{k}_ms": [round(x, 4) for x in v] for k, v in t.items()},
             masked_over_tagged=round(t["masked_call_per_tenant"][0] / t["one_tagged_call"][0], 3))
        del keeps
    del docs
