#!/usr/bin/env python3
"""Candidate search, event timing with interleaved rounds on one build and one GPU, over [docs] x 256 rows (default 10M).
  leg "gather"       tt_score_ids_f32 / _bf16 alone at B = 1024, C in {64, 1024}, uniformly random ids: time, the algorithmic
                     bytes (B*C*d*s of rows + ids + outputs + Q) and GB/s, beside the kernel guide's figure for random whole
                     rows of ~1 KB from a table far larger than the caches (5.5-5.6 TB/s chip-wide; a reference point, not a
                     bar; the guide has no figure for 512-byte rows).
  leg "rerank_b1"    B = 1, C = 1024, k = 10: search(q, 10, candidates=ids) against the only route to the same answer without
                     it, search(q, 10, keep=pack_keep_mask(<the candidate set>)) on the same index, which streams all N rows.
                     The results must be equal and the candidate search the faster of the two.
  leg "rerank_b1024" B = 1024, C = 1024, k = 10: the whole search, and its scoring launch and merge launch alone; and k = 100,
                     where repeats are turned into padding (a row-wise sort) in front of the large merge.
The tool exits with status 1 (and a FAILED line) when the B = 1 results differ or the candidate search is not the faster.
One JSON line per measurement (times in ms: median, and min..max over the rounds).
Usage: score_ids_time.py [docs] > profiles/score_ids_time.log"""
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch

import bench
import twotowermlretrieval_amd as tt
from twotowermlretrieval_amd import index as ttx

n = int(sys.argv[1]) if len(sys.argv) > 1 else bench.N_DOCS
dev = torch.device("cuda:0")
D_, ROUNDS = bench.DIM, 7
GUIDE = {4: "5.5-5.6 TB/s for random 1152-byte rows gathered into registers (MI355X_MICROARCH.md, Indexed rows)",
         2: "not measured there (no figure for 512-byte rows)"}


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


g = torch.Generator(device=dev).manual_seed(0)
docs32 = bench.gen_rows(0, n, dev)
docs16 = docs32.to(torch.bfloat16)

# ---- gather: the kernel alone
B = 1024
q = bench.gen_queries(B, dev, seed=B)
for docs in (docs32, docs16):
    s = docs.element_size()
    for C in (64, 1024):
        ids = torch.randint(0, n, (B, C), device=dev, generator=g)
        ov = torch.empty((B, C), dtype=torch.float32, device=dev)
        oi = torch.empty((B, C), dtype=torch.int64, device=dev)
        t = interleaved({"k": lambda: ttx._score_ids_into(q, docs, ids, 0, None, ov, oi)}, iters=20)["k"]
        nbytes = B * C * D_ * s + B * C * (8 + 4 + 8) + B * D_ * 4
        emit(leg="gather", rows="bf16" if s == 2 else "f32", docs=n, d=D_, B=B, C=C, row_bytes=D_ * s, kernel_ms=ms(t),
             algorithmic_bytes=nbytes, GBps=round(nbytes / t[0] / 1e6, 1), GBps_best=round(nbytes / t[1] / 1e6, 1),
             guide_reference=GUIDE[s])

# ---- rerank, B = 1: against the masked search of the whole corpus
ix = tt.BruteForceIndex(docs32)
K, C = 10, 1024
q1 = bench.gen_queries(1, dev, seed=1)
ids1 = torch.randint(0, n, (1, C), device=dev, generator=g)
member = torch.zeros(n, dtype=torch.bool, device=dev)
member[ids1[0]] = True
mask = tt.pack_keep_mask(member)
a = ix.search(q1, K, candidates=ids1)
b = ix.search(q1, K, keep=mask)
torch.cuda.synchronize()
same = bool(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]))
t = interleaved({"candidates": lambda: ix.search(q1, K, candidates=ids1), "masked": lambda: ix.search(q1, K, keep=mask)}, iters=10)
emit(leg="rerank_b1", docs=n, B=1, C=C, k=K, results_equal=same, candidates_ms=ms(t["candidates"]), masked_search_ms=ms(t["masked"]),
     masked_over_candidates=round(t["masked"][0] / t["candidates"][0], 1), candidates_is_faster=bool(t["candidates"][2] < t["masked"][1]))
failed = []
if not same:
    failed.append("rerank_b1: search(candidates=) and the masked search returned different rows")
if not t["candidates"][2] < t["masked"][1]:
    failed.append("rerank_b1: the candidate search is not faster than the masked search of the whole corpus")

# ---- rerank, B = 1024: the scoring launch and the merge launch
ids = torch.randint(0, n, (B, C), device=dev, generator=g)
sv = torch.empty((B, C), dtype=torch.float32, device=dev)
si = torch.empty((B, C), dtype=torch.int64, device=dev)
out = ttx._out_pair(B, K, dev)
ttx._score_ids_into(q, docs32, ids, 0, None, sv, si)
t = interleaved({"search": lambda: ix.search(q, K, candidates=ids, out=out),
                 "score": lambda: ttx._score_ids_into(q, docs32, ids, 0, None, sv, si),
                 "merge": lambda: ttx._merge_candidates(sv, si, K, out)}, iters=10)
emit(leg="rerank_b1024", docs=n, B=B, C=C, k=K, search_ms=ms(t["search"]), score_launch_ms=ms(t["score"]),
     merge_launch_ms=ms(t["merge"]), merge_share_of_launches=round(t["merge"][0] / (t["merge"][0] + t["score"][0]), 3))

# ---- the same above k = 64: repeats become padding first (_unique_pairs), then the large merge
KL = 100
outl = ttx._out_pair(B, KL, dev)
t = interleaved({"search": lambda: ix.search(q, KL, candidates=ids, out=outl),
                 "unique": lambda: ttx._unique_pairs(sv, si),
                 "merge": lambda: ttx._merge_candidates(sv, si, KL, outl)}, iters=10)
emit(leg="rerank_b1024_k100", docs=n, B=B, C=C, k=KL, search_ms=ms(t["search"]), unique_pairs_ms=ms(t["unique"]),
     unique_and_merge_ms=ms(t["merge"]), score_launch_ms="as in rerank_b1024")

if failed:
    for f in failed:
        print("FAILED: " + f, file=sys.stderr, flush=True)
        emit(leg="FAILED", what=f)
    sys.exit(1)
