#!/usr/bin/env python3
"""Fused lists, event timing with interleaved rounds on one build and one GPU.
  leg "fuse"    tt_topk_fuse_rank_f32 alone (fuse_topk over a packed [B,L,M] pair, out= given) at (B, L, M, k) = (1024, 2, 512,
                10), (32, 8, 128, 10) and (1024, 2, 64, 10) -- HybridIndex's default fetch -- against the same rule written with
                stock torch ops on the device: cat, a stable sort by id, segment sums (scatter_add over the runs of equal ids),
                a stable descending sort, the first k.  Every list holds M distinct ids out of 2 M, so two lists share about
                half of them.  The torch form assumes what a search guarantees (no id twice in a list) and adds a segment's
                terms in whatever order the atomics land, so for L > 2 its sums can differ in the last bit: the log says how
                many result ids agree and the largest difference of the values.  The launches are enqueued back to back from
                Python, so a figure of some 10 us is the host's enqueue rate as much as the kernel's time.
  leg "hybrid"  [docs] x 256 rows (default 1M) in a BruteForceIndex and a Zipf CSR of the same size in a LexicalIndex
                (tools/lexical_bench.py's corpus), B = 32 queries: HybridIndex.search(q, q_lex, 10) against the two searches it
                makes (dense at 64, lexical at 64), each alone and one after the other, so the difference is the packing and
                the fuse launch.
One JSON line per measurement (times in ms: median, and min..max over the rounds); "spread" = (max - min) / median of a
measurement's own rounds.  Usage: fuse_time.py [docs] > profiles/fuse_time.log"""
import json
import sys
from pathlib import Path

sys.path[:0] = [str(Path(__file__).resolve().parent.parent), str(Path(__file__).resolve().parent)]
import torch

import bench
import lexical_bench
import twotowermlretrieval_amd as tt
from twotowermlretrieval_amd.fusion import _fuse_packed

n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
dev = torch.device("cuda:0")
ROUNDS = 7


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


def torch_rule(idx, table, k):
    """Reciprocal rank fusion with stock torch ops: idx [B,L,M] (no id twice in a list), table [L,M] -> (vals [B,k], idx [B,k]),
    (fused desc, id asc), tail (-inf, -1).  missing = 0."""
    B, L, M = idx.shape
    E = L * M
    big = torch.iinfo(torch.int64).max
    ids = torch.where(idx >= 0, idx, torch.full_like(idx, big)).reshape(B, E)      # padding sorts last
    term = table.reshape(1, E).expand(B, E)
    ids, perm = torch.sort(ids, dim=1, stable=True)
    term = term.gather(1, perm)
    start = torch.ones((B, E), dtype=torch.bool, device=idx.device)
    start[:, 1:] = ids[:, 1:] != ids[:, :-1]
    seg = torch.cumsum(start, 1) - 1                                                # the run of equal ids an entry belongs to
    fused = torch.zeros((B, E), device=idx.device).scatter_add_(1, seg, term)
    uid = torch.full((B, E), big, dtype=torch.int64, device=idx.device).scatter_(1, seg, ids)   # ascending: ids were sorted
    fused = torch.where(uid != big, fused, torch.full_like(fused, float("-inf")))
    v, order = torch.sort(fused, dim=1, descending=True, stable=True)               # stable: id asc inside a tie
    i = uid.gather(1, order[:, :k])
    return v[:, :k], torch.where(i != big, i, torch.full_like(i, -1))


g_ = torch.Generator(device=dev).manual_seed(0)
for B, L, M, k in ((1024, 2, 512, 10), (32, 8, 128, 10), (1024, 2, 64, 10)):
    idx = torch.stack([torch.stack([torch.randperm(2 * M, device=dev, generator=g_)[:M] for _ in range(L)]) for _ in range(B)])
    table = tt.rrf_weights(L, M).to(dev)
    out = (torch.empty((B, k), device=dev), torch.empty((B, k), dtype=torch.int64, device=dev))
    pos = torch.empty((B, k, L), dtype=torch.int32, device=dev)
    _fuse_packed(None, idx, k, "rrf", 60.0, table, None, None, False, out)
    want = torch_rule(idx, table, k)
    torch.cuda.synchronize()
    t = interleaved({"fuse": lambda: _fuse_packed(None, idx, k, "rrf", 60.0, table, None, None, False, out),
                     "fuse_pos": lambda: _fuse_packed(None, idx, k, "rrf", 60.0, table, None, None, True, (*out, pos)),
                     "torch": lambda: torch_rule(idx, table, k)}, iters=50)
    emit(leg="fuse", B=B, L=L, M=M, k=k, union_mean=round(sum(torch.unique(r).numel() for r in idx[:32]) / 32, 1),
         ids_equal_to_the_torch_rule=round(float((out[1] == want[1]).float().mean()), 5),
         max_value_difference=float((out[0] - want[0]).abs().max()),
         fuse_ms=[round(x, 5) for x in t["fuse"]], fuse_with_positions_ms=[round(x, 5) for x in t["fuse_pos"]],
         torch_ms=[round(x, 5) for x in t["torch"]], fuse_spread=spread(t["fuse"]), torch_spread=spread(t["torch"]),
         us_per_row=round(1e3 * t["fuse"][0] / B, 3), torch_over_fuse=round(t["torch"][0] / t["fuse"][0], 2))

B, K, FETCH = 32, 10, 64
dense = tt.BruteForceIndex(bench.gen_rows(0, n, dev), screen=True)
indptr, cols, vals = lexical_bench.zipf_csr(n, 5, dev)
lex = tt.LexicalIndex((indptr, cols, vals, lexical_bench.F))
hy = tt.HybridIndex(dense, lex)
q = bench.gen_queries(B, dev, seed=B)
qs = [lexical_bench.zipf_query(6, 100 + b, dev) for b in range(B)]
q_indptr = torch.zeros(B + 1, dtype=torch.int64, device=dev)
q_indptr[1:] = torch.cumsum(torch.tensor([c.numel() for _, c, _ in qs], device=dev), 0)
q_lex = (q_indptr, torch.cat([c for _, c, _ in qs]), torch.cat([v for _, _, v in qs]))
got = hy.search(q, q_lex, K, return_components=True)
torch.cuda.synchronize()
in_both = float((~torch.isnan(got[2]) & ~torch.isnan(got[3])).float().mean())


def both():
    dense.search(q, FETCH)
    lex.search(q_lex, FETCH)


t = interleaved({"dense_k64": lambda: dense.search(q, FETCH), "lexical_k64": lambda: lex.search(q_lex, FETCH), "both": both,
                 "hybrid_k10": lambda: hy.search(q, q_lex, K),
                 "hybrid_k10_components": lambda: hy.search(q, q_lex, K, return_components=True)}, iters=5)
emit(leg="hybrid", B=B, docs=n, k=K, fetch_k=FETCH, nnz=int(cols.numel()), results_in_both_lists=round(in_both, 4),
     **{f"{name}_ms": [round(x, 4) for x in v] for name, v in t.items()}, both_spread=spread(t["both"]),
     hybrid_over_both=round(t["hybrid_k10"][0] / t["both"][0], 4), difference_ms=round(t["hybrid_k10"][0] - t["both"][0], 4))
