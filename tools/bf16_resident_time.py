#!/usr/bin/env python3
"""bf16-resident index vs the fp32 (+ fp16 shadow) index, event timing with interleaved A/B rounds on one GPU:
  1. the screened fp32 + shadow index vs the screened bf16 index over the same 10M x 256 rows, B in {1, 32, 1024}, k = 10;
  2. the exact kernels alone at B = 32: tt_score_topk_f32 over the widened rows vs tt_score_topk_bf16 (fraction of HBM
     peak over the bytes each one streams);
  3. a 100M x 256 bf16 index resident on one GPU (51.2 GB), at B = 1024 and B = 32.
One JSON line per measurement.  Usage: bf16_resident_time.py [docs] [big_docs]  (0 skips the 100M leg)."""
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch

import bench
import twotowermlretrieval_amd as tt

HBM_GBPS = 8000.0  # MI355X peak HBM bandwidth
n = int(sys.argv[1]) if len(sys.argv) > 1 else bench.N_DOCS
big = int(sys.argv[2]) if len(sys.argv) > 2 else 100_000_000
dev = torch.device("cuda:0")


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


def ab(fa, fb, iters, rounds=3):
    """Interleaved A/B: rounds x (A, B), the median of each side (ms)."""
    ta, tb = [], []
    for _ in range(rounds):
        ta.append(timeit(fa, iters))
        tb.append(timeit(fb, iters))
    return sorted(ta)[len(ta) // 2], sorted(tb)[len(tb) // 2]


def emit(**kw):
    print(json.dumps(kw), flush=True)


docs_b = bench.gen_rows(0, n, dev).to(torch.bfloat16)
docs_w = docs_b.float()
ix_f = tt.BruteForceIndex(docs_w, screen=True)   # fp32 rows + fp16 shadow: 6 bytes per element
ix_b = tt.BruteForceIndex(docs_b, screen=True)   # bf16 rows: 2 bytes per element, screened from them
for B in (1, 32, 1024):
    q = bench.gen_queries(B, dev, seed=B)
    vf, i_f = ix_f.search(q, 10)
    vb, ib = ix_b.search(q, 10)
    same = bool(torch.equal(vf, vb) and torch.equal(i_f, ib))
    tf, tb = ab(lambda: ix_f.search(q, 10), lambda: ix_b.search(q, 10), iters=3 if B > 64 else 10)
    emit(leg="index", B=B, docs=n, f32_shadow_ms=round(tf, 4), bf16_ms=round(tb, 4), bf16_over_f32_shadow=round(tb / tf, 3),
         hbm_bytes_f32_shadow=n * 256 * 6, hbm_bytes_bf16=n * 256 * 2, identical=same)

q = bench.gen_queries(32, dev, seed=32)
tf, tb = ab(lambda: tt.score_topk(q, docs_w, 10), lambda: tt.score_topk(q, docs_b, 10), iters=10)
emit(leg="k4_b32", docs=n, f32_ms=round(tf, 4), bf16_ms=round(tb, 4), bf16_over_f32=round(tb / tf, 3),
     f32_hbm_frac=round(n * 1024 / tf / 1e6 / HBM_GBPS, 3), bf16_hbm_frac=round(n * 512 / tb / 1e6 / HBM_GBPS, 3))
del ix_f, ix_b, docs_w, docs_b
torch.cuda.empty_cache()

if big > 0:
    step = 10_000_000
    docs = torch.empty((big, 256), dtype=torch.bfloat16, device=dev)
    for lo in range(0, big, step):
        hi = min(big, lo + step)
        docs[lo:hi] = bench.gen_rows(lo, hi, dev).to(torch.bfloat16)
    ix = tt.BruteForceIndex(docs, screen=True)
    for B in (1024, 32):
        q = bench.gen_queries(B, dev, seed=B)
        t = timeit(lambda: ix.search(q, 10), iters=2 if B > 64 else 5)
        emit(leg="resident_100m", B=B, docs=big, hbm_gb=round(big * 512 / 1e9, 1), ms=round(t, 3),
             queries_per_s=round(B / t * 1e3, 1), hbm_frac=round(big * 512 / t / 1e6 / HBM_GBPS, 3),
             mem_allocated_gb=round(torch.cuda.memory_allocated() / 1e9, 1))
