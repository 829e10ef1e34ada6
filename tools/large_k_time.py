"""Device-event times of the exact search at large k, with the tier of every query.

    python tools/large_k_time.py [--docs 10000000] [--reps 5] [--out FILE]

k in {64 (the k <= 64 call: the baseline), 100, 1000} x B in {1, 32, 1024} over N x 256 rows kept as fp32 and as bf16
(tt_score_topk_large_f32 / _bf16 through index.score_topk), plus bench.make_clustered_corpus (near-duplicate clusters and
64-row exact tie groups: where tier 1 is expected).  Prints one JSON line per case and writes all of them to --out.
The slow tiers are timed on the random fp32 rows with query 0's answer made to need them (the constructions of
tests/test_large_k_gpu.py at full size): "tier1" = 3000 near-duplicates of its best neighbour in one block of rows (k = 1000),
"tier2" = 20 000 exact copies of the query in one block (k = 1024).
For the kernel split take a separate run under rocprofv3 --kernel-trace --stats with --reps 1."""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from twotowermlretrieval_amd import _lib, index  # noqa: E402


def _tiers(B, N, d, k, dtype, Q, D):
    """One large call with its own workspace; the per-query tiers from tt_score_topk_large_tier_offset."""
    L = _lib.lib()
    bf = int(dtype == torch.bfloat16)
    ws = torch.empty(index._exact_route(dtype, k, False).workspace_bytes(B, N, d, k, dtype), dtype=torch.uint8, device=Q.device)
    index.score_topk(Q, D, k, workspace=ws)
    torch.cuda.synchronize()
    if k <= index.SMALL_KMAX:
        return [B, 0, 0]
    o = L.tt_score_topk_large_tier_offset(B, N, d, k, bf)
    t = ws[o:o + 4 * B].view(torch.int32).cpu().numpy()
    return np.bincount(t, minlength=3).tolist()


def time_case(name, Q, D, k, reps):
    B, d = Q.shape
    N = D.shape[0]
    ws = torch.empty(index._exact_route(D.dtype, k, False).workspace_bytes(B, N, d, k, D.dtype), dtype=torch.uint8, device=Q.device)
    index.score_topk(Q, D, k, workspace=ws)  # warm-up (code objects, allocator)
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        index.score_topk(Q, D, k, workspace=ws)
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    row = {"case": name, "dtype": str(D.dtype).replace("torch.", ""), "B": B, "N": N, "d": d, "k": k,
           "ms_median": round(float(np.median(ms)), 3), "ms_min": round(float(np.min(ms)), 3),
           "tiers_0_1_2": _tiers(B, N, d, k, D.dtype, Q, D)}
    print(json.dumps(row), flush=True)
    return row


def forced(D, q, kind):
    """A copy of D in which query q's top-k needs the rescan (tier1) or the histogram refinement (tier2)."""
    D = D.clone()
    lo = D.shape[0] // 2
    if kind == "tier2":
        D[lo:lo + 20_000] = q
        return D
    j = int(torch.argmax(D @ q))
    g = torch.Generator(device=D.device).manual_seed(23)
    R = torch.randn((3000, D.shape[1]), device=D.device, generator=g)
    for u in (q, D[j].clone()):
        un = u / u.norm()
        R -= torch.outer(R @ un, un)
    R /= R.norm(dim=1, keepdim=True)
    eps = 1e-3 + 2e-2 * torch.arange(3000, device=D.device, dtype=torch.float32) / 3000
    blk = D[j][None, :] + eps[:, None] * R
    D[lo:lo + 3000] = blk / blk.norm(dim=1, keepdim=True)
    return D


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batches", default="1,32,1024")
    ap.add_argument("--ks", default="64,100,1000")
    ap.add_argument("--clustered-docs", type=int, default=2_000_000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    rows = []
    D32 = torch.randn((a.docs, 256), device=dev, generator=g)
    D32 /= D32.norm(dim=1, keepdim=True)
    Qall = torch.randn((1024, 256), device=dev, generator=g)
    Qall /= Qall.norm(dim=1, keepdim=True)
    Bs = [int(x) for x in a.batches.split(",")]
    ks = [int(x) for x in a.ks.split(",")]
    for D in (D32, D32.to(torch.bfloat16)):
        for B in Bs:
            for k in ks:
                rows.append(time_case("random", Qall[:B].contiguous(), D, k, a.reps))
    del D
    for kind, k in (("tier1", 1000), ("tier2", 1024)):
        Df = forced(D32, Qall[0], kind)
        for B in Bs:
            rows.append(time_case(kind, Qall[:B].contiguous(), Df, 64, a.reps))   # the same corpus at k = 64: the baseline
            rows.append(time_case(kind, Qall[:B].contiguous(), Df, k, a.reps))
        del Df
        torch.cuda.empty_cache()
    del D32
    torch.cuda.empty_cache()
    import bench
    Dc, Qc, _ = bench.make_clustered_corpus(a.clustered_docs, 1024, dev)
    for B in Bs:
        for k in ks:
            rows.append(time_case("clustered", Qc[:B].contiguous(), Dc.contiguous(), k, a.reps))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(rows, indent=1))


if __name__ == "__main__":
    main()
