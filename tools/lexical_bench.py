#!/usr/bin/env python3
"""Lexical search timing on one GPU: LexicalIndex.search at B = 1 over a synthetic Zipf corpus in CSR (about 50 entries per row,
F = 20 000 columns, unit-norm rows), next to the host's way of getting the same rows (sklearn cosine_similarity + argsort over
all N, what hybrid.py's default path runs), in the same process on the same matrix.

  leg "search"      k in {10, 50}.  search_ms: LexicalIndex.search(q, k) as hybrid.py calls it, q the scipy row the vectorizer
                    returns (host clock around calls that end in a synchronise: conversion, three small uploads, the launches).
                    device_ms: the same search with the query already on the device (lexical_score_topk, device events; median,
                    min..max over the rounds), the bytes one pass has to read, nnz * 8 + (N + 1) * 8, and GB/s against the
                    measured copy rate of the MI355X (6.29 TB/s).  Leg "score_all" is the scoring pass alone (no selection, no
                    merge; it writes N floats), so the difference is what selection and the merges cost.
  leg "host"        cosine_similarity(q, matrix) + stable argsort on the host, with the core count; whether its top-k rows are
                    the GPU's (the scores differ in the last bits: f32 chain vs float64 cosine, so near-ties may swap; the
                    largest score difference over the returned rows is printed).
One JSON line per measurement.  Usage: lexical_bench.py [--gpu-only] [docs ...] > profiles/lexical_time.log   (default: 1000000
10000000; --gpu-only leaves the host leg out, for a run under rocprofv3 --kernel-trace --stats)"""
import json
import os
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np
import torch

F, MEAN_LEN, COPY_RATE_GBPS, ROUNDS = 20000, 50, 6290.0, 7


def emit(**kw):
    print(json.dumps(kw), flush=True)


def zipf_cols(shape, gen, device):
    """Columns with a Zipf-like skew: floor(F * u^3) puts half of the draws into the first eighth of the vocabulary."""
    u = torch.rand(shape, generator=gen, device=device)
    return (u * u * u * F).to(torch.int32).clamp_(max=F - 1)


def zipf_csr(n, seed, device, block=1 << 20):
    """(indptr int64 [n+1], cols int32, vals f32): rows of 30..70 draws, sorted, duplicates dropped, values uniform in
    (0.2, 1) and the row L2-normalised in fp32, generated on `device` in blocks of rows."""
    gen = torch.Generator(device=device).manual_seed(seed)
    lens_all, cols_all, vals_all = [], [], []
    lmax = MEAN_LEN + 20
    for r0 in range(0, n, block):
        m = min(block, n - r0)
        want = torch.randint(MEAN_LEN - 20, lmax + 1, (m, 1), generator=gen, device=device)
        c = zipf_cols((m, lmax), gen, device)
        c = torch.where(torch.arange(lmax, device=device)[None, :] < want, c, torch.full_like(c, F))   # padding sorts last
        c = c.sort(dim=1).values
        live = c < F
        live[:, 1:] &= c[:, 1:] != c[:, :-1]
        v = torch.rand((m, lmax), generator=gen, device=device) * 0.8 + 0.2
        v = torch.where(live, v, torch.zeros_like(v))
        v = v / v.square().sum(dim=1, keepdim=True).sqrt().clamp_(min=1e-30)
        lens_all.append(live.sum(dim=1))
        cols_all.append(c[live])
        vals_all.append(v[live])
    indptr = torch.zeros(n + 1, dtype=torch.int64, device=device)
    torch.cumsum(torch.cat(lens_all), 0, out=indptr[1:])
    return indptr, torch.cat(cols_all).contiguous(), torch.cat(vals_all).to(torch.float32).contiguous()


def zipf_query(terms, seed, device):
    gen = torch.Generator(device=device).manual_seed(seed)
    c = torch.unique(zipf_cols((terms,), gen, device))
    v = torch.rand(c.shape, generator=gen, device=device) * 0.8 + 0.2
    v = v / v.square().sum().sqrt()
    return torch.tensor([0, c.numel()], dtype=torch.int64, device=device), c.to(torch.int32), v.to(torch.float32)


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


def rounds(fn, iters):
    t = sorted(timeit(fn, iters) for _ in range(ROUNDS))
    return [round(x, 4) for x in (t[len(t) // 2], t[0], t[-1])]


def main(sizes, host=True):
    import scipy.sparse as sp
    from sklearn.metrics.pairwise import cosine_similarity
    import twotowermlretrieval_amd as tt
    if not torch.cuda.is_available():
        raise SystemExit("lexical_bench.py measures on a GPU: none found")
    dev = torch.device("cuda:0")
    cores = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else os.cpu_count()
    emit(leg="setup", device=torch.cuda.get_device_name(0), F=F, host_cores_usable=cores, host_cores_total=os.cpu_count(),
         threads_env=os.environ.get("OMP_NUM_THREADS"), copy_rate_GBps=COPY_RATE_GBPS)
    for n in sizes:
        indptr, cols, vals = zipf_csr(n, 1, dev)
        nnz = cols.numel()
        ix = tt.LexicalIndex.__new__(tt.LexicalIndex)   # the generator's rows are valid by construction: no host round trip
        ix.indptr, ix.cols, ix.vals, ix._n_features, ix.idx_offset, ix._keep = indptr, cols, vals, F, 0, None
        q = zipf_query(8, 2, dev)
        pass_bytes = nnz * 8 + (n + 1) * 8
        corpus = (indptr, cols, vals)
        S = tt.lexical_score_all(corpus, F, q)
        torch.cuda.synchronize()
        matched = float((S > 1e-5).float().mean())
        del S
        iters = 20 if n <= 2_000_000 else 5
        t_all = rounds(lambda: tt.lexical_score_all(corpus, F, q), iters)
        emit(leg="score_all", docs=n, nnz=nnz, query_terms=int(q[1].numel()), docs_above_1e_5=round(matched, 3),
             ms=t_all, pass_bytes=pass_bytes, GBps=round(pass_bytes / t_all[0] / 1e6, 1),
             share_of_copy_rate=round(pass_bytes / t_all[0] / 1e6 / COPY_RATE_GBPS, 3))
        res = {}
        qm = sp.csr_matrix((q[2].cpu().numpy(), q[1].cpu().numpy(), q[0].cpu().numpy()), shape=(1, F))
        for k in (10, 50):
            t = rounds(lambda: tt.lexical_score_topk(corpus, F, q, k), iters)
            v, i = ix.search(qm, k)
            torch.cuda.synchronize()
            res[k] = (v[0].cpu().numpy(), i[0].cpu().numpy())
            t0 = time.perf_counter()
            for _ in range(iters):
                ix.search(qm, k)
            torch.cuda.synchronize()
            emit(leg="search", docs=n, nnz=nnz, B=1, k=k, search_ms=round((time.perf_counter() - t0) * 1e3 / iters, 4),
                 device_ms=t, pass_bytes=pass_bytes, GBps=round(pass_bytes / t[0] / 1e6, 1),
                 share_of_copy_rate=round(pass_bytes / t[0] / 1e6 / COPY_RATE_GBPS, 3),
                 selection_and_merge_ms=round(t[0] - t_all[0], 4))
        if not host:
            continue
        # the parent's way, on this machine's host, on the same matrix
        mat = sp.csr_matrix((vals.cpu().numpy(), cols.cpu().numpy(), indptr.cpu().numpy()), shape=(n, F))
        reps = 3 if n <= 2_000_000 else 1
        for k in (10, 50):
            ts = []
            for _ in range(reps):
                t0 = time.perf_counter()
                sims = cosine_similarity(qm, mat).flatten()
                order = np.argsort(-sims, kind="stable")[:k]
                ts.append((time.perf_counter() - t0) * 1e3)
            gv, gi = res[k]
            emit(leg="host", docs=n, k=k, what="sklearn cosine_similarity + stable argsort over N", host_cores_usable=cores,
                 ms=[round(x, 1) for x in (sorted(ts)[len(ts) // 2], min(ts), max(ts))], repeats=reps,
                 same_rows_as_gpu=bool(np.array_equal(order, gi)),
                 max_abs_score_difference=float(np.abs(sims[gi[gi >= 0]] - gv[gi >= 0]).max()))
        del mat, ix, indptr, cols, vals
        torch.cuda.empty_cache()


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "--gpu-only"]
    main([int(a) for a in args] or [1_000_000, 10_000_000], host="--gpu-only" not in sys.argv)
