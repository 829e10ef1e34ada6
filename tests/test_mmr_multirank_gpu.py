"""Diversified search on the sharded index, two ranks on the REAL kernels (gloo, both processes on cuda:0, like
tests/test_score_ids_multirank_gpu.py).  Every rank runs the sharded search for fetch_k, fills a [B,fetch_k,d] block with the
rows of the candidates it owns, one all_reduce(SUM) completes the blocks, and every rank selects from them.  Both ranks must
return what one BruteForceIndex over the whole corpus returns, which is the reference's selection from the oracle's top
fetch_k -- with candidates that straddle the shards and a tie across them."""
import datetime
import os
import socket
import sys
import time

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import mmr_ref
import synth
from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

N, D_, B = 20_000, 256, 12
CASES = ((10, 0.5, None), (10, 0.3, 64), (40, 0.7, 128), (3, 0.0, 3))   # (k, lambda, fetch_k)
STEP_TIMEOUT = 60       # seconds: a collective one rank never enters fails instead of hanging
JOB_TIMEOUT = 240


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _corpus():
    D = synth.unit_rows(91, N, D_).copy()
    Q = synth.unit_rows(92, B, D_).copy()
    D[100 + np.arange(B)] = Q                 # query q's best document is row 100 + q (rank 0's shard) ...
    D[15_000 + np.arange(B)] = Q              # ... tied with its twin, row 15 000 + q (rank 1's shard)
    return D, Q


def _worker(rank, world, port, tmp):
    sys.path[:0] = [str(ROOT), str(GOLDEN)]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=STEP_TIMEOUT))
    torch.cuda.set_device(0)
    import twotowermlretrieval_amd as tt
    dev = torch.device("cuda", 0)
    D, Q = _corpus()
    lo, hi = tt.shard_bounds(N, rank, world)
    ix = tt.ShardedIndex(torch.from_numpy(D[lo:hi]).to(dev), lo, shard_k=50)
    Qd = torch.from_numpy(Q).to(dev)
    res = {}
    for n, (k, lam, fk) in enumerate(CASES):
        v, i = ix.diverse_search(Qd, k, lam, fetch_k=fk)
        torch.cuda.synchronize()
        res[f"v{n}"], res[f"i{n}"] = v.cpu().numpy(), i.cpu().numpy()
    v1, i1 = ix.diverse_search(Qd[2], 10, 0.5)                             # one query [d]
    torch.cuda.synchronize()
    assert np.array_equal(i1.cpu().numpy(), res["i0"][2]) and np.array_equal(v1.cpu().numpy(), res["v0"][2])
    np.savez(os.path.join(tmp, f"rank{rank}.npz"), **res)
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_sharded_diverse_search(oracle, tmp_path):
    import twotowermlretrieval_amd as tt
    D, Q = _corpus()
    ctx = mp.spawn(_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=False)
    deadline = time.monotonic() + JOB_TIMEOUT
    while not ctx.join(timeout=5):
        if time.monotonic() > deadline:
            for p in ctx.processes:
                p.kill()
            pytest.fail("a rank hung in the sharded diverse search")
    ranks = [np.load(tmp_path / f"rank{r}.npz") for r in range(2)]

    one = tt.BruteForceIndex(torch.from_numpy(D).cuda())                   # one index over the whole corpus
    Qd = torch.from_numpy(Q).cuda()
    for n, (k, lam, fk) in enumerate(CASES):
        fetch = min(128, 4 * k) if fk is None else fk
        tv, ti = oracle.score_topk(Q, D, fetch)
        assert ((ti < 10_000).any(1) & (ti >= 10_000).any(1)).all()        # the candidates straddle the shards
        assert np.array_equal(ti[:, 0], 100 + np.arange(B)) and np.array_equal(ti[:, 1], 15_000 + np.arange(B))   # the tie
        want_v, want_i, _ = mmr_ref.select(oracle, tv, ti, D, k, lam)
        v, i = one.diverse_search(Qd, k, lam, fetch_k=fk)
        assert np.array_equal(i.cpu().numpy(), want_i) and np.array_equal(v.cpu().numpy(), want_v), n
        for r in ranks:
            assert np.array_equal(r[f"i{n}"], want_i) and np.array_equal(r[f"v{n}"], want_v), n
        if lam == 0.3:   # the twin across the shards is demoted by its similarity (|q|^2 = 1), by the rule alone
            assert (want_i[:, 1] != 15_000 + np.arange(B)).all() and (want_i[:, 0] == 100 + np.arange(B)).all()
        if lam == 0.5:   # the query IS document 0 of its list: lambda r - mu <x_c, q> = 0 for every c, a tie the position breaks
            assert (want_i[:, 1] == 15_000 + np.arange(B)).all()
