"""Collapsed search on the sharded index, two ranks on the REAL kernels (gloo, both processes on cuda:0, like
tests/test_mmr_multirank_gpu.py).  Every rank runs the sharded search, fills in the group ids of the result ids it owns, one
all_reduce(SUM) completes them, and every rank runs the filter.  Both ranks must return what one BruteForceIndex over the
whole corpus returns, which is the contract over the oracle's scores -- with a query whose head one page owns (1 100 rows over
both shards), so that the continuation rounds, the masked one included, run as collectives."""
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

import collapse_ref
from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

N = 4096
CASES = ((10, 1, True, 0), (10, 3, True, 0), (10, 1, False, 0), (10, 2, True, 5), (70, 1, True, 0))   # (k, m, exact, E)
STEP_TIMEOUT = 60       # seconds: a collective one rank never enters fails instead of hanging
JOB_TIMEOUT = 240


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _exclude(S, E):
    """Every query's own best E rows."""
    return np.ascontiguousarray(np.argsort(-S, axis=1, kind="stable")[:, :E], dtype=np.int64)


def _worker(rank, world, port, tmp):
    sys.path[:0] = [str(ROOT), str(GOLDEN)]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=STEP_TIMEOUT))
    torch.cuda.set_device(0)
    import twotowermlretrieval_amd as tt
    dev = torch.device("cuda", 0)
    D, Q, g, _ = collapse_ref.planted(N)
    S = np.load(os.path.join(tmp, "scores.npy"))
    lo, hi = tt.shard_bounds(N, rank, world)
    ix = tt.ShardedIndex(torch.from_numpy(D[lo:hi]).to(dev), lo, shard_k=50)
    ix.set_groups(torch.from_numpy(g[lo:hi]).to(dev))
    Qd = torch.from_numpy(Q).to(dev)
    res = {}
    for n, (k, m, exact, E) in enumerate(CASES):
        ex = torch.from_numpy(_exclude(S, E)).to(dev) if E else None
        out = ix.collapsed_search(Qd, k, m, exclude=ex, exact=exact)
        torch.cuda.synchronize()
        for name, t in zip("vigc", out):
            res[f"{name}{n}"] = t.cpu().numpy()
        res[f"r{n}"] = np.array(ix.collapse_rounds)
    one = ix.collapsed_search(Qd[0], 10, 1)                                    # one query [d], the one that needs the rounds
    torch.cuda.synchronize()
    assert np.array_equal(one[1].cpu().numpy(), res["i0"][0]) and np.array_equal(one[2].cpu().numpy(), res["g0"][0])
    np.savez(os.path.join(tmp, f"rank{rank}.npz"), **res)
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_sharded_collapsed_search(oracle, tmp_path):
    import twotowermlretrieval_amd as tt
    D, Q, g, where = collapse_ref.planted(N)
    S = oracle.score_all(Q, D)
    np.save(tmp_path / "scores.npy", S)
    assert (where < N // 2).any() and (where >= N // 2).any()                  # the page straddles the shards
    ctx = mp.spawn(_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=False)
    deadline = time.monotonic() + JOB_TIMEOUT
    while not ctx.join(timeout=5):
        if time.monotonic() > deadline:
            for p in ctx.processes:
                p.kill()
            pytest.fail("a rank hung in the sharded collapsed search")
    ranks = [np.load(tmp_path / f"rank{r}.npz") for r in range(2)]

    one = tt.BruteForceIndex(torch.from_numpy(D).cuda())                       # one index over the whole corpus
    one.set_groups(torch.from_numpy(g).cuda())
    Qd = torch.from_numpy(Q).cuda()
    for n, (k, m, exact, E) in enumerate(CASES):
        ex = _exclude(S, E)
        el = np.ones(S.shape, bool)
        np.put_along_axis(el, ex, False, axis=1)
        wv, wi, wg = collapse_ref.search(S, g, k, m, el)
        got = one.collapsed_search(Qd, k, m, exclude=torch.from_numpy(ex).cuda() if E else None, exact=exact)
        torch.cuda.synchronize()
        sv, si, sg, sc = (t.cpu().numpy() for t in got)
        for r in ranks:
            assert np.array_equal(r[f"i{n}"], si) and np.array_equal(r[f"v{n}"], sv) and np.array_equal(r[f"g{n}"], sg), n
            assert np.array_equal(r[f"c{n}"], sc), n
        if exact:
            assert np.array_equal(si, wi) and np.array_equal(sv, wv) and np.array_equal(sg, wg) and (sc == 1).all(), n
            for r in ranks:                                                     # query 0 went through a masked round, on both
                assert r[f"r{n}"][1] >= 1, n
        else:
            assert sc.tolist() == [0, 1, 1] and si[0, 0] == wi[0, 0] and (si[0, 1:] == -1).all()
            assert np.array_equal(si[1:], wi[1:])
