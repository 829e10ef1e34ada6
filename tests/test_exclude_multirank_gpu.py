"""Per-query exclusion lists on the sharded search, two ranks on the REAL kernels (gloo, both processes on cuda:0, like
tests/test_masked_multirank_gpu.py).  Every rank passes the same lists; each query's list takes its best documents out of
BOTH shards, the local searches, the exchange and the merge run for k + E, and the filter runs once on the merged rows.  Both
ranks must return the reference idiom over the whole corpus (oracle.score_all, the listed entries -inf, sorted, first k), for
k + E below 64 (screened shards, union seed) and above (the exact large-k route, no seed exchange)."""
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

import synth
from conftest import GOLDEN, ROOT
from test_exclude_gpu import idiom, own_top
from test_search_aux_gpu import par_rows

pytestmark = pytest.mark.gpu

N, D_, B, K = 140_000, 256, 12, 10
WIDTHS = (5, 60)        # k + E = 15 and 70
STEP_TIMEOUT = 60       # seconds: a collective one rank never enters fails instead of hanging
JOB_TIMEOUT = 240


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _corpus():
    D = synth.unit_rows(61, N, D_).copy()
    Q = synth.unit_rows(62, B, D_).copy()
    D[100 + np.arange(B)] = Q                 # query q's best document is row 100 + q (rank 0's shard) ...
    D[100_000 + np.arange(B)] = Q             # ... tied with row 100 000 + q (rank 1's shard)
    return D, Q


def _worker(rank, world, port, tmp):
    sys.path[:0] = [str(ROOT), str(GOLDEN)]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=STEP_TIMEOUT))
    torch.cuda.set_device(0)
    import twotowermlretrieval_amd as tt
    dev = torch.device("cuda", 0)
    D, Q = _corpus()
    lists = np.load(os.path.join(tmp, "lists.npz"))
    lo, hi = tt.shard_bounds(N, rank, world)
    ix = tt.ShardedIndex(torch.from_numpy(D[lo:hi]).to(dev), lo, shard_k=50, screen=True)
    assert ix._seed_exchange is True                               # 70 000 rows per shard: the union seed is agreed on
    Qd = torch.from_numpy(Q).to(dev)
    res = {}
    for E in WIDTHS:
        ex = torch.from_numpy(lists[f"ex{E}"]).to(dev)
        v, i = ix.search(Qd, k=K, exclude=ex)
        pv, pi = ix.submit(Qd, k=K, exclude=ex).result()
        torch.cuda.synchronize()
        assert v.shape == (B, K) and torch.equal(pv, v) and torch.equal(pi, i), E
        res[f"v{E}"], res[f"i{E}"] = v.cpu().numpy(), i.cpu().numpy()
    pend = [ix.submit(Qd, k=K, exclude=torch.from_numpy(lists[f"ex{E}"]).to(dev)) for E in WIDTHS]   # two steps in flight
    for E, p in zip(WIDTHS, pend):
        pv, pi = p.result()
        torch.cuda.synchronize()
        assert np.array_equal(pv.cpu().numpy(), res[f"v{E}"]) and np.array_equal(pi.cpu().numpy(), res[f"i{E}"]), E
    v, i = ix.search(Qd[0], k=K, exclude=torch.from_numpy(lists[f"ex{WIDTHS[0]}"][0]).to(dev))   # one query, [E]
    torch.cuda.synchronize()
    assert np.array_equal(i.cpu().numpy(), res[f"i{WIDTHS[0]}"][0])
    np.savez(os.path.join(tmp, f"rank{rank}.npz"), **res)
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_sharded_search_with_exclusion_lists(oracle, tmp_path):
    D, Q = _corpus()
    S = par_rows(lambda q: oracle.score_all(q, D), Q)
    rs = np.random.RandomState(63)
    lists = {f"ex{E}": own_top(S, E, rs, 2) for E in WIDTHS}
    for ex in lists.values():                                      # every list takes documents out of both shards
        assert ((ex[:, :3] < 70_000).any(axis=1) & (ex[:, :3] >= 70_000).any(axis=1)).all()
    np.savez(tmp_path / "lists.npz", **lists)
    ctx = mp.spawn(_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=False)
    deadline = time.monotonic() + JOB_TIMEOUT
    while not ctx.join(timeout=5):
        if time.monotonic() > deadline:
            for p in ctx.processes:
                p.kill()
            pytest.fail("a rank hung in the sharded search with exclusion lists")
    ranks = [np.load(tmp_path / f"rank{r}.npz") for r in range(2)]
    for E in WIDTHS:
        ov, oi = idiom(S, lists[f"ex{E}"], K)
        for r in ranks:
            assert np.array_equal(r[f"i{E}"], oi) and np.array_equal(r[f"v{E}"], ov), E
        assert not np.isin(oi[:, 0], [100 + np.arange(B), 100_000 + np.arange(B)]).any()   # both planted rows are listed
