"""Tagged sharded search with two ranks on the REAL kernels (gloo, both processes on cuda:0, like
tests/test_masked_multirank_gpu.py).  The tenants are split unevenly across the shards and one lies wholly in rank 0's: rank 1
has no eligible document for its queries and still enters the same collectives -- tagged search involves no seed exchange,
so nothing about it is a rank-local decision.  Both ranks must return the expected value of the whole corpus.  submit() is
not involved."""
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
import tagged_ref
from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

N, D_, B, K = 140_000, 256, 40, 10
STEP_TIMEOUT = 60       # seconds: a collective one rank never enters fails instead of hanging
JOB_TIMEOUT = 240


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _corpus():
    D = synth.unit_rows(51, N, D_).copy()
    Q = synth.unit_rows(52, B, D_).copy()
    n = np.arange(N)
    # tenant 0: rows below 30 000 only (all in rank 0's shard [0, 70 000)); tenant 1: 3/4 of rank 0's remaining rows and 1/4 of
    # rank 1's; tenant 2: the rest
    tags = np.where(n < 30_000, 0, np.where(n < 70_000, np.where(n % 4 < 3, 1, 2), np.where(n % 4 < 1, 1, 2))).astype(np.int32)
    mv = (np.arange(B) % 3).astype(np.int32)
    D[100 + np.arange(B)] = Q                 # query q's best document overall: tenant 0, eligible for q % 3 == 0 only
    D[100_000] = Q[1]                         # tenant 1's copy of query 1's best, in rank 1's shard (100 000 % 4 == 0)
    return D, Q, tags, mv


def _worker(rank, world, port, tmp):
    sys.path[:0] = [str(ROOT), str(GOLDEN)]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=STEP_TIMEOUT))
    torch.cuda.set_device(0)
    import twotowermlretrieval_amd as tt
    dev = torch.device("cuda", 0)
    D, Q, tags, mv = _corpus()
    lo, hi = tt.shard_bounds(N, rank, world)
    ix = tt.ShardedIndex(torch.from_numpy(D[lo:hi]).to(dev), lo, shard_k=50, screen=True)
    assert ix.tags is None
    ix.set_tags(torch.from_numpy(tags[lo:hi]).to(dev))
    assert ix.tags is not None
    Qd = torch.from_numpy(Q).to(dev)
    v, i = ix.tagged_search(Qd, K, 0xFFFFFFFF, torch.from_numpy(mv).to(dev))
    v1, i1 = ix.tagged_search(Qd[1], K, 0xFFFFFFFF, 1)
    torch.cuda.synchronize()
    assert torch.equal(i1, i[1]) and torch.equal(v1, v[1])
    np.savez(os.path.join(tmp, f"rank{rank}.npz"), v=v.cpu().numpy(), i=i.cpu().numpy())
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_tagged_sharded_search(oracle, tmp_path):
    ctx = mp.spawn(_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=False)
    deadline = time.monotonic() + JOB_TIMEOUT
    while not ctx.join(timeout=5):
        if time.monotonic() > deadline:
            for p in ctx.processes:
                p.kill()
            pytest.fail("a rank hung in the tagged sharded search")
    ranks = [np.load(tmp_path / f"rank{r}.npz") for r in range(2)]
    D, Q, tags, mv = _corpus()
    assert tags[:70_000].tolist().count(0) == 30_000 and not (tags[70_000:] == 0).any()   # tenant 0: rank 0's shard only
    elig = tagged_ref.eligibility(tags, 0xFFFFFFFF, mv)
    ov, oi = tagged_ref.expected(oracle, Q, D, elig, K, np.arange(B))
    for r in ranks:
        assert np.array_equal(r["i"], oi) and np.array_equal(r["v"], ov)
    assert [int(x) for x in ranks[1]["i"][::3, 0]] == [100 + q for q in range(0, B, 3)]   # tenant 0's queries find their rows
    assert int(ranks[0]["i"][1, 0]) == 100_000                                            # query 1: its tenant's copy, rank 1's
    assert (oi[::3] < 30_000).all()
