"""Masked sharded search with two ranks on the REAL kernels (gloo, both processes on cuda:0, like tests/test_multirank_gpu.py).
Whether a search is masked decides whether a rank enters the seed all-gather, so it has to be a property of the job: every
rank calls remove_ids with ids that all fall in rank 0's shard, and a rank-local decision would leave rank 1 alone in that
all-gather.  Both ranks must return the expected value of the whole masked corpus."""
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
from test_search_aux_gpu import par_rows

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
    D[100 + np.arange(B)] = Q                 # query q's best document is row 100 + q: rank 0's shard
    D[100_000] = Q[0]                         # a tie of query 0's best in rank 1's shard
    removed = np.concatenate([100 + np.arange(0, B, 2), np.random.RandomState(1).choice(70_000, 500, replace=False)])
    call = np.random.RandomState(2).rand(N) < 0.5
    return D, Q, removed, call


def _worker(rank, world, port, tmp):
    sys.path[:0] = [str(ROOT), str(GOLDEN)]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=STEP_TIMEOUT))
    torch.cuda.set_device(0)
    import twotowermlretrieval_amd as tt
    dev = torch.device("cuda", 0)
    D, Q, removed, call = _corpus()
    lo, hi = tt.shard_bounds(N, rank, world)
    ix = tt.ShardedIndex(torch.from_numpy(D[lo:hi]).to(dev), lo, shard_k=50, screen=True)
    assert ix._seed_exchange is True and ix.keep_mask is None      # 70 000 rows per shard: the union seed is agreed on
    Qd = torch.from_numpy(Q).to(dev)
    res = {}
    v, i = ix.search(Qd, k=K)
    res["v_plain"], res["i_plain"] = v.cpu().numpy(), i.cpu().numpy()
    assert removed.max() < 70_000                                  # every id falls in rank 0's shard ...
    ix.remove_ids(torch.from_numpy(removed))
    assert ix.keep_mask is not None                                # ... and rank 1 has a mask all the same
    if rank:
        ones = tt.pack_keep_mask(torch.ones(hi - lo, dtype=torch.bool, device=dev))
        assert torch.equal(ix.keep_mask, ones)                     # (every row kept: none of the ids is rank 1's)
    v, i = ix.search(Qd, k=K)
    pv, pi = ix.submit(Qd, k=K).result()
    torch.cuda.synchronize()
    assert torch.equal(pv, v) and torch.equal(pi, i)
    res["v_removed"], res["i_removed"] = v.cpu().numpy(), i.cpu().numpy()
    keep = tt.pack_keep_mask(torch.from_numpy(call[lo:hi]).to(dev))  # a per-call keep: this rank's rows, on all ranks
    v, i = ix.search(Qd, k=K, keep=keep)
    torch.cuda.synchronize()
    res["v_call"], res["i_call"] = v.cpu().numpy(), i.cpu().numpy()
    np.savez(os.path.join(tmp, f"rank{rank}.npz"), **res)
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_masked_sharded_search(oracle, tmp_path):
    ctx = mp.spawn(_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=False)
    deadline = time.monotonic() + JOB_TIMEOUT
    while not ctx.join(timeout=5):
        if time.monotonic() > deadline:
            for p in ctx.processes:
                p.kill()
            pytest.fail("a rank hung in the masked sharded search")
    ranks = [np.load(tmp_path / f"rank{r}.npz") for r in range(2)]
    D, Q, removed, call = _corpus()

    def want(mask):
        kept = np.flatnonzero(mask)
        Dk = np.ascontiguousarray(D[kept])
        v, i = par_rows(lambda q: oracle.score_topk(q, Dk, K), Q)
        return v, np.where(i >= 0, kept[np.maximum(i, 0)], -1)

    mask = np.ones(N, dtype=bool)
    for name, m in (("plain", mask), ("removed", None), ("call", None)):
        if name == "removed":
            mask[removed] = False
            m = mask
        elif name == "call":
            m = mask & call
        ov, oi = want(m)
        for r in ranks:
            assert np.array_equal(r[f"i_{name}"], oi) and np.array_equal(r[f"v_{name}"], ov), name
    assert ranks[0]["i_plain"][0, :2].tolist() == [100, 100_000]
    assert ranks[0]["i_removed"][0, 0] == 100_000                   # row 100 is gone, its tie in the other shard is not
    assert not np.isin(ranks[1]["i_removed"], removed).any()
