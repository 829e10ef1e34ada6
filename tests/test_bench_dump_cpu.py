"""bench.py's output dump (--dump-outputs DIR) and its argument checks, on the host: the files a comparison of two builds
reads, their dtypes and their values; a step count below one is refused before any device is touched; the legs beyond the
headline figure run only when --full asks for them."""
import subprocess
import sys

import numpy as np
import torch

from conftest import ROOT


def test_dump_outputs_writes_what_the_caller_receives(tmp_path):
    import bench
    g = torch.Generator().manual_seed(0)
    vals = torch.sort(torch.rand((bench.BATCH, bench.TOPK), generator=g), dim=1, descending=True).values
    idx = torch.randint(0, bench.N_DOCS, (bench.BATCH, bench.TOPK), generator=g, dtype=torch.int64)
    idx[0, 0] = bench.N_DOCS - 1
    names = bench.dump_outputs(tmp_path / "out", vals, idx)
    assert names == ["topk_indices", "topk_scores"]
    s, i = np.load(tmp_path / "out" / "topk_scores.npy"), np.load(tmp_path / "out" / "topk_indices.npy")
    assert s.dtype == np.float32 and i.dtype == np.float64
    assert np.array_equal(s, vals.numpy()) and np.array_equal(i.astype(np.int64), idx.numpy())
    assert sum(p.stat().st_size for p in (tmp_path / "out").iterdir()) <= 64 << 20


def test_bench_refuses_zero_steps():
    for args in (["--steps", "0"], ["--warmup", "-1"]):
        r = subprocess.run([sys.executable, str(ROOT / "bench.py"), *args], capture_output=True, text=True, timeout=120)
        assert r.returncode == 2 and "--steps must be >= 1" in r.stderr, (args, r.returncode, r.stderr[-500:])


def test_legs_beyond_the_headline_need_full():
    import bench
    assert not bench.parse_args(["--gpus", "1", "--steps", "5", "--warmup", "2"]).full
    assert bench.parse_args(["--full", "--no-cpu-baseline"]).full
