#!/usr/bin/env python3
"""What soft targets cost the softmax loss over a pool, and whether the SOFT template argument cost the existing entries anything.
Event timing with interleaved rounds on one GPU (the method and helpers of tools/grouped_loss_time.py).
  leg "soft"     tt_contrastive_loss_soft_f32 with dense targets (softmax(3 randn) per row, [B, M] f32: 16.8 MB) against
                 tt_contrastive_loss_f32 from the same library at the 8-rank shape B = 512, M = 8192, H = 256, pos_offset =
                 3072 (unit rows, temperature 0.05), full call and loss-only call, alternating.  Also the soft entry on one-hot
                 targets, whose bits must be the plain entry's.  The ratio soft / plain is reported, not gated; it is set beside
                 the plain entry's own min..max spread in the run.
  leg "parent"   tt_contrastive_loss_f32 and tt_contrastive_loss_grouped_f32 at the same shape from this tree's library and from
                 a library built from the parent commit (--parent-lib PATH: the same build of the parent's sources), loaded side
                 by side in one process and timed alternately; first their results on the same rows are compared bit for bit.
                 The time difference is reported against the parent's own min..max spread in this run.
                 Without --parent-lib the leg says "not measured".
Without a leg argument the tool is the driver: each leg runs as a child process of its own under its own time limit, and the
first leg that fails or runs out of time ends the run (exit status 1, nothing more is started on the GPU).
One JSON line per measurement (times in ms: median, and min..max over the 7 rounds).
Usage: soft_loss_time.py [--parent-lib PATH] > profiles/soft_loss_time.log"""
import argparse
import ctypes as C
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
LEGS = {"soft": 240, "parent": 240}   # leg -> time limit of its process, seconds
sys.path.insert(0, str(Path(__file__).resolve().parent))
from contrastive_loss_time import unit_rows  # noqa: E402
from grouped_loss_time import Buffers  # noqa: E402
from in_batch_loss_time import emit, interleaved, ms  # noqa: E402

SHAPE = dict(B=512, M=8192, H=256, pos_offset=3072, temperature=0.05)
ENTRY, GROUPED, SOFT = "tt_contrastive_loss_f32", "tt_contrastive_loss_grouped_f32", "tt_contrastive_loss_soft_f32"


def driver(parent_lib):
    for leg, limit in LEGS.items():
        cmd = [sys.executable, str(Path(__file__).resolve()), leg] + (["--parent-lib", parent_lib] if parent_lib else [])
        try:
            rc = subprocess.run(cmd, timeout=limit).returncode
        except subprocess.TimeoutExpired:
            rc = 124
        if rc != 0:
            emit(leg="FAILED", what=f"leg {leg}: exit status {rc}" + (f" (time limit {limit} s)" if rc == 124 else ""))
            print(f"FAILED: leg {leg} (exit status {rc}); nothing more is run", file=sys.stderr, flush=True)
            return 1
    return 0


def same_bits(xs, ys):
    import torch
    return all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(xs, ys))


def leg_soft(B, M, H, pos_offset, temperature):
    import torch
    from twotowermlretrieval_amd import _lib
    dev = torch.device("cuda:0")
    L = _lib.lib()
    q, docs = unit_rows((B, H), dev, 0), unit_rows((M, H), dev, 1)
    g = torch.Generator(device=dev).manual_seed(2)
    dense = torch.softmax(3.0 * torch.randn((B, M), device=dev, generator=g), dim=1).contiguous()
    one_hot = torch.zeros((B, M), dtype=torch.float32, device=dev)
    one_hot[torch.arange(B, device=dev), pos_offset + torch.arange(B, device=dev)] = 1.0
    need = {"soft": L.tt_contrastive_loss_soft_workspace_bytes(B, M, H), "plain": L.tt_contrastive_loss_workspace_bytes(B, M, H)}
    bufs = {who: Buffers(n, q, docs) for who, n in need.items()}
    st = torch.cuda.current_stream(dev).cuda_stream

    def call(who, grads, targets=dense):
        b = bufs[who]
        g2 = (b.dq.data_ptr(), b.ddocs.data_ptr()) if grads else (None, None)
        if who == "soft":
            rc = L.tt_contrastive_loss_soft_f32(q.data_ptr(), B, docs.data_ptr(), M, H, targets.data_ptr(), temperature,
                                                b.loss.data_ptr(), *g2, b.ws.data_ptr(), need[who], st)
        else:
            rc = L.tt_contrastive_loss_f32(q.data_ptr(), B, docs.data_ptr(), M, H, pos_offset, temperature, b.loss.data_ptr(), *g2,
                                           b.ws.data_ptr(), need[who], st)
        _lib.check(rc)
    call("soft", True, one_hot)
    call("plain", True)
    torch.cuda.synchronize()
    same = same_bits(bufs["soft"].results(), bufs["plain"].results())
    fns = {f"{who}_{kind}": (lambda who=who, grads=grads: call(who, grads))
           for who in bufs for kind, grads in (("full", True), ("loss_only", False))}
    fns["soft_one_hot_full"] = lambda: call("soft", True, one_hot)
    t = interleaved(fns, iters=50)
    call("soft", True)
    values = {who: float(b.loss.item()) for who, b in bufs.items()}
    assert all(v == v and abs(v) < 1e30 for v in values.values()), values
    spread = t["plain_full"][2] - t["plain_full"][1]
    over = t["soft_full"][0] - t["plain_full"][0]
    emit(leg="soft", what=f"{SOFT} (dense targets) against {ENTRY}, the same library, alternating", B=B, M=M, H=H,
         pos_offset=pos_offset, temperature=temperature, workspace_bytes=need, target_bytes=dense.numel() * 4,
         soft_ms=ms(t["soft_full"]), plain_ms=ms(t["plain_full"]), soft_one_hot_ms=ms(t["soft_one_hot_full"]),
         soft_loss_only_ms=ms(t["soft_loss_only"]), plain_loss_only_ms=ms(t["plain_loss_only"]),
         soft_over_plain=round(t["soft_full"][0] / t["plain_full"][0], 4),
         soft_over_plain_loss_only=round(t["soft_loss_only"][0] / t["plain_loss_only"][0], 4),
         soft_minus_plain_median_ms=round(over, 5),
         soft_minus_plain_loss_only_median_ms=round(t["soft_loss_only"][0] - t["plain_loss_only"][0], 5),
         plain_spread_ms=round(spread, 5), one_hot_same_bits_as_plain=same, loss=values, note="the ratio is reported, not gated")
    assert same, "one-hot targets did not reproduce the plain entry's bits"


def leg_parent(parent_lib, B, M, H, pos_offset, temperature):
    import torch
    from twotowermlretrieval_amd import _lib
    if not parent_lib:
        emit(leg="parent", what="not measured: no --parent-lib given")
        return
    dev = torch.device("cuda:0")
    libs = {"tree": _lib.lib(), "parent": C.CDLL(str(Path(parent_lib).resolve()))}
    for name in ("tt_contrastive_loss_workspace_bytes", ENTRY, GROUPED):
        fn = getattr(libs["parent"], name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    assert not hasattr(libs["parent"], SOFT), "--parent-lib has the new entry: it is not the parent's build"
    q, docs = unit_rows((B, H), dev, 0), unit_rows((M, H), dev, 1)
    qg = (torch.arange(B, device=dev) // 4).to(torch.int64)
    dg = torch.full((M,), -1, dtype=torch.int64, device=dev)
    dg[pos_offset:pos_offset + B] = qg
    st = torch.cuda.current_stream(dev).cuda_stream
    state = {(who, e): Buffers(L.tt_contrastive_loss_workspace_bytes(B, M, H), q, docs) for who, L in libs.items() for e in (ENTRY, GROUPED)}

    def call(who, entry):
        b = state[(who, entry)]
        labels = (qg.data_ptr(), dg.data_ptr()) if entry == GROUPED else ()
        rc = getattr(libs[who], entry)(q.data_ptr(), B, docs.data_ptr(), M, H, pos_offset, *labels, temperature, b.loss.data_ptr(),
                                       b.dq.data_ptr(), b.ddocs.data_ptr(), b.ws.data_ptr(), b.ws.numel(), st)
        assert rc == 0, (who, entry, rc)
    for key in state:
        call(*key)
    torch.cuda.synchronize()
    same = {e: same_bits(state[("tree", e)].results(), state[("parent", e)].results()) for e in (ENTRY, GROUPED)}
    t = interleaved({f"{who}:{e}": (lambda who=who, e=e: call(who, e)) for who, e in state}, iters=50)
    for e in (ENTRY, GROUPED):
        tree, parent = t[f"tree:{e}"], t[f"parent:{e}"]
        over, spread = tree[0] - parent[0], parent[2] - parent[1]
        emit(leg="parent", what=f"{e}, full call, this tree's library against the parent commit's, alternating", B=B, M=M, H=H,
             pos_offset=pos_offset, temperature=temperature, same_bits_as_parent=same[e],
             workspace_bytes={w: state[(w, e)].ws.numel() for w in libs}, tree_ms=ms(tree), parent_ms=ms(parent),
             tree_minus_parent_median_ms=round(over, 5), parent_spread_ms=round(spread, 5), within_parent_spread=bool(over <= spread))
    assert all(same.values()), f"an existing entry's bits changed against the parent: {same}"


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("leg", nargs="?", choices=list(LEGS))
    ap.add_argument("--parent-lib", default=None)
    a = ap.parse_args()
    if a.leg is None:
        sys.exit(driver(a.parent_lib))
    sys.path.insert(0, str(ROOT))
    leg_soft(**SHAPE) if a.leg == "soft" else leg_parent(a.parent_lib, **SHAPE)
