#!/usr/bin/env python3
"""What the softmax loss over a gathered pool costs, and whether making K9 rectangular cost the in-batch entry anything.
Event timing with interleaved rounds on one GPU (the method of tools/in_batch_loss_time.py).
  leg "pool"    tt_contrastive_loss_f32 at the 8-rank shape B = 512, M = 8192, H = 256, pos_offset = 3072 (unit rows,
                temperature 0.05): the full call (six launches) and the loss-only call (four); the products' FLOPs (five products
                of B x M x H: S for the statistics, S again in each gradient pass, G Dh, G^T qh) over the full call's time,
                beside the f32-input MFMA's peak (the bound of this kernel family).
  leg "parent"  tt_in_batch_loss_f32 at B = 512, H = 256 from this tree's library and from a library built from the parent
                commit (--parent-lib PATH: the same build of the parent's sources), loaded side by side in one process and
                timed alternately; first their results on the same rows are compared bit for bit.  The tree's median may exceed
                the parent's by no more than the parent's own min..max spread in this run ("within_parent_spread").
                Without --parent-lib the leg says "not measured".
Without a leg argument the tool is the driver: each leg runs as a child process of its own under its own time limit, and the
first leg that fails or runs out of time ends the run (exit status 1, nothing more is started on the GPU).
One JSON line per measurement (times in ms: median, and min..max over the rounds).
Usage: contrastive_loss_time.py [--parent-lib PATH] > profiles/contrastive_loss_time.log"""
import argparse
import ctypes as C
import json
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
LEGS = {"pool": 240, "parent": 240}   # leg -> time limit of its process, seconds
sys.path.insert(0, str(Path(__file__).resolve().parent))
from in_batch_loss_time import F32_MFMA_PEAK_TFLOPS, emit, interleaved, ms  # noqa: E402


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


def unit_rows(shape, dev, seed):
    import torch
    g = torch.Generator(device=dev).manual_seed(seed)
    return torch.nn.functional.normalize(torch.randn(shape, device=dev, generator=g), dim=1)


def leg_pool(B=512, M=8192, H=256, pos_offset=3072, temperature=0.05):
    import torch
    from twotowermlretrieval_amd import _lib
    from twotowermlretrieval_amd.model import contrastive_workspace
    dev = torch.device("cuda:0")
    L = _lib.lib()
    q, docs = unit_rows((B, H), dev, 0), unit_rows((M, H), dev, 1)
    loss = torch.empty((), dtype=torch.float32, device=dev)
    dq, ddocs = torch.empty_like(q), torch.empty_like(docs)
    ws = contrastive_workspace(B, M, H, dev)
    st = torch.cuda.current_stream(dev).cuda_stream

    def call(grads):
        g2 = (dq.data_ptr(), ddocs.data_ptr()) if grads else (None, None)
        _lib.check(L.tt_contrastive_loss_f32(q.data_ptr(), B, docs.data_ptr(), M, H, pos_offset, temperature, loss.data_ptr(), *g2,
                                             ws.data_ptr(), ws.numel(), st))
    t = interleaved({"full": lambda: call(True), "loss_only": lambda: call(False)}, iters=50)
    value = float(loss.item())
    assert value == value and abs(value) < 1e30, value
    flop = 5 * 2.0 * B * M * H
    emit(leg="pool", B=B, M=M, H=H, pos_offset=pos_offset, temperature=temperature, workspace_bytes=ws.numel(),
         contrastive_ms=ms(t["full"]), contrastive_loss_only_ms=ms(t["loss_only"]), product_flop=flop,
         product_tflops=round(flop / t["full"][0] / 1e9, 2), f32_mfma_peak_tflops=F32_MFMA_PEAK_TFLOPS,
         share_of_f32_mfma_peak=round(flop / t["full"][0] / 1e9 / F32_MFMA_PEAK_TFLOPS, 4), loss=value,
         note="back-to-back calls on one stream: launch gaps between the call's launches are inside the time; the share is the "
              "whole call's (prep, statistics and projection launches included), compute-bound side only")


def leg_parent(parent_lib, B=512, H=256, temperature=0.05):
    import torch
    from twotowermlretrieval_amd import _lib
    if not parent_lib:
        emit(leg="parent", what="not measured: no --parent-lib given")
        return
    dev = torch.device("cuda:0")
    libs = {"tree": _lib.lib(), "parent": C.CDLL(str(Path(parent_lib).resolve()))}
    for name in ("tt_in_batch_loss_workspace_bytes", "tt_in_batch_loss_f32"):
        fn = getattr(libs["parent"], name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    assert not hasattr(libs["parent"], "tt_contrastive_loss_f32"), "--parent-lib has the new entry: it is not the parent's build"
    q, p, n = (unit_rows((B, H), dev, s) for s in range(3))
    st = torch.cuda.current_stream(dev).cuda_stream
    state = {}
    for who, L in libs.items():
        need = L.tt_in_batch_loss_workspace_bytes(B, H)
        state[who] = dict(loss=torch.empty(1, device=dev), g=[torch.empty_like(q) for _ in range(3)],
                          ws=torch.empty(need, dtype=torch.uint8, device=dev))

    def call(who):
        s, L = state[who], libs[who]
        rc = L.tt_in_batch_loss_f32(q.data_ptr(), p.data_ptr(), n.data_ptr(), B, H, temperature, s["loss"].data_ptr(),
                                    *(g.data_ptr() for g in s["g"]), s["ws"].data_ptr(), s["ws"].numel(), st)
        assert rc == 0, (who, rc)
    for who in libs:
        call(who)
    torch.cuda.synchronize()
    same = all(torch.equal(a.view(torch.int32), b.view(torch.int32))
               for a, b in zip([state["tree"]["loss"]] + state["tree"]["g"], [state["parent"]["loss"]] + state["parent"]["g"]))
    t = interleaved({who: (lambda who=who: call(who)) for who in libs}, iters=50)
    over = t["tree"][0] - t["parent"][0]
    spread = t["parent"][2] - t["parent"][1]
    emit(leg="parent", what="tt_in_batch_loss_f32, full call, this tree's library against the parent commit's, alternating", B=B, H=H,
         temperature=temperature, same_bits_as_parent=same, workspace_bytes={w: s["ws"].numel() for w, s in state.items()},
         tree_ms=ms(t["tree"]), parent_ms=ms(t["parent"]), tree_minus_parent_median_ms=round(over, 5),
         parent_spread_ms=round(spread, 5), within_parent_spread=bool(over <= spread))
    assert same, "the in-batch entry's bits changed against the parent"


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("leg", nargs="?", choices=list(LEGS))
    ap.add_argument("--parent-lib", default=None)
    a = ap.parse_args()
    if a.leg is None:
        sys.exit(driver(a.parent_lib))
    sys.path.insert(0, str(ROOT))
    leg_pool() if a.leg == "pool" else leg_parent(a.parent_lib)
