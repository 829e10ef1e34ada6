#!/usr/bin/env python3
"""What the in-batch softmax loss costs, event timing with interleaved rounds on one build and one GPU.
  leg "kernel"  tt_in_batch_loss_f32 alone at B = 512, H = 256 (unit rows, temperature 0.05): the full call (six launches), the
                loss-only call (four), and tt_triplet_loss_f32 (K6) on the same rows; the products' FLOPs (five products of
                B x 2B x H: S for the statistics, S again in each gradient pass, G Dh, G^T qh) over the call's time, beside
                the f32-input MFMA's peak (the bound of this kernel family).
  leg "step"    the graphed train step of the bench (north-star model, 512 triplets, bench.make_encoder_inputs) with
                negatives="paired" and with negatives="in_batch", alternating in the same process: ms per step each, and the
                added time per step beside the kernel-alone difference (in-batch call minus K6) from a run of leg "kernel"
                inside the same process.
Without an argument the tool is the driver: each leg runs as a child process of its own under its own time limit, and the
first leg that fails or runs out of time ends the run (exit status 1, nothing more is started on the GPU).
One JSON line per measurement (times in ms: median, and min..max over the rounds).
Usage: in_batch_loss_time.py > profiles/in_batch_loss_time.log"""
import json
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
LEGS = {"kernel": 240, "step": 420}   # leg -> time limit of its process, seconds
ROUNDS = 7
F32_MFMA_PEAK_TFLOPS = 157.3          # 256 CUs x 4 SIMDs x 64 FLOP/clk x 2.4 GHz (f32-input MFMA = the f32 vector rate)


def emit(**kw):
    print(json.dumps(kw), flush=True)


def ms(t, nd=5):
    return [round(x, nd) for x in t]


def driver():
    for leg, limit in LEGS.items():
        try:
            r = subprocess.run([sys.executable, str(Path(__file__).resolve()), leg], timeout=limit)
            rc = r.returncode
        except subprocess.TimeoutExpired:
            rc = 124
        if rc != 0:
            emit(leg="FAILED", what=f"leg {leg}: exit status {rc}" + (f" (time limit {limit} s)" if rc == 124 else ""))
            print(f"FAILED: leg {leg} (exit status {rc}); nothing more is run", file=sys.stderr, flush=True)
            return 1
    return 0


def timeit(fn, iters):
    import torch
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def interleaved(fns, iters, rounds=ROUNDS):
    """rounds x (every fn in turn): per fn (median, min, max) in ms."""
    ts = {name: [] for name in fns}
    for _ in range(rounds):
        for name, fn in fns.items():
            ts[name].append(timeit(fn, iters))
    return {name: (sorted(t)[len(t) // 2], min(t), max(t)) for name, t in ts.items()}


def kernel_calls(B, H, temperature=0.05):
    """{name: launch closure} for the in-batch call (with and without gradients) and K6 on the same unit rows."""
    import torch
    from twotowermlretrieval_amd import _lib
    from twotowermlretrieval_amd.model import in_batch_workspace
    dev = torch.device("cuda:0")
    L = _lib.lib()
    g = torch.Generator(device=dev).manual_seed(0)
    q, p, n = (torch.nn.functional.normalize(torch.randn((B, H), device=dev, generator=g), dim=1) for _ in range(3))
    loss = torch.empty((), dtype=torch.float32, device=dev)
    dq, dp, dn = (torch.empty_like(q) for _ in range(3))
    rows = torch.empty(B, dtype=torch.float32, device=dev)
    ws = in_batch_workspace(B, H, dev)
    st = torch.cuda.current_stream(dev).cuda_stream

    def in_batch(grads=True):
        g3 = (dq.data_ptr(), dp.data_ptr(), dn.data_ptr()) if grads else (None, None, None)
        _lib.check(L.tt_in_batch_loss_f32(q.data_ptr(), p.data_ptr(), n.data_ptr(), B, H, temperature, loss.data_ptr(), *g3,
                                          ws.data_ptr(), ws.numel(), st))

    def triplet():
        _lib.check(L.tt_triplet_loss_f32(q.data_ptr(), p.data_ptr(), n.data_ptr(), B, H, 0.5, loss.data_ptr(), dq.data_ptr(),
                                         dp.data_ptr(), dn.data_ptr(), rows.data_ptr(), st))
    keep = (q, p, n, loss, dq, dp, dn, rows, ws)
    return {"in_batch": lambda: in_batch(True), "in_batch_loss_only": lambda: in_batch(False), "triplet_k6": triplet}, keep


def leg_kernel(B=512, H=256):
    import torch
    fns, keep = kernel_calls(B, H)
    t = interleaved(fns, iters=50)
    loss = float(keep[3].item())
    assert loss == loss and abs(loss) < 1e30, loss
    flop = 5 * 2.0 * B * (2 * B) * H
    emit(leg="kernel", B=B, H=H, temperature=0.05, in_batch_ms=ms(t["in_batch"]), in_batch_loss_only_ms=ms(t["in_batch_loss_only"]),
         triplet_k6_ms=ms(t["triplet_k6"]), in_batch_minus_k6_ms=round(t["in_batch"][0] - t["triplet_k6"][0], 5),
         product_flop=flop, product_tflops=round(flop / t["in_batch"][0] / 1e9, 2), f32_mfma_peak_tflops=F32_MFMA_PEAK_TFLOPS,
         share_of_f32_mfma_peak=round(flop / t["in_batch"][0] / 1e9 / F32_MFMA_PEAK_TFLOPS, 4),
         note="back-to-back calls on one stream: launch gaps between the call's launches are inside the time")
    del keep
    return t


def leg_step():
    import copy
    import torch
    sys.path.insert(0, str(ROOT))
    import bench
    import twotowermlretrieval_amd as tt
    dev = torch.device("cuda:0")
    inp = bench.make_encoder_inputs(dev, with_index_batch=False)
    B = inp["B"]
    qd, pd, nd = inp["q"].to(dev), inp["p"].to(dev), inp["n"].to(dev)
    r32 = lambda x: (int(x) + 31) // 32 * 32  # noqa: E731
    steps = {}
    for kind in ("paired", "in_batch"):
        m = copy.deepcopy(inp["model"]).train()
        opt = tt.FusedClipAdam(m.parameters(), lr=5e-5, max_norm=1.0)
        steps[kind] = tt.GraphedTrainStep(m, opt, batch=B, q_width=r32(qd.shape[1]), doc_width=r32(max(pd.shape[1], nd.shape[1])),
                                          margin=0.5, defer_check=True, negatives=kind, temperature=0.05)
    bench._settle_gc()
    t = interleaved({kind: (lambda s=s: s(qd, pd, nd)) for kind, s in steps.items()}, iters=20)
    for s in steps.values():
        s.flush()
    losses = {kind: float(s.loss.item()) for kind, s in steps.items()}
    k = interleaved(kernel_calls(B, bench.ENC_H)[0], iters=50)
    added = t["in_batch"][0] - t["paired"][0]
    alone = k["in_batch"][0] - k["triplet_k6"][0]
    emit(leg="step", what="graphed train step, deferred check, 512 triplets, north-star model", B=B, H=bench.ENC_H,
         q_width=steps["paired"].q_width, doc_width=steps["paired"].doc_width, paired_ms=ms(t["paired"]), in_batch_ms=ms(t["in_batch"]),
         added_ms_per_step=round(added, 5), added_share_of_paired_step=round(added / t["paired"][0], 4),
         kernel_alone_in_batch_ms=ms(k["in_batch"]), kernel_alone_triplet_k6_ms=ms(k["triplet_k6"]),
         kernel_alone_difference_ms=round(alone, 5), added_minus_kernel_difference_ms=round(added - alone, 5), last_losses=losses)


if __name__ == "__main__":
    if len(sys.argv) < 2:
        sys.exit(driver())
    sys.path.insert(0, str(ROOT))
    {"kernel": leg_kernel, "step": leg_step}[sys.argv[1]]()
