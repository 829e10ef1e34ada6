#!/usr/bin/env python3
"""What group labels cost the softmax loss over a pool, and whether templating K9 on them cost the ungrouped entry anything.
Event timing with interleaved rounds on one GPU (the method and helpers of tools/contrastive_loss_time.py).
  leg "grouped"  tt_contrastive_loss_grouped_f32 against tt_contrastive_loss_f32 from the same library at the 8-rank shape
                 B = 512, M = 8192, H = 256, pos_offset = 3072 (unit rows, temperature 0.05), full call and loss-only call,
                 alternating.  Groups of 4 consecutive queries share a label and their positives carry it; every other row
                 has no group.  The ratio grouped / ungrouped is reported, not gated; it is set beside the ungrouped
                 entry's own min..max spread in the run.
  leg "parent"   tt_contrastive_loss_f32 at the same shape from this tree's library and from a library built from the parent
                 commit (--parent-lib PATH: the same build of the parent's sources), loaded side by side in one process and
                 timed alternately; first their results on the same rows are compared bit for bit.  The tree's median may exceed
                 the parent's by no more than the parent's own min..max spread in this run ("within_parent_spread").
                 Without --parent-lib the leg says "not measured".
Without a leg argument the tool is the driver: each leg runs as a child process of its own under its own time limit, and the
first leg that fails or runs out of time ends the run (exit status 1, nothing more is started on the GPU).
One JSON line per measurement (times in ms: median, and min..max over the rounds).
Usage: grouped_loss_time.py [--parent-lib PATH] > profiles/grouped_loss_time.log"""
import argparse
import ctypes as C
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
LEGS = {"grouped": 240, "parent": 240}   # leg -> time limit of its process, seconds
sys.path.insert(0, str(Path(__file__).resolve().parent))
from contrastive_loss_time import unit_rows  # noqa: E402
from in_batch_loss_time import emit, interleaved, ms  # noqa: E402

SHAPE = dict(B=512, M=8192, H=256, pos_offset=3072, temperature=0.05)
ENTRY, GROUPED = "tt_contrastive_loss_f32", "tt_contrastive_loss_grouped_f32"


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


class Buffers:
    """Outputs and workspace of one caller at SHAPE (the inputs are shared)."""

    def __init__(self, need, q, docs):
        import torch
        self.loss = torch.empty(1, dtype=torch.float32, device=q.device)
        self.dq, self.ddocs = torch.empty_like(q), torch.empty_like(docs)
        self.ws = torch.empty(need, dtype=torch.uint8, device=q.device)

    def results(self):
        return [self.loss, self.dq, self.ddocs]


def leg_grouped(B, M, H, pos_offset, temperature):
    import torch
    from twotowermlretrieval_amd import _lib
    dev = torch.device("cuda:0")
    L = _lib.lib()
    q, docs = unit_rows((B, H), dev, 0), unit_rows((M, H), dev, 1)
    qg = (torch.arange(B, device=dev) // 4).to(torch.int64)
    dg = torch.full((M,), -1, dtype=torch.int64, device=dev)
    dg[pos_offset:pos_offset + B] = qg
    need = L.tt_contrastive_loss_workspace_bytes(B, M, H)
    bufs = {"grouped": Buffers(need, q, docs), "ungrouped": Buffers(need, q, docs)}
    st = torch.cuda.current_stream(dev).cuda_stream

    def call(who, grads):
        b = bufs[who]
        g2 = (b.dq.data_ptr(), b.ddocs.data_ptr()) if grads else (None, None)
        if who == "grouped":
            rc = L.tt_contrastive_loss_grouped_f32(q.data_ptr(), B, docs.data_ptr(), M, H, pos_offset, qg.data_ptr(), dg.data_ptr(),
                                                   temperature, b.loss.data_ptr(), *g2, b.ws.data_ptr(), need, st)
        else:
            rc = L.tt_contrastive_loss_f32(q.data_ptr(), B, docs.data_ptr(), M, H, pos_offset, temperature, b.loss.data_ptr(), *g2,
                                           b.ws.data_ptr(), need, st)
        _lib.check(rc)
    t = interleaved({f"{who}_{kind}": (lambda who=who, grads=grads: call(who, grads))
                     for who in bufs for kind, grads in (("full", True), ("loss_only", False))}, iters=50)
    values = {who: float(b.loss.item()) for who, b in bufs.items()}
    assert all(v == v and abs(v) < 1e30 for v in values.values()) and values["grouped"] < values["ungrouped"], values
    spread = t["ungrouped_full"][2] - t["ungrouped_full"][1]
    over = t["grouped_full"][0] - t["ungrouped_full"][0]
    emit(leg="grouped", what=f"{GROUPED} against {ENTRY}, the same library, alternating; groups of 4 queries share a label",
         B=B, M=M, H=H, pos_offset=pos_offset, temperature=temperature, workspace_bytes=need,
         grouped_ms=ms(t["grouped_full"]), ungrouped_ms=ms(t["ungrouped_full"]),
         grouped_loss_only_ms=ms(t["grouped_loss_only"]), ungrouped_loss_only_ms=ms(t["ungrouped_loss_only"]),
         grouped_over_ungrouped=round(t["grouped_full"][0] / t["ungrouped_full"][0], 4),
         grouped_over_ungrouped_loss_only=round(t["grouped_loss_only"][0] / t["ungrouped_loss_only"][0], 4),
         grouped_minus_ungrouped_median_ms=round(over, 5), ungrouped_spread_ms=round(spread, 5),
         within_ungrouped_spread=bool(over <= spread), loss=values, note="the ratio is reported, not gated")


def leg_parent(parent_lib, B, M, H, pos_offset, temperature):
    import torch
    from twotowermlretrieval_amd import _lib
    if not parent_lib:
        emit(leg="parent", what="not measured: no --parent-lib given")
        return
    dev = torch.device("cuda:0")
    libs = {"tree": _lib.lib(), "parent": C.CDLL(str(Path(parent_lib).resolve()))}
    for name in ("tt_contrastive_loss_workspace_bytes", ENTRY):
        fn = getattr(libs["parent"], name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    assert not hasattr(libs["parent"], GROUPED), "--parent-lib has the new entry: it is not the parent's build"
    q, docs = unit_rows((B, H), dev, 0), unit_rows((M, H), dev, 1)
    st = torch.cuda.current_stream(dev).cuda_stream
    state = {who: Buffers(L.tt_contrastive_loss_workspace_bytes(B, M, H), q, docs) for who, L in libs.items()}

    def call(who):
        b = state[who]
        rc = getattr(libs[who], ENTRY)(q.data_ptr(), B, docs.data_ptr(), M, H, pos_offset, temperature, b.loss.data_ptr(),
                                       b.dq.data_ptr(), b.ddocs.data_ptr(), b.ws.data_ptr(), b.ws.numel(), st)
        assert rc == 0, (who, rc)
    for who in libs:
        call(who)
    torch.cuda.synchronize()
    same = all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(state["tree"].results(), state["parent"].results()))
    t = interleaved({who: (lambda who=who: call(who)) for who in libs}, iters=50)
    over = t["tree"][0] - t["parent"][0]
    spread = t["parent"][2] - t["parent"][1]
    emit(leg="parent", what=f"{ENTRY}, full call, this tree's library against the parent commit's, alternating", B=B, M=M, H=H,
         pos_offset=pos_offset, temperature=temperature, same_bits_as_parent=same,
         workspace_bytes={w: s.ws.numel() for w, s in state.items()}, tree_ms=ms(t["tree"]), parent_ms=ms(t["parent"]),
         tree_minus_parent_median_ms=round(over, 5), parent_spread_ms=round(spread, 5), within_parent_spread=bool(over <= spread))
    assert same, "the ungrouped entry's bits changed against the parent"


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("leg", nargs="?", choices=list(LEGS))
    ap.add_argument("--parent-lib", default=None)
    a = ap.parse_args()
    if a.leg is None:
        sys.exit(driver(a.parent_lib))
    sys.path.insert(0, str(ROOT))
    leg_grouped(**SHAPE) if a.leg == "grouped" else leg_parent(a.parent_lib, **SHAPE)
