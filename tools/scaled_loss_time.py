#!/usr/bin/env python3
"""What reading the temperature from device memory -- and returning its gradient -- costs the softmax loss over a pool, and
whether adding it cost the existing entries anything.  Event timing with interleaved rounds on one GPU (the method and helpers of
tools/sym_loss_time.py), at the 8-rank shape B = 512, M = 8192, H = 256, pos_offset = 3072 (unit rows, temperature 0.05), with
gradients.
  leg "scaled"   tt_contrastive_loss_ls_f32 and tt_contrastive_loss_sym_ls_f32 (alpha = 0.5), with d_log_scale and without,
                 from this tree's library against tt_contrastive_loss_f32 from a library built from the parent commit
                 (--parent-lib PATH: the same build of the parent's sources; the parent has tt_contrastive_loss_sym_f32 too, and
                 the symmetric pair is timed against that), loaded side by side in one process and timed alternately.  First the
                 parent entries, called at the temperature read back from temperature_out, must write the new entries' bits.
                 What the new entries add is one scalar load per launch, one [B] write and one one-block sum.  The ratios are
                 reported, not gated, beside the parent entries' own min..max spread in the run.
  leg "parent"   the plain, grouped, soft and symmetric float entries from this tree's library and from the parent's,
                 alternating; first their results on the same rows are compared bit for bit.  The time difference is reported
                 against the parent's own min..max spread in this run.
Without --parent-lib both legs say "not measured".  Without a leg argument the tool is the driver: each leg runs as a child
process of its own under its own time limit, and the first leg that fails or runs out of time ends the run (exit status 1,
nothing more is started on the GPU).
One JSON line per measurement (times in ms: median, and min..max over the 7 rounds).
Usage: scaled_loss_time.py [--parent-lib PATH] > profiles/scaled_loss_time.log"""
import argparse
import ctypes as C
import math
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
LEGS = {"scaled": 240, "parent": 240}   # leg -> time limit of its process, seconds
sys.path.insert(0, str(Path(__file__).resolve().parent))
from contrastive_loss_time import unit_rows  # noqa: E402
from grouped_loss_time import Buffers  # noqa: E402
from in_batch_loss_time import emit, interleaved, ms  # noqa: E402
from soft_loss_time import same_bits  # noqa: E402
from sym_loss_time import labels  # noqa: E402

SHAPE = dict(B=512, M=8192, H=256, pos_offset=3072, temperature=0.05)
ENTRY, GROUPED, SOFT = "tt_contrastive_loss_f32", "tt_contrastive_loss_grouped_f32", "tt_contrastive_loss_soft_f32"
SYM = "tt_contrastive_loss_sym_f32"
LS, SYM_LS = "tt_contrastive_loss_ls_f32", "tt_contrastive_loss_sym_ls_f32"
OLD = ("tt_contrastive_loss_workspace_bytes", "tt_contrastive_loss_soft_workspace_bytes", "tt_contrastive_loss_sym_workspace_bytes",
       ENTRY, GROUPED, SOFT, SYM)
LO, HI = 0.0, math.log(100.0)


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


def parent_library(path):
    from twotowermlretrieval_amd import _lib
    lib = C.CDLL(str(Path(path).resolve()))
    for name in OLD:
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    assert not hasattr(lib, LS), "--parent-lib has the new entry: it is not the parent's build"
    return lib


def leg_scaled(parent_lib, B, M, H, pos_offset, temperature):
    import torch
    from twotowermlretrieval_amd import _lib
    if not parent_lib:
        emit(leg="scaled", what="not measured: no --parent-lib given")
        return
    dev = torch.device("cuda:0")
    L, P = _lib.lib(), parent_library(parent_lib)
    q, docs = unit_rows((B, H), dev, 0), unit_rows((M, H), dev, 1)
    need = {"ls": L.tt_contrastive_loss_ls_workspace_bytes(B, M, H, 0), "sym_ls": L.tt_contrastive_loss_sym_ls_workspace_bytes(B, M, H),
            "parent": P.tt_contrastive_loss_workspace_bytes(B, M, H), "parent_sym": P.tt_contrastive_loss_sym_workspace_bytes(B, M, H)}
    bufs = {who: Buffers(n, q, docs) for who, n in need.items()}
    word = torch.tensor([-math.log(temperature)], dtype=torch.float32, device=dev)
    t_out, dl = torch.empty(1, dtype=torch.float32, device=dev), torch.empty(2, dtype=torch.float32, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream

    def ls(with_dl=True):
        b = bufs["ls"]
        _lib.check(L.tt_contrastive_loss_ls_f32(q.data_ptr(), B, docs.data_ptr(), M, H, pos_offset, None, None, None, word.data_ptr(),
                                                LO, HI, b.loss.data_ptr(), t_out.data_ptr(), dl[0:1].data_ptr() if with_dl else None,
                                                b.dq.data_ptr(), b.ddocs.data_ptr(), b.ws.data_ptr(), need["ls"], st))

    def sym_ls(with_dl=True):
        b = bufs["sym_ls"]
        _lib.check(L.tt_contrastive_loss_sym_ls_f32(q.data_ptr(), B, docs.data_ptr(), M, H, pos_offset, None, None, word.data_ptr(),
                                                    LO, HI, 0.5, b.loss.data_ptr(), None, t_out.data_ptr(),
                                                    dl[1:2].data_ptr() if with_dl else None, b.dq.data_ptr(), b.ddocs.data_ptr(),
                                                    b.ws.data_ptr(), need["sym_ls"], st))
    ls()
    sym_ls()
    torch.cuda.synchronize()
    T = float(t_out.item())

    def parent():
        b = bufs["parent"]
        rc = P.tt_contrastive_loss_f32(q.data_ptr(), B, docs.data_ptr(), M, H, pos_offset, T, b.loss.data_ptr(), b.dq.data_ptr(),
                                       b.ddocs.data_ptr(), b.ws.data_ptr(), need["parent"], st)
        assert rc == 0, rc

    def parent_sym():
        b = bufs["parent_sym"]
        rc = P.tt_contrastive_loss_sym_f32(q.data_ptr(), B, docs.data_ptr(), M, H, pos_offset, None, None, T, 0.5, b.loss.data_ptr(),
                                           None, b.dq.data_ptr(), b.ddocs.data_ptr(), b.ws.data_ptr(), need["parent_sym"], st)
        assert rc == 0, rc
    parent()
    parent_sym()
    torch.cuda.synchronize()
    same = {"ls": same_bits(bufs["ls"].results(), bufs["parent"].results()),
            "sym_ls": same_bits(bufs["sym_ls"].results(), bufs["parent_sym"].results())}
    values = dict(T=T, d_log_scale=float(dl[0].item()), d_log_scale_sym=float(dl[1].item()), loss=float(bufs["ls"].loss.item()))
    assert all(v == v and abs(v) < 1e30 for v in values.values()), values
    t = interleaved({"ls": ls, "parent": parent, "sym_ls": sym_ls, "parent_sym": parent_sym,
                     "ls_no_dl": lambda: ls(False), "sym_ls_no_dl": lambda: sym_ls(False)}, iters=50)
    for new, old, entry, against in (("ls", "parent", LS, ENTRY), ("sym_ls", "parent_sym", SYM_LS, SYM)):
        spread = t[old][2] - t[old][1]
        emit(leg="scaled", what=f"{entry} (with d_log_scale) of this tree against {against} of the parent commit's library, "
             "alternating", B=B, M=M, H=H, pos_offset=pos_offset, temperature=T, workspace_bytes={new: need[new], old: need[old]},
             new_ms=ms(t[new]), parent_ms=ms(t[old]), new_without_d_log_scale_ms=ms(t[new + "_no_dl"]),
             new_over_parent=round(t[new][0] / t[old][0], 4),
             new_without_d_log_scale_over_parent=round(t[new + "_no_dl"][0] / t[old][0], 4),
             new_minus_parent_median_ms=round(t[new][0] - t[old][0], 5), parent_spread_ms=round(spread, 5),
             parent_spread_over_median=round(spread / t[old][0], 4), same_bits_as_parent_at_T=same[new], values=values,
             note="the ratio is reported, not gated")
    assert all(same.values()), f"the parent entry at the temperature read back did not reproduce the new entry's bits: {same}"


def leg_parent(parent_lib, B, M, H, pos_offset, temperature):
    import torch
    from twotowermlretrieval_amd import _lib
    if not parent_lib:
        emit(leg="parent", what="not measured: no --parent-lib given")
        return
    dev = torch.device("cuda:0")
    libs = {"tree": _lib.lib(), "parent": parent_library(parent_lib)}
    q, docs = unit_rows((B, H), dev, 0), unit_rows((M, H), dev, 1)
    qg, dg = labels(B, M, pos_offset, dev)
    g = torch.Generator(device=dev).manual_seed(2)
    dense = torch.softmax(3.0 * torch.randn((B, M), device=dev, generator=g), dim=1).contiguous()
    st = torch.cuda.current_stream(dev).cuda_stream
    size = {ENTRY: "tt_contrastive_loss_workspace_bytes", GROUPED: "tt_contrastive_loss_workspace_bytes",
            SOFT: "tt_contrastive_loss_soft_workspace_bytes", SYM: "tt_contrastive_loss_sym_workspace_bytes"}
    state = {(who, e): Buffers(getattr(lib, size[e])(B, M, H), q, docs) for who, lib in libs.items() for e in size}

    def call(who, entry):
        b = state[(who, entry)]
        grads = (b.dq.data_ptr(), b.ddocs.data_ptr(), b.ws.data_ptr(), b.ws.numel(), st)
        fn, head = getattr(libs[who], entry), (q.data_ptr(), B, docs.data_ptr(), M, H)
        if entry == SOFT:
            rc = fn(*head, dense.data_ptr(), temperature, b.loss.data_ptr(), *grads)
        elif entry == SYM:
            rc = fn(*head, pos_offset, qg.data_ptr(), dg.data_ptr(), temperature, 0.5, b.loss.data_ptr(), None, *grads)
        else:
            lab = (qg.data_ptr(), dg.data_ptr()) if entry == GROUPED else ()
            rc = fn(*head, pos_offset, *lab, temperature, b.loss.data_ptr(), *grads)
        assert rc == 0, (who, entry, rc)
    for key in state:
        call(*key)
    torch.cuda.synchronize()
    same = {e: same_bits(state[("tree", e)].results(), state[("parent", e)].results()) for e in size}
    t = interleaved({f"{who}:{e}": (lambda who=who, e=e: call(who, e)) for who, e in state}, iters=50)
    for e in size:
        tree, parent = t[f"tree:{e}"], t[f"parent:{e}"]
        over, spread = tree[0] - parent[0], parent[2] - parent[1]
        emit(leg="parent", what=f"{e}, full call, this tree's library against the parent commit's, alternating", B=B, M=M, H=H,
             pos_offset=pos_offset, temperature=temperature, same_bits_as_parent=same[e],
             workspace_bytes={w: state[(w, e)].ws.numel() for w in libs}, tree_ms=ms(tree), parent_ms=ms(parent),
             tree_over_parent=round(tree[0] / parent[0], 4), tree_minus_parent_median_ms=round(over, 5),
             parent_spread_ms=round(spread, 5), within_parent_spread=bool(over <= spread))
    assert all(same.values()), f"an existing entry's bits changed against the parent: {same}"


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("leg", nargs="?", choices=list(LEGS))
    ap.add_argument("--parent-lib", default=None)
    a = ap.parse_args()
    if a.leg is None:
        sys.exit(driver(a.parent_lib))
    sys.path.insert(0, str(ROOT))
    (leg_scaled if a.leg == "scaled" else leg_parent)(a.parent_lib, **SHAPE)
