#!/usr/bin/env python3
"""What the document-to-query direction costs the softmax loss over a pool, and whether adding it cost the existing entries
anything.  Event timing with interleaved rounds on one GPU (the method and helpers of tools/grouped_loss_time.py), at the
8-rank shape B = 512, M = 8192, H = 256, pos_offset = 3072 (unit rows, temperature 0.05), with gradients.
  leg "sym"      tt_contrastive_loss_sym_f32 (alpha = 0.5, with loss_dirs; also loss-only, and with labels) from this tree's
                 library against tt_contrastive_loss_f32 from a library built from the parent commit (--parent-lib PATH: the
                 same build of the parent's sources), loaded side by side in one process and timed alternately.  At alpha = 0
                 the symmetric call's loss and gradients must be the parent entry's bits.  The arithmetic the direction adds
                 is B / M = 1/16 more score work in the statistics pass, one more expf per pair in 512 of 8192 columns in the
                 gradient pass, and two more one-block sums; the products are unchanged.  The ratio is reported, not gated,
                 beside the parent entry's own min..max spread in the run.
  leg "parent"   the plain, grouped and soft entries from this tree's library and from the parent's, alternating; first
                 their results on the same rows are compared bit for bit.  The time difference is reported against the
                 parent's own min..max spread in this run.
Without --parent-lib both legs say "not measured".  Without a leg argument the tool is the driver: each leg runs as a child
process of its own under its own time limit, and the first leg that fails or runs out of time ends the run (exit status 1,
nothing more is started on the GPU).
One JSON line per measurement (times in ms: median, and min..max over the 7 rounds).
Usage: sym_loss_time.py [--parent-lib PATH] > profiles/sym_loss_time.log"""
import argparse
import ctypes as C
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
LEGS = {"sym": 240, "parent": 240}   # leg -> time limit of its process, seconds
sys.path.insert(0, str(Path(__file__).resolve().parent))
from contrastive_loss_time import unit_rows  # noqa: E402
from grouped_loss_time import Buffers  # noqa: E402
from in_batch_loss_time import emit, interleaved, ms  # noqa: E402
from soft_loss_time import same_bits  # noqa: E402

SHAPE = dict(B=512, M=8192, H=256, pos_offset=3072, temperature=0.05)
ENTRY, GROUPED, SOFT = "tt_contrastive_loss_f32", "tt_contrastive_loss_grouped_f32", "tt_contrastive_loss_soft_f32"
SYM = "tt_contrastive_loss_sym_f32"
OLD = ("tt_contrastive_loss_workspace_bytes", "tt_contrastive_loss_soft_workspace_bytes", ENTRY, GROUPED, SOFT)


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
    assert not hasattr(lib, SYM), "--parent-lib has the new entry: it is not the parent's build"
    return lib


def labels(B, M, pos_offset, dev):
    import torch
    qg = (torch.arange(B, device=dev) // 4).to(torch.int64)
    dg = torch.full((M,), -1, dtype=torch.int64, device=dev)
    dg[pos_offset:pos_offset + B] = qg
    return qg, dg


def leg_sym(parent_lib, B, M, H, pos_offset, temperature):
    import torch
    from twotowermlretrieval_amd import _lib
    if not parent_lib:
        emit(leg="sym", what="not measured: no --parent-lib given")
        return
    dev = torch.device("cuda:0")
    L, P = _lib.lib(), parent_library(parent_lib)
    q, docs = unit_rows((B, H), dev, 0), unit_rows((M, H), dev, 1)
    qg, dg = labels(B, M, pos_offset, dev)
    need = {"sym": L.tt_contrastive_loss_sym_workspace_bytes(B, M, H), "parent": P.tt_contrastive_loss_workspace_bytes(B, M, H)}
    bufs = {who: Buffers(n, q, docs) for who, n in need.items()}
    dirs = torch.empty(2, dtype=torch.float32, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream

    def sym(alpha=0.5, grads=True, grouped=False):
        b = bufs["sym"]
        g2 = (b.dq.data_ptr(), b.ddocs.data_ptr()) if grads else (None, None)
        lab = (qg.data_ptr(), dg.data_ptr()) if grouped else (None, None)
        _lib.check(L.tt_contrastive_loss_sym_f32(q.data_ptr(), B, docs.data_ptr(), M, H, pos_offset, *lab, temperature, alpha,
                                                 b.loss.data_ptr(), dirs.data_ptr(), *g2, b.ws.data_ptr(), need["sym"], st))

    def parent(grads=True):
        b = bufs["parent"]
        g2 = (b.dq.data_ptr(), b.ddocs.data_ptr()) if grads else (None, None)
        rc = P.tt_contrastive_loss_f32(q.data_ptr(), B, docs.data_ptr(), M, H, pos_offset, temperature, b.loss.data_ptr(), *g2,
                                       b.ws.data_ptr(), need["parent"], st)
        assert rc == 0, rc
    sym(alpha=0.0)
    parent()
    torch.cuda.synchronize()
    same = same_bits(bufs["sym"].results(), bufs["parent"].results())
    t = interleaved({"sym_full": sym, "parent_full": parent, "sym_loss_only": lambda: sym(grads=False),
                     "parent_loss_only": lambda: parent(grads=False), "sym_grouped_full": lambda: sym(grouped=True)}, iters=50)
    sym()
    values = dict(loss=float(bufs["sym"].loss.item()), L_qd=float(dirs[0].item()), L_dq=float(dirs[1].item()))
    assert all(v == v and abs(v) < 1e30 for v in values.values()), values
    spread = t["parent_full"][2] - t["parent_full"][1]
    emit(leg="sym", what=f"{SYM} (alpha = 0.5, loss_dirs) of this tree against {ENTRY} of the parent commit's library, alternating",
         B=B, M=M, H=H, pos_offset=pos_offset, temperature=temperature, workspace_bytes=need, sym_ms=ms(t["sym_full"]),
         parent_ms=ms(t["parent_full"]), sym_grouped_ms=ms(t["sym_grouped_full"]), sym_loss_only_ms=ms(t["sym_loss_only"]),
         parent_loss_only_ms=ms(t["parent_loss_only"]), sym_over_parent=round(t["sym_full"][0] / t["parent_full"][0], 4),
         sym_over_parent_loss_only=round(t["sym_loss_only"][0] / t["parent_loss_only"][0], 4),
         sym_minus_parent_median_ms=round(t["sym_full"][0] - t["parent_full"][0], 5),
         sym_minus_parent_loss_only_median_ms=round(t["sym_loss_only"][0] - t["parent_loss_only"][0], 5),
         parent_spread_ms=round(spread, 5), alpha_0_same_bits_as_parent=same, values=values,
         note="the ratio is reported, not gated")
    assert same, "alpha = 0 did not reproduce the parent entry's bits"


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
            SOFT: "tt_contrastive_loss_soft_workspace_bytes"}
    state = {(who, e): Buffers(getattr(L, size[e])(B, M, H), q, docs) for who, L in libs.items() for e in size}

    def call(who, entry):
        b = state[(who, entry)]
        tail = (temperature, b.loss.data_ptr(), b.dq.data_ptr(), b.ddocs.data_ptr(), b.ws.data_ptr(), b.ws.numel(), st)
        if entry == SOFT:
            rc = getattr(libs[who], entry)(q.data_ptr(), B, docs.data_ptr(), M, H, dense.data_ptr(), *tail)
        else:
            lab = (qg.data_ptr(), dg.data_ptr()) if entry == GROUPED else ()
            rc = getattr(libs[who], entry)(q.data_ptr(), B, docs.data_ptr(), M, H, pos_offset, *lab, *tail)
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
    (leg_sym if a.leg == "sym" else leg_parent)(a.parent_lib, **SHAPE)
