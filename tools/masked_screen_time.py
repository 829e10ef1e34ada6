#!/usr/bin/env python3
"""Masked SCREENED search, event timing with interleaved rounds on one build and one GPU: 10M x 256 rows (fp32 + fp16 shadow,
and bf16 rows), k = 10, B = 32 and B = 1024.
  leg "masked"             a masked search on a screen_masked=True index (all ones, random 50 %, 1 % kept) against (a) the same
                           masked search as an index WITHOUT the keyword runs it -- the masked exact route, which is what the
                           parent commit runs -- and (b) the unmasked screened search of this build (the cost of the mask).
                           The 50 % result must equal the exact route's, the all-ones result the unmasked one's.
  leg "unmasked_vs_parent" with --parent PATH (a libtt.so built from the parent commit): that library's
                           tt_score_topk_screened_f32 against this build's, same process, interleaved -- the unmasked
                           instantiations did not move.
One JSON line per measurement (times in ms: median, and min..max over the rounds); "spread" = (max - min) / median of the
baseline's own rounds.  Usage: masked_screen_time.py [docs] [--parent PATH] > profiles/masked_screen_time.log"""
import ctypes as C
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch

import bench
import twotowermlretrieval_amd as tt
from twotowermlretrieval_amd import _lib

args = sys.argv[1:]
parent = None
if "--parent" in args:
    at = args.index("--parent")
    parent = args[at + 1]
    del args[at:at + 2]
n = int(args[0]) if args else bench.N_DOCS
dev = torch.device("cuda:0")
K, ROUNDS = 10, 5


def timeit(fn, iters):
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


def spread(t):
    return round((t[2] - t[1]) / t[0], 4)


def emit(**kw):
    print(json.dumps(kw), flush=True)


def same(a, b):
    return bool(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]))


g = torch.Generator(device=dev).manual_seed(0)
masks = {"ones": torch.ones(n, dtype=torch.bool, device=dev),
         "half": torch.rand(n, device=dev, generator=g) < 0.5,
         "one_percent": torch.rand(n, device=dev, generator=g) < 0.01}
keeps = {name: tt.pack_keep_mask(m) for name, m in masks.items()}
docs32 = bench.gen_rows(0, n, dev)
shadow = None
for dtype in (torch.float32, torch.bfloat16):
    docs = docs32 if dtype == torch.float32 else docs32.to(torch.bfloat16)
    ixm = tt.BruteForceIndex(docs, screen=True, screen_masked=True)
    ix0 = tt.BruteForceIndex(docs, screen=ixm._screen)          # the same layout without the keyword: today's routing
    if dtype == torch.float32:
        shadow = ixm._screen
    for B in (32, 1024):
        q = bench.gen_queries(B, dev, seed=B)
        assert ixm._screens(B, K, True) and not ix0._screens(B, K, True) and ix0._screens(B, K, False)
        plain = ixm.search(q, K)
        ones = ixm.search(q, K, keep=keeps["ones"])
        half = ixm.search(q, K, keep=keeps["half"])
        flags_half = int(ixm.fallback_flags.ne(0).sum())
        exact_half = ix0.search(q, K, keep=keeps["half"])
        torch.cuda.synchronize()
        fns = {"exact_half": lambda: ix0.search(q, K, keep=keeps["half"]), "unmasked": lambda: ixm.search(q, K)}
        for name, keep in keeps.items():
            fns[name] = (lambda keep: lambda: ixm.search(q, K, keep=keep))(keep)
        t = interleaved(fns, iters=3 if B > 64 else 20)
        emit(leg="masked", dtype=str(dtype).split(".")[1], B=B, docs=n, all_ones_identical=same(plain, ones),
             half_identical_to_exact=same(half, exact_half), half_flagged_tiles=flags_half,
             **{f"{name}_ms": [round(x, 4) for x in v] for name, v in t.items()},
             exact_half_spread=spread(t["exact_half"]), unmasked_spread=spread(t["unmasked"]),
             exact_half_over_screened_half=round(t["exact_half"][0] / t["half"][0], 3),
             **{f"{name}_over_unmasked": round(t[name][0] / t["unmasked"][0], 4) for name in keeps})
    del docs, ixm, ix0

if parent:
    old = C.CDLL(parent)
    name = "tt_score_topk_screened_f32"
    getattr(old, name).restype, getattr(old, name).argtypes = _lib.SIGNATURES[name]
    new = _lib.lib()
    st = torch.cuda.current_stream().cuda_stream
    for B in (32, 1024):
        q = bench.gen_queries(B, dev, seed=B)
        ws = torch.empty(new.tt_score_topk_screened_workspace_bytes(B, n, 256, K), dtype=torch.uint8, device=dev)
        outs = {}

        def call(lib, tag):
            v, i, f = outs.setdefault(tag, (torch.empty((B, K), device=dev), torch.empty((B, K), dtype=torch.int64, device=dev),
                                            torch.empty((B + 31) // 32, dtype=torch.int32, device=dev)))
            _lib.check(getattr(lib, name)(q.data_ptr(), B, 256, shadow.rows.data_ptr(), shadow.filt.data_ptr(), n, K,
                                          shadow.dmax_norm, 0, v.data_ptr(), i.data_ptr(), f.data_ptr(), ws.data_ptr(),
                                          ws.numel(), None, st))

        t = interleaved({"parent": lambda: call(old, "parent"), "this": lambda: call(new, "this")}, iters=3 if B > 64 else 20)
        torch.cuda.synchronize()
        emit(leg="unmasked_vs_parent", B=B, docs=n, identical=all(bool(torch.equal(a, b)) for a, b in zip(outs["parent"], outs["this"])),
             parent_ms=[round(x, 4) for x in t["parent"]], this_ms=[round(x, 4) for x in t["this"]],
             parent_spread=spread(t["parent"]), this_over_parent=round(t["this"][0] / t["parent"][0], 4))
