"""The library calls behind the index classes' public methods, recorded (tests/test_index_call_trace_gpu.py).

`tracing()` replaces `_lib.lib` with a proxy around the real library for the length of a block: every call of a name in
`_lib.SIGNATURES` is recorded as [name, args] and forwarded unchanged.  Arguments are recorded by their declared C type:
c_int / c_int64 / c_float by value, a pointer as "null" or "ptr", c_size_t as "size" (workspace sizes depend on the device's
CU count).  ctypes makes c_uint64 the same class as c_size_t on LP64, so a uint64 argument cannot be told apart and would read
"size" too; no call of the index classes takes one (only the encoder entry points do).  `index_traces()` makes a fixed
list of public calls over seeded data (tests/golden/synth.py) on every index class and layout and returns {label: trace};
a call that raises is recorded as ["raises", [type, message]] behind the calls it made.  It uses the public API and `_lib` only, so it runs on any tree that has them.

    python tests/call_trace.py --write --commit <hash of the tree it runs on>

writes tests/golden/index_call_trace.json; the test compares a later tree's traces with that file.
"""
import argparse
import contextlib
import ctypes as C
import inspect
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden"
for _p in (str(ROOT), str(GOLDEN)):
    if _p not in sys.path:
        sys.path.insert(0, _p)

TRACE_FILE = GOLDEN / "index_call_trace.json"

_BY_VALUE = (C.c_int, C.c_int64)


def _recorded(ctype, arg):
    if ctype is C.c_size_t:  # (and c_uint64, the same class on LP64: the module docstring)
        return "size"
    if ctype in _BY_VALUE:
        return int(arg)
    if ctype is C.c_float:
        return float(C.c_float(arg).value)
    if ctype is C.c_void_p:
        if isinstance(arg, C.c_void_p):
            arg = arg.value
        return "ptr" if arg else "null"
    return "other"


class _Proxy:
    def __init__(self, real, calls):
        self._real, self._calls = real, calls

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        sig = _lib().SIGNATURES.get(name)
        if sig is None:
            return fn

        def call(*args):
            self._calls.append([name, [_recorded(t, a) for t, a in zip(sig[1], args)]])
            return fn(*args)

        return call


def _lib():
    from twotowermlretrieval_amd import _lib as L
    return L


@contextlib.contextmanager
def tracing():
    """The calls made inside the block, as a list that fills while it runs."""
    L = _lib()
    calls = []
    proxy = _Proxy(L.lib(), calls)
    real = L.lib
    L.lib = lambda: proxy
    try:
        yield calls
    finally:
        L.lib = real


N, D, B, K, OFF = 200, 64, 3, 5, 7   # the exact indexes
SCREEN_N, SCREEN_D = 4096, 256       # the screened ones: one 4096-row block, as the cross-stream tests screen
SHARD_K = 16
MIN_SCORE = 0.1


class _Data:
    """Rows, queries and every other argument of the calls, for a corpus of n rows x d numbered from OFF."""

    def __init__(self, n: int, d: int, seed: int):
        import numpy as np
        import torch
        import synth
        import twotowermlretrieval_amd as tt
        rs = np.random.RandomState(seed)
        self.n, self.d = n, d
        self.host_bf16 = torch.from_numpy(synth.unit_rows(seed + 1, n, d)).to(torch.bfloat16)
        self.bf16 = self.host_bf16.cuda()
        self.f32 = self.bf16.to(torch.float32)
        self.q = torch.from_numpy(synth.unit_rows(seed + 2, B, d)).cuda()
        self.keep = tt.pack_keep_mask(torch.from_numpy(rs.rand(n) < 0.7).cuda())
        self.exclude = torch.from_numpy(rs.randint(OFF, OFF + n, size=(B, 2)).astype(np.int64)).cuda()
        cand = rs.randint(OFF, OFF + n, size=(B, 12)).astype(np.int64)
        cand[:, 3], cand[:, 7], cand[:, 9] = -1, OFF + n + 5, cand[:, 1]  # padding, beyond the corpus, a repeat
        self.cand = torch.from_numpy(cand).cuda()
        self.tags = torch.from_numpy(rs.randint(0, 8, size=n).astype(np.int32)).cuda()
        self.match_value = torch.from_numpy(rs.randint(0, 4, size=B).astype(np.int32)).cuda()
        self.bias = torch.from_numpy((rs.standard_normal(n) * 0.05).astype(np.float32)).cuda()
        g = (np.arange(n) % 7).astype(np.int64)
        g[rs.rand(n) < 0.1] = -1
        self.groups = torch.from_numpy(g).cuda()
        self.removed = torch.from_numpy(rs.randint(OFF, OFF + n, size=9).astype(np.int64)).cuda()
        torch.cuda.synchronize()


def _takes(method, name: str) -> bool:
    return name in inspect.signature(method).parameters


def _calls(ix, c: _Data, sharded: bool):
    """(label, thunk) of every public call made on one index, in order; remove_ids comes last."""
    import torch
    out = (torch.empty((B, K), dtype=torch.float32, device="cuda"), torch.empty((B, K), dtype=torch.int64, device="cuda"))
    steps = [
        ("set", lambda: (ix.set_tags(c.tags), ix.set_bias(c.bias), ix.set_groups(c.groups))),
        ("search", lambda: ix.search(c.q, K)),
        ("search_keep", lambda: ix.search(c.q, K, keep=c.keep)),
        ("search_exclude", lambda: ix.search(c.q, K, exclude=c.exclude)),
        ("search_candidates", lambda: ix.search(c.q, K, candidates=c.cand)),
        ("search_k100", lambda: ix.search(c.q, 100)),
        ("search_1d", lambda: ix.search(c.q[0], K)),
    ]
    if _takes(ix.search, "out"):
        steps.append(("search_out", lambda: ix.search(c.q, K, out=out)))
    steps += [
        ("tagged_search", lambda: ix.tagged_search(c.q, K, 0x3, c.match_value)),
        ("tagged_search_keep", lambda: ix.tagged_search(c.q, K, 0x3, c.match_value, keep=c.keep)),
        ("biased_search", lambda: ix.biased_search(c.q, K)),
        ("biased_search_keep", lambda: ix.biased_search(c.q, K, keep=c.keep)),
    ]
    if _takes(ix.biased_search, "exclude"):
        steps.append(("biased_search_exclude", lambda: ix.biased_search(c.q, K, exclude=c.exclude)))
    steps += [
        ("search_after", lambda: ix.search_after(c.q, K, after=(0.05, -1))),
        ("search_after_keep_exclude", lambda: ix.search_after(c.q, K, keep=c.keep, exclude=c.exclude)),
        ("pages", lambda: list(ix.pages(c.q, K, n_pages=2))),
        ("count", lambda: ix.count(c.q, MIN_SCORE)),
        ("count_keep", lambda: ix.count(c.q, MIN_SCORE, keep=c.keep)),
        ("range_search", lambda: ix.range_search(c.q, MIN_SCORE, K)),
        ("score_ids", lambda: ix.score_ids(c.q, c.cand)),
        ("diverse_search", lambda: ix.diverse_search(c.q, K, 0.5)),
        ("collapsed_fast", lambda: ix.collapsed_search(c.q, K, max_per_group=1, exact=False)),
        ("collapsed_exact", lambda: ix.collapsed_search(c.q, K, max_per_group=1, exact=True)),
    ]
    if sharded:
        def pipeline():
            p1 = ix.submit(c.q, K)
            p2 = ix.submit(c.q, K)
            r1 = p1.result()
            r = ix.search(c.q, K)
            p3 = ix.submit(c.q, K)
            return r1, r, p2.result(), p3.result()

        steps.append(("submit_pipeline", pipeline))
    steps += [
        ("remove_ids", lambda: ix.remove_ids(c.removed)),
        ("search_removed", lambda: ix.search(c.q, K)),
    ]
    return steps


def _trace_index(traces: dict, label: str, make, c: _Data, sharded: bool = False) -> None:
    import torch

    def run(name, thunk):
        with tracing() as calls:
            try:
                res = thunk()
            except Exception as e:  # noqa: BLE001 -- a refusal is part of the record
                res = None
                calls.append(["raises", [type(e).__name__, str(e)]])
        torch.cuda.synchronize()
        traces[f"{label}/{name}"] = list(calls)
        return res

    ix = run("build", make)
    for name, thunk in _calls(ix, c, sharded):
        run(name, thunk)


def index_traces() -> dict:
    """{label: [[name, args], ...]} of the fixed list of calls on every index class and layout."""
    import twotowermlretrieval_amd as tt
    from twotowermlretrieval_amd import index as _index
    traces = {}
    c = _Data(N, D, 900)
    _trace_index(traces, "brute_f32", lambda: tt.BruteForceIndex(c.f32, idx_offset=OFF), c)
    _trace_index(traces, "brute_bf16", lambda: tt.BruteForceIndex(c.bf16, idx_offset=OFF), c)
    _trace_index(traces, "streamed_b64", lambda: tt.StreamedIndex(c.host_bf16, block_docs=64, idx_offset=OFF), c)
    _trace_index(traces, "streamed_b50", lambda: tt.StreamedIndex(c.host_bf16, block_docs=50, idx_offset=OFF), c)
    _trace_index(traces, "sharded_resident", lambda: tt.ShardedIndex(c.f32, OFF, shard_k=SHARD_K), c, sharded=True)
    _trace_index(traces, "sharded_streamed", lambda: tt.ShardedIndex(
        tt.StreamedIndex(c.host_bf16, block_docs=64, idx_offset=OFF), OFF, shard_k=SHARD_K), c, sharded=True)
    s = _Data(SCREEN_N, SCREEN_D, 910)
    min_docs = _index.SCREEN_MIN_DOCS
    _index.SCREEN_MIN_DOCS = 0  # (the cross-stream tests screen their small corpora the same way)
    try:
        _trace_index(traces, "screened", lambda: tt.BruteForceIndex(s.f32, idx_offset=OFF, screen=True), s)
        _trace_index(traces, "screened_masked",
                     lambda: tt.BruteForceIndex(s.f32, idx_offset=OFF, screen=True, screen_masked=True), s)
        t = _Data(SCREEN_N + 1000, SCREEN_D, 920)  # two blocks of a streamed index, 4096 and 1000 rows: each block screens
        _trace_index(traces, "streamed_screened",
                     lambda: tt.StreamedIndex(t.host_bf16, block_docs=SCREEN_N, idx_offset=OFF), t)
        _trace_index(traces, "sharded_screened", lambda: tt.ShardedIndex(s.f32, OFF, shard_k=SHARD_K, screen=True), s,
                     sharded=True)
    finally:
        _index.SCREEN_MIN_DOCS = min_docs
    return traces


def dumps(commit: str, traces: dict) -> str:
    """The file's text: one call per line, so that a difference reads as a line."""
    parts = []
    for label, calls in traces.items():
        body = ",\n".join("  " + json.dumps(call) for call in calls)
        parts.append(f" {json.dumps(label)}: [\n{body}\n ]" if calls else f" {json.dumps(label)}: []")
    return '{"commit": %s, "traces": {\n%s\n}}\n' % (json.dumps(commit), ",\n".join(parts))


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--write", action="store_true", help=f"write {TRACE_FILE.relative_to(ROOT)}")
    ap.add_argument("--commit", default="unknown", help="the commit of the tree this runs on, for the file's header")
    ap.add_argument("--to", type=Path, default=TRACE_FILE, help="another path to write to")
    args = ap.parse_args()
    text = dumps(args.commit, index_traces())
    if args.write:
        args.to.parent.mkdir(parents=True, exist_ok=True)
        args.to.write_text(text)
        print(f"{args.to}: {len(text)} bytes")
    else:
        sys.stdout.write(text)


if __name__ == "__main__":
    main()
