"""The corpus, the queries and the list of calls the cross-stream tests share (tests/test_streams_*_gpu.py).

Corpus: N = 17 400 unit rows x 256 (synth.unit_rows) rounded through bf16, so an fp32, a bf16 and a streamed index hold the
same values and answer bit for bit alike; tags, biases and group ids are set and 40 ids are removed (`dress`).  With
block_docs = 4096 a StreamedIndex walks 5 blocks, the last of 1 016 rows.
Queries: 'a' is B = 130 (the screen's shared-tile form), 'b' is B = 5 (its streaming form), different rows.
CALLS: name -> call(index, cases, 'a' | 'b'); every argument beside the index is made once, on the default stream."""
import functools

import numpy as np
import torch

import synth

N, DIM, K = 17_400, 256, 10
BLOCK = 4096
MIN_SCORE = 0.12  # ~ 2 sigma of a random unit pair's score at d = 256 (sigma = 1/16): a few hundred matches per query


class Cases:
    def __init__(self):
        import twotowermlretrieval_amd as tt
        rows = torch.from_numpy(synth.unit_rows(41, N, DIM)).to(torch.bfloat16)
        self.host_bf16 = rows                                  # what a StreamedIndex / a bf16 index is built from
        self.rows = rows.to(torch.float32)                     # the same values widened (exact)
        rs = np.random.RandomState(43)
        self.q, self.excl, self.cand, self.match = {}, {}, {}, {}
        top = {}
        for s, (seed, B) in {"a": (44, 130), "b": (45, 5)}.items():
            q = synth.unit_rows(seed, B, DIM)
            self.q[s] = torch.from_numpy(q).cuda()
            top[s] = np.argsort(-(q @ self.rows.numpy().T), axis=1, kind="stable")[:, :40]
        # removed: the best row of some queries (so a removal shows) and random ones, 40 ids in all
        first = np.unique(np.concatenate([top["a"][:12, 0], top["b"][:3, 0]]))
        rest = np.setdiff1d(rs.permutation(N), first)[:40 - first.size]
        self.removed = torch.from_numpy(np.concatenate([first, rest]).astype(np.int64))
        assert self.removed.numel() == 40
        for s in ("a", "b"):
            B = top[s].shape[0]
            self.excl[s] = torch.from_numpy(top[s][:, 1:5].astype(np.int64)).cuda()
            # candidates: the 30 best, 14 random rows, a removed id, an id beyond the corpus, padding, a repeat
            cand = np.concatenate([top[s][:, :30], rs.randint(0, N, size=(B, 14)),
                                   np.full((B, 1), int(self.removed[0])), np.full((B, 1), N + 7), np.full((B, 1), -1),
                                   top[s][:, 2:3]], axis=1).astype(np.int64)
            self.cand[s] = torch.from_numpy(cand).cuda()
            self.match[s] = (torch.full((B,), 0x3, dtype=torch.int32, device="cuda"),
                             torch.from_numpy(rs.randint(0, 4, size=B).astype(np.int32)).cuda())
        self.tags = torch.from_numpy(rs.randint(0, 8, size=N).astype(np.int32)).cuda()
        self.bias = torch.from_numpy((rs.standard_normal(N) * 0.05).astype(np.float32)).cuda()
        g = (np.arange(N) % 50).astype(np.int64)
        g[rs.rand(N) < 0.1] = -1                               # ungrouped rows are never collapsed
        self.groups = torch.from_numpy(g).cuda()
        self.keep = tt.pack_keep_mask(torch.from_numpy(rs.rand(N) < 0.7).cuda())
        self._page1 = {}
        torch.cuda.synchronize()

    def dress(self, ix):
        """Tags, biases, group ids and the removals onto an index (a ShardedIndex of world 1 included)."""
        ix.set_tags(self.tags)
        ix.set_bias(self.bias)
        ix.set_groups(self.groups)
        ix.remove_ids(self.removed.cuda())
        torch.cuda.synchronize()
        return ix

    def page1_tail(self, ix, s):
        """The cursor of page 2: the last column of the SERIAL page 1 (made once per index and query set, synchronised)."""
        key = (id(ix), s)
        if key not in self._page1:
            torch.cuda.synchronize()
            v, i = ix.search_after(self.q[s], K)
            self._page1[key] = (v[:, -1].clone(), i[:, -1].clone())
            torch.cuda.synchronize()
        return self._page1[key]


@functools.lru_cache(maxsize=1)
def cases() -> Cases:
    return Cases()


CALLS = {
    "search": lambda ix, c, s: ix.search(c.q[s], K),
    "search_k100": lambda ix, c, s: ix.search(c.q[s], 100),
    "search_keep": lambda ix, c, s: ix.search(c.q[s], K, keep=c.keep),
    "search_exclude": lambda ix, c, s: ix.search(c.q[s], K, exclude=c.excl[s]),
    "search_candidates": lambda ix, c, s: ix.search(c.q[s], K, candidates=c.cand[s]),
    "tagged_search": lambda ix, c, s: ix.tagged_search(c.q[s], K, *c.match[s]),
    "biased_search": lambda ix, c, s: ix.biased_search(c.q[s], K),
    "search_after": lambda ix, c, s: ix.search_after(c.q[s], K, after=c.page1_tail(ix, s)),
    "count": lambda ix, c, s: ix.count(c.q[s], MIN_SCORE),
    "range_search": lambda ix, c, s: ix.range_search(c.q[s], MIN_SCORE, K),
    "score_ids": lambda ix, c, s: ix.score_ids(c.q[s], c.cand[s]),
    "diverse_search": lambda ix, c, s: ix.diverse_search(c.q[s], K, 0.5),
    "collapsed_fast": lambda ix, c, s: ix.collapsed_search(c.q[s], K, max_per_group=1, exact=False),
    "collapsed_exact": lambda ix, c, s: ix.collapsed_search(c.q[s], K, max_per_group=1, exact=True),
}


class Wants:
    """The serial result of (index, call, query set), computed once on the default stream and never written again."""

    def __init__(self):
        self._want = {}

    def __call__(self, ix, name, s):
        import stream_sched as ss
        key = (id(ix), name, s)
        if key not in self._want:
            c = cases()
            if name == "search_after":
                c.page1_tail(ix, s)
            self._want[key] = ss.serial(lambda: CALLS[name](ix, c, s))
        return self._want[key]


def oracle_topk_without(oracle, q: np.ndarray, rows: np.ndarray, removed: np.ndarray, k: int):
    """The oracle's exact top-k over the rows that are not removed: its top-(k + len(removed)) with the removed ids struck
    out (at most len(removed) of them can be in it), cut to k."""
    v, i = oracle.score_topk(q, rows, k + removed.size)
    out_v, out_i = np.empty((q.shape[0], k), np.float32), np.empty((q.shape[0], k), np.int64)
    for b in range(q.shape[0]):
        ok = ~np.isin(i[b], removed)
        out_v[b], out_i[b] = v[b][ok][:k], i[b][ok][:k]
    return out_v, out_i
