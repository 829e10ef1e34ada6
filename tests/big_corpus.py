"""A corpus past 2^32 elements whose exact answers need no scan on the CPU: a bounded random background on the GPU plus a few
thousand planted rows on the host, for the tests of row addresses beyond 2^31 and 2^32 elements (test_big_offsets_gpu.py; the
layout alone: test_big_corpus_cpu.py).  A helper module, not a conftest.

Layout (d = 256): N = 2^24 + 2^16 + 77 = 16 842 829 rows (not a multiple of 32): 17.25 GB as fp32 (+ 8.6 GB fp16 shadow),
8.6 GB as bf16.  With unit = 2^32 / (4 d) rows (2^22 at d = 256) the boundaries are, as row numbers: 2^32 BYTES of fp32 at every
multiple of unit; 2^31 elements (= 2^32 bytes of bf16) at 2 unit; 2^32 elements at 4 unit.  N = 4 unit + unit / 64 + 77 at any
d, so d = 512 has the same boundaries at half the row numbers (N = 2^23 + 2^15 + 77).

Background: normal_() * (BG_SCALE / sqrt(d)), filled on the GPU in chunks; build_corpus() asserts, chunk by chunk in float64, that
no background row norm exceeds BG_NORM_MAX = 0.6.  With unit-norm queries Cauchy-Schwarz bounds every background score by
0.6 (1 + 1e-6), whatever rows the generator produced; nothing but gathered rows ever reaches the host.
  BG_SCALE is 0.45, not the 0.5 first proposed: a row norm is BG_SCALE sqrt(chi2_d / d), and over 1.7e7 rows of d = 256 the
  largest sqrt(chi2_d / d) is about 1.24 (Wilson-Hilferty: P(> 1.2) = 5e-6 per row, ~85 rows), so 0.5 would break the 0.6 bound
  for certain, while 0.45 breaks it with probability ~5e-6 per corpus (it takes sqrt(chi2 / d) > 1.333: 3e-13 per row).

Planted rows P (unit norm, kept in ascending row order, so an index tie-break over P alone is the corpus's): G = 16 random unit
directions c_g; a planted row of group g is normalize(c_g + 0.5 z / sqrt(d)), and so is a query of group g, so within a group
the cosine is about 0.8 and across groups about 0.  Group 0 has 1100 rows (the k > 64 cases), groups 1..15 have 80 each (every
case with k <= 64).  Positions: rows 0 and N - 1, three rows of the last full 32-row tile, unit j - 1, unit j, unit j + 1 for
j = 1..4; of every group more than half beyond row 4 unit and a quarter in [2 unit, 4 unit]; eight exact-duplicate pairs (groups
0..7), one copy below row unit, the other above row 4 unit: ties by index ascending across every boundary.  For a bf16 corpus P
is truncated to the bf16 grid before it is scored and uploaded (exact either way).

Reference: oracle.score_all(Q, P) -- the exact fp32 chain over the planted rows -- and a stable descending sort.  It is the
corpus's answer only where the k-th planted score (a count's threshold, a rank's target score) exceeds 1.05 x the largest
background norm: Reference.topk / .count assert that for every query of every case.  It is a condition, not a tolerance: every
comparison is equality on values (bits) and indices.

What the assertions measured (layout seed 20, queries of seeds 31 / 32; test_big_corpus_cpu.py prints and bounds them):
  smallest same-group planted score over all 1024 + 40 queries: 0.7132 in fp32, 0.7110 truncated to bf16 (d = 512: 0.7412 /
  0.7391); largest other-group score 0.2822 (d = 512: 0.1855) -- on either side of the largest floor the bound allows,
  1.05 x 0.6 = 0.63, so a valid case's k-th score is always a same-group row's.
  largest background norm, as build_corpus() measured it on an MI355X (test_big_offsets_gpu.py prints it per corpus): 0.563631
  (fp32, d = 256, seed 1), 0.567350 (bf16, seed 2), 0.532491 (fp32, d = 512, seed 3); the floors are 1.05 x these.
"""
import functools

import numpy as np

D = 256
G = 16
GROUP0 = 1100
GROUP_N = 80
NOISE = 0.5
BG_SCALE = 0.45
BG_NORM_MAX = 0.6
FLOOR_FACTOR = 1.05
OFFSETS = (0, 2 ** 33 + 5)
NEG_INF = np.float32(-np.inf)
LAYOUT_SEED = 20


def to_bf16(x):
    """fp32 -> the bf16 grid (truncation), still fp32: the exactly widened rows the oracle scores."""
    return (np.ascontiguousarray(x, dtype=np.float32).view(np.uint32) & np.uint32(0xffff0000)).view(np.float32)


def _unit(x):
    x = np.asarray(x, dtype=np.float64)
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


class Layout:
    """The planted rows of one corpus shape: pos int64 [P] ascending, group int [P], rows f32 [P,d] unit norm, dups [(low, high)]
    column pairs of identical rows, and the shape itself (n, d, unit)."""

    def __init__(self, d=D, seed=LAYOUT_SEED):
        rs = np.random.RandomState(seed)
        self.d = d
        self.unit = unit = 2 ** 32 // (4 * d)
        self.n = n = 4 * unit + unit // 64 + 77
        self.last_full = last_full = (n // 32 - 1) * 32
        self.boundaries = [unit * j for j in range(1, 5)]
        self.edges = [0, *self.boundaries, n]                      # band j = rows [edges[j], edges[j + 1])
        self.specials = [0, n - 1, last_full, last_full + 15, last_full + 31] + [b + e for b in self.boundaries for e in (-1, 0, 1)]
        sizes = [GROUP0] + [GROUP_N] * (G - 1)
        # random rows come from the open interior of five ranges, so they never meet a special row or each other's range
        ranges = [(1, unit - 1), (unit + 2, 2 * unit - 1), (2 * unit + 2, 3 * unit - 1), (3 * unit + 2, 4 * unit - 1),
                  (4 * unit + 2, last_full)]
        mine = [[s for i, s in enumerate(self.specials) if i % G == g] for g in range(G)]
        need = np.zeros((G, 5), dtype=np.int64)
        for g, size in enumerate(sizes):
            hi, mid = size // 2 + 1, size // 4
            low = size - hi - mid
            want = [(low + 1) // 2, low // 2, (mid + 1) // 2, mid // 2, hi]
            have = [sum(1 for s in mine[g] if self._range_of(s) == r) for r in range(5)]
            need[g] = np.array(want) - np.array(have)
            assert (need[g] > 0).all()
        pos, group = [], []
        for r, (lo, hi) in enumerate(ranges):
            draw = lo + rs.choice(hi - lo, int(need[:, r].sum()), replace=False)
            at = 0
            for g in range(G):
                pos += draw[at:at + need[g, r]].tolist()
                group += [g] * int(need[g, r])
                at += need[g, r]
        for g in range(G):
            pos += mine[g]
            group += [g] * len(mine[g])
        order = np.argsort(pos)
        self.pos = np.asarray(pos, dtype=np.int64)[order]
        self.group = np.asarray(group)[order]
        assert len(np.unique(self.pos)) == len(self.pos) == sum(sizes) and self.pos[0] == 0 and self.pos[-1] == n - 1
        self.centres = _unit(rs.standard_normal((G, d)))
        self.rows = self._noisy(rs, self.group)
        self.dups = []
        for g in range(8):
            cols = np.flatnonzero(self.group == g)
            low, high = cols[self.pos[cols] < unit][-1], cols[self.pos[cols] > 4 * unit][0]
            self.rows[low] = self.rows[high]
            self.dups.append((int(low), int(high)))

    def _range_of(self, row):
        """0..4: which of the five ranges of random rows a row lies in (boundary rows count with the range they close)."""
        u = self.unit
        return 4 if row > 4 * u else 3 if row > 3 * u else 2 if row >= 2 * u else 1 if row >= u else 0

    def band(self, rows):
        """0..4 per row: the band between boundaries a row lies in ([0, unit), [unit, 2 unit), ..., [4 unit, n))."""
        return np.searchsorted(np.asarray(self.boundaries), rows, side="right")

    def _noisy(self, rs, groups):
        return _unit(self.centres[groups] + NOISE * rs.standard_normal((len(groups), self.d)) / np.sqrt(self.d))

    def queries(self, groups, seed):
        """Unit-norm queries f32 [len(groups), d], query i around the direction of group groups[i]."""
        return self._noisy(np.random.RandomState(seed), np.asarray(groups))

    def small_queries(self, B=1024):
        """(Q, groups): B queries cycling through groups 1..15, for every case with k <= 64."""
        groups = 1 + np.arange(B) % (G - 1)
        return self.queries(groups, 31), groups

    def group0_queries(self, B=40):
        return self.queries(np.zeros(B, dtype=np.int64), 32)

    def removals(self, seed=5, n_background=100_000):
        """(columns of P, background rows) a mask removes: in every band between boundaries 60 % of group 0's planted rows and
        15 % (at least one) of every other group's -- 36 % of the planted rows on each side of every boundary, weighted to
        group 0 so that groups 1..15 keep more than 64 rows each (a masked k = 64 search still has its k-th score among the
        planted rows) -- plus random background rows everywhere."""
        rs = np.random.RandomState(seed)
        band = self.band(self.pos)
        cols = []
        for b in range(5):
            for g in range(G):
                c = rs.permutation(np.flatnonzero((band == b) & (self.group == g)))
                cols += c[:max(1, int((0.6 if g == 0 else 0.15) * len(c)))].tolist() if len(c) else []
        cols = np.array(sorted(cols))
        dup_cols = {c for pair in self.dups for c in pair}
        cols = np.array([c for c in cols if c not in dup_cols or self.group[c] == 0])     # groups 1..7 keep their tie
        bg = np.unique(rs.randint(0, self.n, size=n_background))
        bg = np.concatenate([bg[~np.isin(bg, self.pos)], [1, self.n - 2]])
        for b in range(5):
            inb = band == b
            assert np.isin(np.flatnonzero(inb), cols).sum() >= 0.3 * inb.sum()
        for g in range(1, G):
            assert (self.group == g).sum() - (self.group[cols] == g).sum() > 64
        return cols, np.unique(bg)

    def keep_bool(self, cols, bg):
        keep = np.ones(self.n, dtype=bool)
        keep[self.pos[cols]] = False
        keep[bg] = False
        return keep


@functools.lru_cache(maxsize=None)
def layout(d=D):
    """The one Layout of width d (the fp32 and the bf16 corpus of a width share it)."""
    return Layout(d)


def pack_bits(keep_bool):
    """numpy's version of the packed keep-bitmask: bit n & 31 of uint32 word n >> 5, the bits beyond N zero."""
    padded = np.zeros((len(keep_bool) + 31) // 32 * 32, dtype=bool)
    padded[:len(keep_bool)] = keep_bool
    return np.packbits(padded, bitorder="little").view("<u4")


def build_corpus(layout, bf16, seed, chunk=1 << 18):
    """(docs [n,d] on cuda:0 -- float32, or bfloat16 --, the largest background row norm): the background filled and measured
    chunk by chunk on the device, then the planted rows written over it."""
    import torch
    n, d = layout.n, layout.d
    gen = torch.Generator(device="cuda")
    gen.manual_seed(seed)
    docs = torch.empty((n, d), dtype=torch.bfloat16 if bf16 else torch.float32, device="cuda")
    worst = torch.zeros((), dtype=torch.float64, device="cuda")
    scale = BG_SCALE / float(np.sqrt(d))
    tmp = torch.empty((chunk, d), dtype=torch.float32, device="cuda") if bf16 else None
    for lo in range(0, n, chunk):
        blk = docs[lo:lo + chunk]
        if bf16:
            t = tmp[:len(blk)]
            t.normal_(generator=gen).mul_(scale)
            blk.copy_(t)
        else:
            blk.normal_(generator=gen).mul_(scale)
        worst = torch.maximum(worst, torch.linalg.vector_norm(blk, dim=1, dtype=torch.float64).max())   # of the stored values
    del tmp
    bg_norm = float(worst)
    assert 0.3 < bg_norm <= BG_NORM_MAX, f"largest background row norm {bg_norm}"
    rows = to_bf16(layout.rows) if bf16 else layout.rows
    docs[torch.from_numpy(layout.pos).cuda()] = torch.from_numpy(rows).cuda().to(docs.dtype)     # (exact: on the grid already)
    return docs, bg_norm


class Reference:
    """The expected answers of one corpus: everything from oracle.score_all over the planted rows, valid above `floor`."""

    def __init__(self, oracle, layout, bf16, bg_norm):
        self.oracle, self.layout = oracle, layout
        self.P = to_bf16(layout.rows) if bf16 else layout.rows
        self.pos = layout.pos
        self.floor = np.float32(FLOOR_FACTOR * bg_norm)
        self._S = {}

    def scores(self, Q, key):
        """oracle.score_all(Q, P) f32 [B,P], computed once per key and never written to."""
        if key not in self._S:
            S = self.oracle.score_all(Q, self.P)
            S.setflags(write=False)
            self._S[key] = S
        return self._S[key]

    @staticmethod
    def without(S, removed):
        if removed is None:
            return S
        S = S.copy()
        S[:, removed] = NEG_INF
        return S

    def topk(self, S, k, off=0, removed=None):
        """(vals f32 [B,k], ids int64 [B,k]) = the exact top-k of the corpus for the queries of S, (score desc, row asc); the
        columns `removed` left out.  Asserts the case's validity: every query's k-th score lies above the background."""
        S = self.without(S, removed)
        order = np.argsort(-S, axis=1, kind="stable")[:, :k]        # (columns ascend with the rows: stable = row asc)
        vals = np.take_along_axis(S, order, 1)
        assert (vals[:, -1] > self.floor).all(), ("k-th planted score not above the background bound", float(vals[:, -1].min()), self.floor)
        return vals, self.pos[order] + off

    def count(self, S, thr, removed=None):
        """int64 [B]: how many rows of the corpus score >= thr[b] (thr above the background bound: asserted)."""
        thr = np.asarray(thr, dtype=np.float32)
        assert (thr > self.floor).all(), ("threshold not above the background bound", float(thr.min()), self.floor)
        return (self.without(S, removed) >= thr[:, None]).sum(1).astype(np.int64)
