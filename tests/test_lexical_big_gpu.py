"""Lexical search where its 64-bit addresses pass 2^32 bytes, 2^31 and 2^32 elements: the nnz stream (p0 + t * 64 + lane, the
indptr values), S[b * N + r], base[b * base_stride + r], keep[r >> 5], and the plan at the largest N a call accepts.  All
comparisons are equality on bits and indices with tests/lexical_ref.py.  One large allocation is alive at a time (module-scoped
holder, as in test_big_offsets_gpu.py): the nnz buffers (34.4 GB) first, then the rows corpus with S (8.7 GB) and base
(25.8 GB) in turn, then the indptr at the cap (17.2 GB, with S [3, N]: 25.8 GB more).

1. The nnz stream.  cols and vals are bases and indptr carries absolute positions, so the `main` corpus of test_lexical_gpu.py
   (lexical_ref.MainCorpus: N = 3 C + 17) can live anywhere in two buffers of 2^32 + 2^20 entries, and its scores are its own.
   Both buffers are filled whole with a decoy: column 256 -- which no row of the corpus holds and every query of this module
   weights 1 -- and value 64, so an entry read from a wrong address moves a score by a multiple of 64 (no score of the corpus
   exceeds 40).  The stream is copied to one base at a time -- nine placements: boundary Z in {2^30, 2^31, 2^32} entries x
     a: Z is a staging-piece edge of the last wave of chunk 1, strictly inside the 3 000-entry row 2 C - 1;
     b: Z is the first entry of row C: between two workgroups;
     c: Z is the second entry of a short row at lane 31 of a wave --
   each with an indptr of its own (asserted on the host), and the decoy is put back behind it.
2. Rows.  N = 2^24 + 2^16 + 77 (big_corpus.py's N), F = 257, all rows empty but about 2 000 planted ones (1..12 entries,
   positive values, columns below 254), indptr built on the device by a cumsum.  Planted: 0, N - 1, the first and last row of the
   last chunk, 2^22 j - 1, 2^22 j, 2^22 j + 1 for j = 1..4; eight duplicate pairs straddle those.  Every other score is +0, so
   a top-k is the planted rows above zero, then the zero rows in index order (sparse_topk below) -- across 4 113 chunks and both
   merge steps.  Column 254 is held by the duplicate pairs only (they rank near the top of the query that weights it), column
   255 by five planted rows only: its query has fewer than k hits.
3. The cap.  N = 2^31 - 65, B = 1: 524 288 chunks, 725 lists per group, 724 groups; indptr constant but for 40 planted rows."""
import gc

import numpy as np
import pytest
import torch

import lexical_ref as ref
import poison

pytestmark = pytest.mark.gpu

F = ref.MAIN_F
DECOY_COL, DECOY_VAL = F - 1, 64.0
NNZ_LEN = 2 ** 32 + 2 ** 20
BOUNDARIES = (2 ** 30, 2 ** 31, 2 ** 32)
OFFSETS = (0, 2 ** 33 + 5)
N_ROWS = 2 ** 24 + 2 ** 16 + 77
N_CAP = 2 ** 31 - 65
PIECE = 512


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _q(queries):
    return tuple(_dev(a) for a in ref.queries_csr(queries))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _assert_rows(got, want, what=""):
    v, i = (x.cpu().numpy() for x in got)
    for b, (wv, wi) in enumerate(want):
        assert np.array_equal(i[b], wi), (what, b, i[b][:12], wi[:12])
        assert np.array_equal(_bits(v[b]), _bits(wv)), (what, b, v[b][:12], wv[:12])


def nonzero_words(t, chunk=1 << 28):
    """How many 32-bit words of t are not zero (a -0 counts), counted on the device in pieces: torch.count_nonzero over
    6.4 G elements at once takes 58 GB of temporaries."""
    words = t.view(torch.int32).view(-1)
    total = torch.zeros((), dtype=torch.int64, device=t.device)
    for lo in range(0, words.numel(), chunk):
        total += torch.count_nonzero(words[lo:lo + chunk])
    return int(total)


def sparse_topk(pos, s, N, k, off=0, removed=()):
    """ref_topk of the N-row score vector that is s at the rows pos (ascending) and +0 elsewhere, without forming it: the rows
    above zero by (value desc, row asc), then the lowest-numbered zero rows, the rows in `removed` left out.  s >= 0."""
    assert (np.diff(pos) > 0).all() and (s >= 0).all()
    gone = set(int(r) for r in removed)
    live = np.array([int(r) not in gone for r in pos], dtype=bool)
    hit = live & (s > 0)
    order = np.flatnonzero(hit)[np.argsort(-s[hit], kind="stable")][:k]
    vals, idx = list(s[order]), list(pos[order])
    skip = gone | set(int(r) for r in pos[hit])
    r = 0
    while len(idx) < k and r < N:
        if r not in skip:
            vals.append(np.float32(0))
            idx.append(r)
        r += 1
    out_v = np.full(k, -np.inf, dtype=np.float32)
    out_i = np.full(k, -1, dtype=np.int64)
    out_v[:len(vals)] = vals
    out_i[:len(idx)] = np.asarray(idx, dtype=np.int64) + off
    return out_v, out_i


# ---- the three families ----------------------------------------------------------------------------------------------------
class NnzFamily:
    """The two decoy-filled nnz buffers and the main corpus on the host."""

    def __init__(self, tt, lib):
        self.tt = tt
        self.C = C = lib.tt_lexical_chunk_docs()
        self.m = m = ref.MainCorpus(C)
        assert DECOY_COL not in m.cols and max(float(np.abs(s).max()) for s in m.S.values()) < DECOY_VAL - 1
        self.cols = torch.empty(NNZ_LEN, dtype=torch.int32, device="cuda")
        self.vals = torch.empty(NNZ_LEN, dtype=torch.float32, device="cuda")
        self.cols.fill_(DECOY_COL)
        self.vals.fill_(DECOY_VAL)
        self.stream = (_dev(m.cols), _dev(m.vals))
        self.names = ("random", "every", "tie")
        queries = []
        for n in self.names:                              # every query holds the decoy column with weight 1
            c, v = (np.asarray(a).copy() for a in m.queries[n])
            if DECOY_COL in c:
                v[c == DECOY_COL] = 1.0
            else:
                c, v = np.append(c, DECOY_COL), np.append(v, np.float32(1.0))
            queries.append((c, v.astype(np.float32)))
        self.q = _q(queries)
        self.placed = None

    def base_of(self, Z, align):
        """The buffer position of the corpus's entry 0 for which boundary Z falls as alignment `align` says (module docstring)."""
        ip, C = self.m.indptr, self.C
        if align == "a":
            a = int(ip[2 * C - 64])                       # the span of the wave that owns rows 2 C - 64 .. 2 C - 1 starts here
            j = (int(ip[2 * C - 1]) - a) // PIECE + 1
            at = a + PIECE * j
            assert ip[2 * C - 1] < at < ip[2 * C] - 1 and (at - a) % PIECE == 0 and ip[2 * C] - ip[2 * C - 1] == 3000
        elif align == "b":
            at = int(ip[C])
            assert ip[C + 1] > ip[C]                      # (row C, a tie row, is not empty: Z is its first entry)
        else:
            lens = np.diff(ip)
            r = next(r for r in range(C + 5 * 64 + 31, 3 * C, 64) if lens[r] >= 3)
            at = int(ip[r]) + 1
            assert r % 64 == 31 and ip[r] < at < ip[r + 1] - 1
        return Z - at

    def place(self, Z, align):
        """indptr (device, absolute positions) of the corpus with its stream copied so that Z falls as `align` says."""
        self.unplace()
        base, nnz = self.base_of(Z, align), self.m.cols.size
        assert 0 <= base and base < Z < base + nnz <= NNZ_LEN
        self.cols[base:base + nnz] = self.stream[0]
        self.vals[base:base + nnz] = self.stream[1]
        self.placed = (base, nnz)
        return _dev(self.m.indptr + base)

    def unplace(self):
        if self.placed:
            base, nnz = self.placed
            self.cols[base:base + nnz].fill_(DECOY_COL)
            self.vals[base:base + nnz].fill_(DECOY_VAL)
            self.placed = None

    def free(self):
        self.cols = self.vals = self.stream = None


class RowsFamily:
    """N_ROWS rows, about 2 000 of them planted; everything N-sized is made on the device."""

    def __init__(self, tt, lib):
        self.tt = tt
        rng = np.random.default_rng(61)
        N = self.N = N_ROWS
        C = lib.tt_lexical_chunk_docs()
        self.n_chunks = -(-N // C)
        last = (self.n_chunks - 1) * C
        u = 2 ** 22
        self.specials = sorted({0, N - 1, last, *(u * j + e for j in range(1, 5) for e in (-1, 0, 1))})
        edges = [0, u, 2 * u, 3 * u, 4 * u, N]
        rand = np.concatenate([lo + 2 + rng.choice(hi - lo - 4, size=400, replace=False)
                               for lo, hi in zip(edges[:-1], edges[1:-1] + [last])] + [last + 1 + rng.choice(N - last - 3, 30, replace=False)])
        self.pos = pos = np.unique(np.concatenate([self.specials, rand])).astype(np.int64)
        assert 2000 < pos.size < 2100 and pos[0] == 0 and pos[-1] == N - 1 and (N - 1) // C == self.n_chunks - 1
        rows = []
        for _ in pos:
            m = int(rng.integers(1, 13))
            rows.append((np.sort(rng.choice(254, size=m, replace=False)).astype(np.int32),
                         rng.uniform(0.01, 1.0, size=m).astype(np.float32)))
        at = {int(r): n for n, r in enumerate(pos)}
        # eight duplicate pairs: across every multiple of 2^22 (row before / row after), and from below 2^22 to above 2^24; the
        # copies hold column 254 (value 1), which the first query of the searches weights 1: they rank near the top
        low, high = pos[(pos > 5) & (pos < u - 5)], pos[pos > 4 * u + 5]
        self.dups = [(u * j - 1, u * j + 1) for j in range(1, 5)] + [(int(low[7 * n + 3]), int(high[5 * n + 2])) for n in range(4)]
        for a, b in self.dups:
            c, v = rows[at[a]]
            rows[at[a]] = rows[at[b]] = (np.append(c, np.int32(254)), np.append(v, np.float32(1.0)))
        self.rare = [u, 2 * u, 4 * u, last, N - 1]                            # the only rows that hold column 255
        assert not set(self.rare) & {r for pair in self.dups for r in pair}
        for r in self.rare:
            c, v = rows[at[r]]
            rows[at[r]] = (np.append(c, np.int32(255)), np.append(v, np.float32(rng.uniform(0.5, 1.0))))
        lens = np.array([len(c) for c, _ in rows], dtype=np.int64)
        self.p_ip = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)   # the planted rows as a corpus of their own
        self.p_cols = np.concatenate([c for c, _ in rows]).astype(np.int32)
        self.p_vals = np.concatenate([v for _, v in rows]).astype(np.float32)
        length = torch.zeros(N, dtype=torch.int64, device="cuda")
        length[_dev(pos)] = _dev(lens)
        indptr = torch.zeros(N + 1, dtype=torch.int64, device="cuda")
        torch.cumsum(length, 0, out=indptr[1:])
        del length
        self.t = (indptr, _dev(self.p_cols), _dev(self.p_vals))
        assert int(indptr[-1]) == self.p_cols.size
        self.pos_dev = _dev(pos)
        # removals: the planted rows on both sides of every special position, and row 0
        sp = np.flatnonzero(np.isin(pos, self.specials))
        cols = np.unique(np.clip(np.concatenate([sp - 1, sp + 1, [0]]), 0, pos.size - 1))
        self.removed = pos[cols]
        keep = torch.ones(N, dtype=torch.bool, device="cuda")
        keep[_dev(self.removed)] = False
        self.keep = tt.pack_keep_mask(keep)
        assert self.keep.numel() == (N + 31) // 32 and 0 in self.removed and int(self.removed.max()) > 4 * u
        self._S = {}

    def scores(self, key, queries):
        """ref_scores32 over the planted rows, one float32 [planted] per query; computed once per key."""
        if key not in self._S:
            S = np.stack([ref.ref_scores32(self.p_ip, self.p_cols, self.p_vals, ref.dense_query(*q, F)) for q in queries])
            S.setflags(write=False)
            self._S[key] = S
        return self._S[key]

    def free(self):
        self.t = self.keep = self.pos_dev = None


class CapFamily:
    """N = 2^31 - 65: the indptr (17.2 GB) is written in 41 constant runs between 40 planted rows."""

    def __init__(self, tt, lib):
        self.tt, self.lib = tt, lib
        rng = np.random.default_rng(71)
        N = self.N = N_CAP
        C = lib.tt_lexical_chunk_docs()
        self.n_chunks = -(-N // C)
        assert self.n_chunks == 2 ** 19 and (N - 1) // C == 2 ** 19 - 1
        last = (2 ** 19 - 1) * C
        self.pos = pos = np.array([*range(7, 17), *range(2 ** 30 - 5, 2 ** 30 + 5), *range(last, last + 10), *range(N - 10, N)],
                                  dtype=np.int64)
        rows = [(np.sort(rng.choice(255, size=m, replace=False)).astype(np.int32), rng.uniform(0.01, 1.0, size=m).astype(np.float32))
                for m in rng.integers(1, 13, size=pos.size)]
        self.rare = [8, 2 ** 30, last, N - 1]
        for r in self.rare:
            n = int(np.flatnonzero(pos == r)[0])
            rows[n] = (np.append(rows[n][0], np.int32(255)), np.append(rows[n][1], np.float32(0.5)))
        lens = np.array([len(c) for c, _ in rows], dtype=np.int64)
        self.p_ip = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        self.p_cols = np.concatenate([c for c, _ in rows]).astype(np.int32)
        self.p_vals = np.concatenate([v for _, v in rows]).astype(np.float32)
        indptr = torch.empty(N + 1, dtype=torch.int64, device="cuda")
        start = 0
        for n, r in enumerate(pos):                       # indptr[x] = entries of the planted rows below x
            indptr[start:int(r) + 1].fill_(int(self.p_ip[n]))
            start = int(r) + 1
        indptr[start:].fill_(int(self.p_ip[-1]))
        self.t = (indptr, _dev(self.p_cols), _dev(self.p_vals))
        self.pos_dev = _dev(pos)
        self.queries = [(rng.choice(255, size=60, replace=False), rng.uniform(0.05, 1.0, size=60).astype(np.float32)),
                        (np.array([255]), np.array([0.5], dtype=np.float32)),
                        (np.arange(255), rng.uniform(0.05, 1.0, size=255).astype(np.float32))]      # every planted row scores
        self.S = np.stack([ref.ref_scores32(self.p_ip, self.p_cols, self.p_vals, ref.dense_query(*q, F)) for q in self.queries])

    def free(self):
        self.t = self.pos_dev = None


class Holder:
    def __init__(self):
        self.live = {}

    def get(self, kind):
        if kind not in self.live:
            self.release()
            import twotowermlretrieval_amd as tt
            from twotowermlretrieval_amd import _lib
            self.live[kind] = {"nnz": NnzFamily, "rows": RowsFamily, "cap": CapFamily}[kind](tt, _lib.lib())
        return self.live[kind]

    def release(self):
        for fam in self.live.values():
            fam.free()
        self.live.clear()
        gc.collect()
        torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def big():
    holder = Holder()
    yield holder
    holder.release()


# ---- 1. the nnz stream -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("align", ["a", "b", "c"])
@pytest.mark.parametrize("Z", BOUNDARIES, ids=["2^30", "2^31", "2^32"])
def test_nnz_stream_across(big, Z, align):
    fam = big.get("nnz")
    tt, m, C = fam.tt, fam.m, fam.C
    indptr = fam.place(Z, align)
    try:
        t = (indptr, fam.cols, fam.vals)
        S = tt.lexical_score_all(t, F, fam.q).cpu().numpy()
        for b, n in enumerate(fam.names):
            bad = np.flatnonzero(_bits(S[b]) != _bits(m.S[n]))
            assert bad.size == 0, (n, bad[:8], S[b][bad[:8]], m.S[n][bad[:8]])
        for k in (10, 1024):
            _assert_rows(tt.lexical_score_topk(t, F, fam.q, k), [ref.ref_topk(m.S[n], k) for n in fam.names], f"k={k}")
        if align == "a":
            # the rows from r0 on as a slice (indptr[r0:], the same bases), ids global
            r0 = C + 5
            off = 2 ** 33 + 5 + r0
            for k in (10, 1024):
                got = tt.lexical_score_topk((indptr[r0:], fam.cols, fam.vals), F, fam.q, k, idx_offset=off)
                _assert_rows(got, [ref.ref_topk(m.S[n][r0:], k, idx_offset=off) for n in fam.names], f"slice k={k}")
            # a LexicalIndex over the placed corpus: its constructor validates a matrix that starts at entry 0 and downloads
            # it whole, so it is built over a one-row matrix and handed the placed tensors
            ix = tt.LexicalIndex((_dev(np.array([0, 1], dtype=np.int64)), _dev(np.array([0], dtype=np.int32)),
                                  _dev(np.array([1.0], dtype=np.float32)), F), idx_offset=OFFSETS[1])
            ix.indptr, ix.cols, ix.vals = t
            assert ix.ntotal == m.N
            _, best = ref.ref_topk(m.S["random"], 3)
            gone = [int(best[0]), int(best[2]), 0, 2 * C - 1, m.N - 1]
            keep = np.ones(m.N, dtype=bool)
            keep[gone] = False
            ix.remove_ids([g + OFFSETS[1] for g in gone] + [5, OFFSETS[1] + m.N + 3])
            _assert_rows(ix.search(fam.q, 20), [ref.ref_topk(m.S[n], 20, keep=keep, idx_offset=OFFSETS[1]) for n in fam.names], "index")
    finally:
        fam.unplace()


# ---- 2. rows, outputs, base and keep ------------------------------------------------------------------------------------------
def _row_queries(seed, B):
    rng = np.random.default_rng(seed)
    return [(rng.choice(254, size=20, replace=False), rng.uniform(0.05, 1.0, size=20).astype(np.float32)) for _ in range(B)]


def _search_queries():
    """Two random queries, the first with the duplicate pairs' column 254, and the query of column 255 (five hits)."""
    q = _row_queries(64, 2)
    q[0] = (np.append(q[0][0], 254), np.append(q[0][1], np.float32(1.0)))
    return q + [(np.array([255]), np.array([1.0], dtype=np.float32))]


def test_rows_score_all_past_2_31_elements(big):
    fam = big.get("rows")
    B, N = 129, fam.N
    assert (B - 1) * N > 2 ** 31
    queries = _row_queries(62, B)
    want = fam.scores("all", queries)
    S = fam.tt.lexical_score_all(fam.t, F, _q(queries))
    assert tuple(S.shape) == (B, N)
    assert nonzero_words(S) == int(np.count_nonzero(want)) > B * 500
    got = S[:, fam.pos_dev].cpu().numpy()
    assert np.array_equal(_bits(got), _bits(want))
    rng = np.random.default_rng(63)
    empty = np.setdiff1d(np.concatenate([rng.integers(0, N, size=2300), rng.integers(2 ** 24, N, size=2300)]), fam.pos)[:4096]
    assert empty.size == 4096 and (empty > 2 ** 24).sum() > 1000
    assert not S[:, _dev(empty)].view(torch.int32).any()


@pytest.mark.parametrize("k", [10, 100, 1024])
def test_rows_search_through_the_two_step_merge(big, k):
    fam = big.get("rows")
    N = fam.N
    assert fam.n_chunks == 4113                            # 65 lists in each of 64 groups
    queries = _search_queries()
    S = fam.scores("topk", queries)
    assert (S[2] > 0).sum() == 5 < k and (S[0] > 0).sum() > 100
    q = _q(queries)
    for off in OFFSETS:
        _assert_rows(fam.tt.lexical_score_topk(fam.t, F, q, k, idx_offset=off), [sparse_topk(fam.pos, s, N, k, off) for s in S],
                     f"k={k} off={off}")
    # the duplicate pairs tie across the boundaries: the lower row first
    want = sparse_topk(fam.pos, S[0], N, k)[1].tolist()
    tied = [(a, b) for a, b in fam.dups if a in want and b in want]
    assert len(tied) == (8 if k >= 100 else len(tied)) > 0 and all(want.index(b) == want.index(a) + 1 for a, b in tied)
    # keep= over N booleans, then the same removals by global id on an index
    off = OFFSETS[1]
    want = [sparse_topk(fam.pos, s, N, k, off, removed=fam.removed) for s in S]
    assert any((sparse_topk(fam.pos, s, N, k, off)[1] != w[1]).any() for s, w in zip(S, want))
    _assert_rows(fam.tt.lexical_score_topk(fam.t, F, q, k, idx_offset=off, keep=fam.keep), want, f"keep k={k}")
    if k == 100:
        ix = fam.tt.LexicalIndex((*fam.t, F), idx_offset=off)
        junk = [off - 1, off + N, off + N + 31, -1, 5]
        ix.remove_ids(_dev(np.concatenate([fam.removed + off, junk]).astype(np.int64)))
        assert torch.equal(ix.keep_mask, fam.keep)
        _assert_rows(ix.search(q, k), want, "removed by id")


def test_rows_base_past_2_32_elements(big):
    """base: a [3, N] view, row stride 2^31 + 64, of a torch.empty buffer of 3 x (2^31 + 64) floats (row 2 starts past 2^32
    elements); only the first N columns of each row are written.  The candidates the reference looks at are the planted rows
    and the 2 000 rows with the largest base value per query; every other row's value is fl(0.3 base) + 0 <= fl(0.3 x the
    2 001st largest base), below the k-th expected value (asserted), so the union is sufficient."""
    fam = big.get("rows")
    N, stride, k = fam.N, 2 ** 31 + 64, 10
    queries = _search_queries()
    S = fam.scores("topk", queries)
    buf = torch.empty(3 * stride, dtype=torch.float32, device="cuda")
    base = torch.as_strided(buf, (3, N), (stride, 1))
    assert 2 * stride > 2 ** 32 and base.stride(0) == stride
    gen = torch.Generator(device="cuda")
    gen.manual_seed(65)
    want = []
    for b in range(3):
        base[b].normal_(generator=gen).mul_(0.1)
        top = torch.topk(base[b], 2001)
        floor = np.float32(0.3) * np.float32(top.values[-1].item())
        rows = np.union1d(fam.pos, top.indices[:2000].cpu().numpy())
        bvals = base[b][_dev(rows)].cpu().numpy()
        s = np.zeros(rows.size, dtype=np.float32)
        s[np.searchsorted(rows, fam.pos)] = S[b]
        v = ref.blend32(bvals, s, 0.3, 0.7)
        wv, wi = ref.ref_topk(v, k)
        want.append((wv, rows[wi]))
        assert wv[-1] > floor + np.float32(0) and np.isin(rows[wi], fam.pos).sum() >= 3, (b, wv, floor)
    got = fam.tt.lexical_score_topk(fam.t, F, _q(queries), k, base=base, w_base=0.3, w_lex=0.7)
    _assert_rows(got, want, "base")
    del buf, base


# ---- 3. N at the cap ------------------------------------------------------------------------------------------------------------
def test_n_at_the_cap(big):
    fam = big.get("cap")
    tt, N, k = fam.tt, fam.N, 10
    need = fam.lib.tt_lexical_workspace_bytes(1, N, k)
    assert need >= 12 * k * 725 * 724
    for b in (0, 1):
        with poison.poisoned_empty(0xFFFFFFFF) as p:
            got = tt.lexical_score_topk(fam.t, F, _q(fam.queries[b:b + 1]), k)
            torch.cuda.synchronize()
        assert p.tensors == 3 and p.bytes == need + k * 4 + k * 8      # the two outputs and a workspace of exactly that size
        want = sparse_topk(fam.pos, fam.S[b], N, k)
        _assert_rows(got, [want], f"query {b}")
    assert (fam.S[1] > 0).sum() == 4 and want[1].tolist() == fam.rare + [0, 1, 2, 3, 4, 5] and not want[0][4:].any()
    assert len({int(r) >> 12 for r in sparse_topk(fam.pos, fam.S[0], N, k)[1]}) >= 2


def test_score_all_at_the_cap_past_2_32_elements(big):
    """S [3, N]: b * N + r passes 2^32 elements in row 2 (25.8 GB)."""
    fam = big.get("cap")
    N = fam.N
    assert 2 * N > 2 ** 32 - 2 ** 20
    S = fam.tt.lexical_score_all(fam.t, F, _q(fam.queries))
    assert tuple(S.shape) == (3, N)
    assert nonzero_words(S) == int(np.count_nonzero(fam.S)) > 50
    assert np.array_equal(_bits(S[:, fam.pos_dev].cpu().numpy()), _bits(fam.S))
    assert fam.S[2][-10:].all() and (2 * N + fam.pos[-10:] > 2 ** 32).all()
