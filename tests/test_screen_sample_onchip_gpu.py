"""The shared-tile sample pass keeps its maxima in registers (csrc/screen.hip, ONCHIP): every lane keeps the STOP = 2 largest
maxima of the 8-document slices it sees and the seed is the k-th largest of the kept values.

What a seed has to be is unchanged: the approximate score of the k_seed-th of k_seed DISTINCT kept documents of the sample.
The approximate score of a pair is within eps_q = 1.10e-3 |q| Dmax + 1e-6 (|q| + Dmax) of its exact one (screen_eps), so
for every query at least k_seed sample rows (kept ones, under a mask) must have a float64 score >= seed - eps_q.  That
is checked for every query of every case; the searches are compared with equality against the CPU oracle (planted queries,
first and last row) and, for all rows, against the exact kernel, with no fallback flag raised.

The plantings (queries QA, QB; scores 2 .. 2.75 against < 1 for every other row):
  QA  STOP + 2 documents at the same slice position (row 5) of tiles 0 .. 3: one lane's stream wherever the first sample
      chunk has four tiles or more (asserted for the shapes where the plan gives it that many), so the lane keeps two of four
  QB  four documents in tile 8, rows 0, 4, 8, 12: four slices of one tile, which the per-tile maxima saw as one value
Masked cases drop exactly the planted rows: a seed vouched for by one of them exceeds every kept score."""
import numpy as np
import pytest
import torch

import synth
from test_masked_gpu import host_f32, rows_on_device
from test_search_aux_gpu import kth_largest, par_rows, sample_tiles, seed_calls

pytestmark = pytest.mark.gpu

STOP = 2
QA, QB = 3, 40
ROWS_A = [32 * t + 5 for t in range(STOP + 2)]
ROWS_B = [32 * 8 + 4 * g for g in range(4)]
BMAX = 1024
NS = (65_536, 300_000)   # 65 536: the smallest corpus with a sample pass
BS = (65, 200, 300, 600, 1024)   # nset 1, 2, 3, 3 x 2 groups, 4 x 2 groups
KS = ((1, 1), (10, 10), (10, 64), (64, 64))


@pytest.fixture(scope="module")
def tt():
    import twotowermlretrieval_amd as m
    from twotowermlretrieval_amd import _lib
    _lib.lib()
    assert torch.cuda.is_available()
    return m


@pytest.fixture(scope="module")
def L():
    from twotowermlretrieval_amd import _lib
    return _lib.lib()


@pytest.fixture(autouse=True)
def product_thresholds(monkeypatch):
    """The routing thresholds of the product (other test modules lower them for the rest of the session)."""
    from twotowermlretrieval_amd import index as _index
    monkeypatch.setattr(_index, "SCREEN_MIN_DOCS", 65536)
    monkeypatch.setattr(_index, "SCREEN_MIN_BATCH", 1)


def sample_chunk_tiles(N, B, k):
    """Tiles of one sample chunk (make_splan: a round of workgroups over the sample tiles, per query group)."""
    if B <= 256:
        per_group = 128 if B <= 128 else 256
    else:                                              # as few groups as 512-query groups need, of 384 where that holds them
        g512 = (B + 511) // 512
        per_group = 384 if (B + g512 - 1) // g512 <= 384 else 512
    groups = (B + per_group - 1) // per_group
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    want = max(1, min((cus + groups - 1) // groups, sample_tiles(N, k)))
    return (sample_tiles(N, k) + want - 1) // want


class Case:
    """One corpus (N rows, fp32 + shadow or bf16) with the plantings, its index, the planted-rows-dropped mask and the exact
    answers, each computed once and shared by the cases."""

    def __init__(self, tt, oracle, N, bf16):
        self.tt, self.oracle, self.N, self.bf16 = tt, oracle, N, bf16
        D = rows_on_device(4100 + N % 1000, N, 256, bf16)
        self.Qn = synth.unit_rows(4101, BMAX, 256)
        self.Q = torch.from_numpy(self.Qn).cuda()
        for q, rows in ((QA, ROWS_A), (QB, ROWS_B)):
            for j, r in enumerate(rows):
                D[r] = (self.Q[q] * (2.0 + 0.25 * j)).to(D.dtype)
        self.D, self.Dn = D, host_f32(D)
        self.ix = tt.BruteForceIndex(D, screen=True, screen_masked=True)
        self.ix.keep_stats = True
        assert self.ix._screen is not None and self.ix._screen.bf16 is bf16
        mask = np.ones(N, dtype=bool)
        mask[ROWS_A + ROWS_B] = False
        self.mask = {False: None, True: mask}
        self.keep = {False: None, True: tt.pack_keep_mask(torch.from_numpy(mask).cuda())}
        self.qnorm = np.linalg.norm(self.Qn.astype(np.float64), axis=1)
        self._oracle, self._exact, self._s64 = {}, {}, {}

    def eps(self, B):
        dmax = float(self.ix.dmax_norm)
        return 1.10e-3 * self.qnorm[:B] * dmax + 1e-6 * (self.qnorm[:B] + dmax)

    def sample_scores64(self, k, masked):
        """float64 scores of every query against the sample rows of a search for k (dropped rows: -inf), on the device."""
        s_docs = 32 * sample_tiles(self.N, k)
        if (s_docs, masked) not in self._s64:
            S = self.Q.double() @ self.D[:s_docs].double().T
            if masked:
                S[:, torch.from_numpy(~self.mask[True][:s_docs]).cuda()] = -float("inf")
            self._s64[(s_docs, masked)] = S
        return self._s64[(s_docs, masked)]

    def assert_valid(self, seed, B, k, k_seed, masked, what):
        """At least k_seed (kept) sample rows reach seed - eps_q in float64, for every query."""
        S = self.sample_scores64(k, masked)[:B]
        bound = torch.from_numpy(seed.astype(np.float64) - self.eps(B)).cuda()
        n = (S >= bound[:, None]).sum(dim=1).cpu().numpy()
        print(f"{what}: rows reaching seed - eps: min {int(n.min())} (need {k_seed}), finite seeds {int(np.isfinite(seed).sum())}/{B}")
        assert np.isfinite(seed).all(), what
        assert (n >= k_seed).all(), (what, np.flatnonzero(n < k_seed)[:8], n.min())

    def oracle_rows(self, rows, masked):
        """oracle top-64 of single queries over the kept rows, indices mapped back; kept per (query, masked)."""
        kept = np.flatnonzero(self.mask[True]) if masked else np.arange(self.N)
        todo = np.array(sorted(r for r in set(rows) if (r, masked) not in self._oracle), dtype=np.int64)
        if len(todo):
            Dk = np.ascontiguousarray(self.Dn[kept])
            v, i = par_rows(lambda q: self.oracle.score_topk(q, Dk, 64), self.Qn[todo])
            for n, r in enumerate(todo):
                self._oracle[(int(r), masked)] = (v[n], kept[i[n]])
        return (np.stack([self._oracle[(r, masked)][0] for r in rows]), np.stack([self._oracle[(r, masked)][1] for r in rows]))

    def exact(self, B, k, masked):
        """The exact kernel's answer for every row."""
        if (B, k, masked) not in self._exact:
            v, i = self.tt.score_topk(self.Q[:B], self.D, k, keep=self.keep[masked])
            torch.cuda.synchronize()
            self._exact[(B, k, masked)] = (v.cpu().numpy(), i.cpu().numpy())
        return self._exact[(B, k, masked)]

    def seed_list(self, B, k, k_seed, masked):
        sc = self.ix._screen
        ws = torch.empty(sc.workspace_bytes(B, k, masked), dtype=torch.uint8, device="cuda")
        flags = torch.full(((B + 31) // 32,), 7, dtype=torch.int32, device="cuda")
        lst = sc.seed_list(self.Q[:B], k, k_seed, flags, ws, self.keep[masked])
        torch.cuda.synchronize()
        return lst.cpu().numpy(), flags, ws

    def seeded(self, B, k, seed, flags, ws, masked):
        v = torch.empty((B, k), dtype=torch.float32, device="cuda")
        i = torch.empty((B, k), dtype=torch.int64, device="cuda")
        self.ix._screen.run(self.Q[:B], k, 0, v, i, flags, ws, torch.from_numpy(seed).cuda(), None, self.keep[masked])
        torch.cuda.synchronize()
        return v.cpu().numpy(), i.cpu().numpy(), flags.cpu().numpy()


@pytest.fixture(scope="module")
def cases(tt, oracle):
    made = {}

    def get(N, bf16):
        if (N, bf16) not in made:
            made[(N, bf16)] = Case(tt, oracle, N, bf16)
        return made[(N, bf16)]

    yield get
    made.clear()
    torch.cuda.empty_cache()


@pytest.mark.parametrize("masked", (False, True))
@pytest.mark.parametrize("k_seed,k", KS)
@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("bf16", (False, True))
@pytest.mark.parametrize("N", NS)
def test_seed_is_valid_and_the_search_exact(L, cases, N, bf16, B, k_seed, k, masked):
    c = cases(N, bf16)
    tpc = sample_chunk_tiles(N, B, k)
    print(f"sample: {sample_tiles(N, k)} tiles, {tpc} per chunk; QA's rows in one stream: {tpc >= len(ROWS_A)}")
    if N == 300_000 and k >= 10:
        assert tpc >= len(ROWS_A)                      # the adversarial stream is real at these shapes
    # seed list -> seed: the k_seed-th largest kept value
    lst, flags, ws = c.seed_list(B, k, k_seed, masked)
    seed = kth_largest(lst, k_seed)
    assert (lst >= seed[:, None]).all()
    c.assert_valid(seed, B, k, k_seed, masked, "seed_list")
    planted = (lst[[QA, QB]] >= 1.5).sum(axis=1)       # (every other score is below 1)
    if masked:                                         # no dropped document vouches
        assert planted.tolist() == [0, 0] and seed[QA] < 1.0 and seed[QB] < 1.0
    elif k_seed >= len(ROWS_A):
        # QA: a lane keeps STOP of the planted rows its chunk holds; QB: four slices of one tile are four documents
        in_chunk = np.bincount(np.arange(len(ROWS_A)) // tpc)
        assert planted.tolist() == [int(np.minimum(in_chunk, STOP).sum()), len(ROWS_B)]
    else:
        assert seed[QA] >= 2.7 and seed[QB] >= 2.7     # k_seed = 1: the best planted row (2.75)
    if not bf16 and not masked:                        # the threshold entry point of the same pass
        thr, _, _ = seed_calls(L, c.ix, c.Q[:B], k, k_seed)
        torch.cuda.synchronize()
        thr = thr.cpu().numpy()
        c.assert_valid(thr, B, k, k_seed, masked, "seed")
        assert np.array_equal(thr, seed)
    # the seeded search under that seed: the exact top-k_seed, no fallback
    v, i, fl = c.seeded(B, k, seed, flags, ws, masked)
    assert not fl.any(), "the exact fallback ran"
    ev, ei = c.exact(B, k, masked)
    assert np.array_equal(i[:, :k_seed], ei[:, :k_seed]) and np.array_equal(v[:, :k_seed], ev[:, :k_seed])
    rows = [0, QA, QB, B - 1]
    ov, oi = c.oracle_rows(rows, masked)
    assert np.array_equal(i[rows, :k_seed], oi[:, :k_seed]) and np.array_equal(v[rows, :k_seed], ov[:, :k_seed])
    # the whole search through the index
    got = c.ix.search(c.Q[:B], k, keep=c.keep[masked])
    torch.cuda.synchronize()
    assert int(c.ix.fallback_flags.ne(0).sum()) == 0
    assert np.array_equal(got[1].cpu().numpy(), ei) and np.array_equal(got[0].cpu().numpy(), ev)
    assert np.array_equal(got[1].cpu().numpy()[rows], oi[:, :k]) and np.array_equal(got[0].cpu().numpy()[rows], ov[:, :k])
    if not masked:
        assert got[1][QA, :len(ROWS_A)].tolist() == ROWS_A[::-1][:k]   # (the last planted row scores highest)
        assert got[1][QB, :len(ROWS_B)].tolist() == ROWS_B[::-1][:k]


def searched(ix, Q, k):
    v, i = ix.search(Q, k)
    torch.cuda.synchronize()
    st = ix.search_stats().cpu().numpy()
    return v.cpu().numpy(), i.cpu().numpy(), int(ix.fallback_flags.ne(0).sum()), st


@pytest.mark.parametrize("bf16", (False, True))
@pytest.mark.parametrize("B,k", [(65, 10), (300, 64), (1024, 10)])
def test_both_forms_return_the_same_top_k(cases, bf16, B, k):
    """The comparison build with TT_SCREEN_SAMPLE_ONCHIP=0 runs the per-tile sample pass this form replaced; same answer."""
    from conftest import ab_library
    c = cases(300_000, bf16)
    v, i, fl, st = searched(c.ix, c.Q[:B], k)
    with ab_library(TT_SCREEN_SAMPLE_ONCHIP=0):
        ov, oi, ofl, ost = searched(c.ix, c.Q[:B], k)
    with ab_library(TT_SCREEN_SAMPLE_ONCHIP=1):
        av, ai, afl, ast = searched(c.ix, c.Q[:B], k)
    print(f"pooled per query: kept maxima {st[:, 0].mean():.2f}, per-tile maxima {ost[:, 0].mean():.2f}")
    assert fl == 0 and ofl == 0 and afl == 0
    assert np.array_equal(i, oi) and np.array_equal(v, ov)
    assert np.array_equal(i, ai) and np.array_equal(v, av)
    assert (st[:, 1] >= k).all() and (ost[:, 1] >= k).all()


def test_pooled_candidates_do_not_grow_at_1m(tt):
    """N = 1M random unit rows, B = 1024, k = 10: the kept maxima must seed at least as well as the per-tile maxima did.  The
    pooled candidates per query (search_stats) move from run to run with the tail pool's block assignment, so the new mean may
    exceed the old path's by no more than two runs of the old path differ.  Same final top-k from both."""
    from conftest import ab_library
    N, B, k = 1_000_000, 1024, 10
    g = torch.Generator(device="cuda").manual_seed(11)
    D = torch.randn((N, 256), device="cuda", generator=g)
    D /= D.norm(dim=1, keepdim=True)
    Q = torch.randn((B, 256), device="cuda", generator=g)
    Q /= Q.norm(dim=1, keepdim=True)
    ix = tt.BruteForceIndex(D, screen=True)
    ix.keep_stats = True
    with ab_library(TT_SCREEN_SAMPLE_ONCHIP=0):
        old = [searched(ix, Q, k) for _ in range(2)]
    new = searched(ix, Q, k)
    m_old = [o[3][:, 0].mean() for o in old]
    m_new = new[3][:, 0].mean()
    print(f"mean pooled candidates per query: per-tile maxima {m_old[0]:.3f}, {m_old[1]:.3f}; kept maxima (T = {STOP}) {m_new:.3f}")
    assert new[2] == 0 and old[0][2] == 0 and old[1][2] == 0
    for o in old:
        assert np.array_equal(new[1], o[1]) and np.array_equal(new[0], o[0])
    assert m_new <= np.mean(m_old) + abs(m_old[0] - m_old[1])
