"""Cursor search (tt_score_topk_after_f32 / _bf16, score_topk_after, the indexes' search_after / pages / deep_search,
mine_hard_negatives): the next k results after a (score, id) position, in one exact top-k pass.

Query b sees document n (global id g) iff its score s lies strictly after the cursor (a_b, i_b) in (score desc, index asc):
s < a_b or (s == a_b and g > i_b).  The expected value is built from the GPU's own score_all (unchanged by this feature; bf16
rows widened to f32, which is exact): the rule, then torch.sort(descending=True, stable=True).  For four queries of every case
it is also cursor_ref over the CPU oracle, and what the MASKED call returns for the query alone under a keep-bitmask of its
eligibility -- the contract's own sentence.  Values and indices are compared with equality, never a tolerance."""
import numpy as np
import pytest
import torch

import cursor_ref
import synth
from poison import PATTERNS, pattern_id, poisoned_empty

pytestmark = pytest.mark.gpu

INF = float("inf")
I64_MAX, I64_MIN = cursor_ref.I64_MAX, cursor_ref.I64_MIN
BIG_OFF = 2 ** 33 + 5
PATTERN_NAMES = ("open", "page2", "deep", "tie_mid", "mixed", "closed", "last_one", "id_extremes")


@pytest.fixture(scope="module")
def tt():
    import twotowermlretrieval_amd as m
    from twotowermlretrieval_amd import _lib
    _lib.lib()
    assert torch.cuda.is_available()
    return m


def rows_on_device(seed, n, d, bf16=False):
    g = torch.Generator(device="cuda").manual_seed(seed)
    D = torch.randn((n, d), device="cuda", generator=g).div_(d ** 0.5)
    return D.to(torch.bfloat16) if bf16 else D


def queries(seed, B, d):
    return torch.from_numpy(synth.unit_rows(seed, B, d)).cuda()


def f32(x, B=None):
    t = torch.as_tensor(x, dtype=torch.float32, device="cuda")
    return t.expand(B).contiguous() if B is not None and t.dim() == 0 else t


def i64(x, B=None):
    t = torch.as_tensor(x, dtype=torch.int64, device="cuda")
    return t.expand(B).contiguous() if B is not None and t.dim() == 0 else t


def eligible(S, av, ai, off=0, keep_bool=None):
    """bool [B,N]: the rule on the GPU's scores."""
    g = torch.arange(S.shape[1], device=S.device, dtype=torch.int64) + off
    e = (S < av[:, None]) | ((S == av[:, None]) & (g[None, :] > ai[:, None]))
    return e if keep_bool is None else e & keep_bool[None, :]


def expected(S, elig, k, off=0):
    """The rule's result from scores S [B,N] and eligibility: a stable descending sort of the eligible scores."""
    B, N = S.shape
    vals = torch.full((B, k), -INF, dtype=torch.float32, device=S.device)
    idx = torch.full((B, k), -1, dtype=torch.int64, device=S.device)
    if N == 0:
        return vals, idx
    sv, si = torch.sort(torch.where(elig, S, torch.full_like(S, -INF)), dim=1, descending=True, stable=True)
    m = min(k, N)
    sv, si = sv[:, :m], si[:, :m]
    ok = torch.gather(elig, 1, si)                          # (an ineligible -inf must not count as a result)
    ok &= torch.cumsum((~ok).to(torch.int32), 1) == 0       # (nor an eligible one behind it: cannot happen with finite scores)
    vals[:, :m] = torch.where(ok, sv, vals[:, :m])
    idx[:, :m] = torch.where(ok, si + off, idx[:, :m])
    return vals, idx


def assert_same(got, want, what=""):
    assert torch.equal(got[1], want[1]) and torch.equal(got[0], want[0]), what


def four(B):
    return np.unique(np.linspace(0, B - 1, min(B, 4)).astype(int))


def tie_positions(N, seed):
    """Up to 70 rows for the copies of one row: both lane halves of a tile (offsets +0 and +4), tile ends and starts
    (32 t - 1, 32 t for t = 1..26 -- the main pass cuts the corpus into chunks of c whole tiles counted from tile 0, and
    c <= 23 at every shape of this grid on a chip of 256 compute units: 9376 tiles over 2048 / 5 chunks at B = 130 is the
    longest -- so the pair at t = c is a chunk's last and the next chunk's first tile), row 0 and row N - 1, and seeded random
    rows for the rest."""
    want = [0, 4, N - 1, N - 5, 36, 100, 104]
    for t in range(1, 27):
        want += [32 * t - 1, 32 * t]
    want = sorted({p for p in want if 0 <= p < N})
    rest = [p for p in np.random.RandomState(seed).permutation(N).tolist() if p not in set(want)]
    return np.array(sorted(want + rest[:max(0, min(70, N) - len(want))]), dtype=np.int64)


class Case:
    """One (corpus, queries) of the grid with what every pattern needs: scores, the sorted rows, a plain search."""

    def __init__(self, tt, D, Q, k):
        self.D, self.Q, self.k = D, Q, k
        self.B, self.N = Q.shape[0], D.shape[0]
        self.S = tt.score_all(Q, D.float() if D.dtype == torch.bfloat16 else D)
        self.sorted, self.order = torch.sort(self.S, dim=1, descending=True, stable=True)
        self.plain = tt.score_topk(Q, D, k)

    def at_rank(self, r):
        return self.sorted[:, r].contiguous(), self.order[:, r].contiguous()


def cursors(case, name, tie_ids=None):
    """(after_val [B], after_idx [B], idx_offset) of one pattern."""
    B, N, k = case.B, case.N, case.k
    deep_rank = max(0, min(5000, N - 2))
    if name == "open":
        return f32(INF, B), i64(-1, B), 0
    if name == "page2":                                     # each query's own k-th result (the tail when N < k: closed)
        return case.plain[0][:, -1].contiguous(), case.plain[1][:, -1].contiguous(), 0
    if name == "deep":
        return (*case.at_rank(deep_rank), 0)
    if name == "tie_mid":                                   # the run's middle id (the 35th of 70), at each query's score of it
        mid = int(tie_ids[(len(tie_ids) - 1) // 2])
        return case.S[:, mid].contiguous(), i64(mid, B), 0
    if name == "mixed":                                     # side by side within a 32-query tile
        dv, di = case.at_rank(deep_rank)
        lane = torch.arange(B, device="cuda") % 4
        av = torch.where(lane == 0, f32(INF, B), torch.where(lane == 1, dv, torch.where(lane == 2, f32(-INF, B), f32(float("nan"), B))))
        ai = torch.where(lane == 1, di, i64(-1, B))
        return av, ai, 0
    if name == "closed":
        return f32(-INF, B), i64(-1, B), 0
    if name == "last_one":                                  # the second-to-last document of the order (N = 1: nothing before it)
        return (*case.at_rank(N - 2), 0) if N >= 2 else (f32(INF, B), i64(-1, B), 0)
    if name == "id_extremes":                               # an existing score; ties excluded (even b) or included (odd b)
        av, _ = case.at_rank(min(3, N - 1))
        ai = torch.where(torch.arange(B, device="cuda") % 2 == 0, i64(I64_MAX, B), i64(I64_MIN, B))
        return av, ai, BIG_OFF
    raise KeyError(name)


# (dtype, d) over the support matrix x B: the 16-query tile, the 32-query tile, two tiles, paced + pooled; N and k rotate
WIDTHS = [(False, 32), (False, 256), (False, 320), (False, 512), (True, 64), (True, 256)]
BS = (1, 16, 17, 33, 130)
NS = (1, 31, 1000, 65_537, 300_001)
KS = (1, 10, 64)
CASES = [(bf, d, B, NS[(a + 2 * b) % len(NS)], KS[(a + b) % len(KS)]) for a, (bf, d) in enumerate(WIDTHS) for b, B in enumerate(BS)]


@pytest.mark.parametrize("bf16,d,B,N,k", CASES)
def test_cursor_patterns(tt, oracle, bf16, d, B, N, k):
    D = rows_on_device(100 + d + N, N, d, bf16)
    Q = queries(200 + B + d, B, d)
    # tie_mid has a corpus of its own: one row copied to (up to) 70 positions, query 0 is that row
    ties = tie_positions(N, d + B)
    Dt, Qt = D.clone(), Q.clone()
    row = Dt[int(ties[0])].float()                           # (norm 2: the copies outscore every other row for query 0)
    Dt[torch.from_numpy(ties).cuda()] = (row / row.norm() * 2.0).to(Dt.dtype)
    Qt[0] = Dt[int(ties[0])].float()
    plain_case, tie_case = Case(tt, D, Q, k), Case(tt, Dt, Qt, k)
    rows = four(B)
    Qn = {False: Q.cpu().numpy(), True: Qt.cpu().numpy()}
    Dn = {False: D.float().cpu().numpy(), True: Dt.float().cpu().numpy()}
    So = {t: oracle.score_all(np.ascontiguousarray(Qn[t][rows]), Dn[t]) for t in (False, True)}   # once per corpus
    for name in PATTERN_NAMES:
        tie = name == "tie_mid"
        case = tie_case if tie else plain_case
        av, ai, off = cursors(case, name, ties)
        got = tt.score_topk_after(case.Q, case.D, av, ai, k, idx_offset=off)
        elig = eligible(case.S, av, ai, off)
        want = expected(case.S, elig, k, off)
        torch.cuda.synchronize()
        bad = int((got[1] != want[1]).sum()), int((got[0] != want[0]).sum())
        print(f"cursor {name}: index mismatches {bad[0]}, value mismatches {bad[1]}, results {int((got[1] >= 0).sum())}")
        assert_same(got, want, name)
        if name == "open":                                   # the unmasked call, bit for bit
            assert_same(got, case.plain, name)
        if name == "closed":
            assert bool((got[1] == -1).all()) and bool(torch.isneginf(got[0]).all())
        if name == "mixed":
            assert torch.equal(got[1][0], case.plain[1][0]) and torch.equal(got[0][0], case.plain[0][0])
            for b in range(2, B, 4):
                assert bool((got[1][b:b + 2] == -1).all())   # the closed and the NaN cursor of every group of four
        if name == "last_one" and N >= 2:
            assert torch.equal(got[1][:, 0], case.order[:, N - 1]) and bool((got[1][:, 1:] == -1).all())
        if name == "deep" and N > 5001 + k:
            assert torch.equal(got[1], case.order[:, 5001:5001 + k]) and torch.equal(got[0], case.sorted[:, 5001:5001 + k])
        if name == "tie_mid":                                # the remaining copies come first, ids ascending
            rest = ties[(len(ties) - 1) // 2 + 1:][:k]
            assert got[1][0, :len(rest)].tolist() == rest.tolist()
            assert bool((got[0][0, :len(rest)] == case.S[0, int(ties[0])]).all())
        if name == "id_extremes" and N >= 4:
            r = min(3, N - 1)
            assert bool((got[0][0::2] < case.sorted[0::2, r:r + 1]).all())                 # INT64_MAX: no tie is eligible
            if B > 1:
                assert torch.equal(got[0][1::2, 0], case.sorted[1::2, r])                  # INT64_MIN: every tie is
        # four queries: the CPU oracle through the numpy reference, and the masked call under the query's own eligibility
        avn, ain = av.cpu().numpy(), ai.cpu().numpy()
        ov, oi = cursor_ref.search_after(So[tie], avn[rows], ain[rows], k, off)
        assert np.array_equal(got[1].cpu().numpy()[rows], oi) and np.array_equal(got[0].cpu().numpy()[rows], ov, equal_nan=False), name
        for b in rows:
            mv, mi = tt.score_topk(case.Q[b], case.D, k, off, keep=tt.pack_keep_mask(elig[b]))
            assert torch.equal(mi, got[1][b]) and torch.equal(mv, got[0][b]), (name, int(b))


@pytest.fixture(scope="module")
def dup_index(tt):
    """N = 1000 with duplicate rows (runs of ties), two query tiles: shared by the paging tests below."""
    N, d, B = 1000, 256, 40
    D = rows_on_device(7, N, d)
    rs = np.random.RandomState(8)
    D[torch.from_numpy(rs.randint(1, N, size=300)).cuda()] = D[0].clone()
    D[torch.from_numpy(rs.randint(0, N - 1, size=100)).cuda()] = D[N - 1].clone()
    Q = queries(9, B, d)
    Q[0] = D[0]
    S = tt.score_all(Q, D)
    return D, Q, torch.sort(S, dim=1, descending=True, stable=True)


@pytest.mark.parametrize("k", [64, 7])
def test_pages_until_the_tail_are_the_stable_sort(tt, dup_index, k):
    D, Q, (sv, si) = dup_index
    N = D.shape[0]
    ix = tt.BruteForceIndex(D, idx_offset=11)
    n_pages = N // k + 1                                     # the last one ends in the tail
    got = list(ix.pages(Q, k, n_pages=n_pages))
    assert len(got) == n_pages
    vals, idx = torch.cat([v for v, _ in got], 1), torch.cat([i for _, i in got], 1)
    torch.cuda.synchronize()
    assert torch.equal(idx[:, :N], si + 11) and torch.equal(vals[:, :N], sv)
    assert bool((idx[:, N:] == -1).all()) and bool(torch.isneginf(vals[:, N:]).all())
    gen = ix.pages(Q[0], k)                                  # a single query; the caller stops an open-ended generator
    v0, i0 = next(gen)
    v1, i1 = next(gen)
    assert v0.shape == (k,) and torch.equal(torch.cat([i0, i1]), si[0, :2 * k] + 11)


def test_sixteen_pages_are_search_1024_and_deep_search_goes_on(tt):
    N, d, B = 300_001, 256, 33
    D = rows_on_device(21, N, d)
    Q = queries(22, B, d)
    ix = tt.BruteForceIndex(D)
    got = list(ix.pages(Q, 64, n_pages=16))
    want = ix.search(Q, 1024)
    assert_same((torch.cat([v for v, _ in got], 1), torch.cat([i for _, i in got], 1)), want)
    sv, si = torch.sort(tt.score_all(Q, D), dim=1, descending=True, stable=True)
    deep = ix.deep_search(Q, 2000)
    assert deep[0].shape == (B, 2000)
    assert_same(deep, (sv[:, :2000], si[:, :2000]))
    one = ix.deep_search(Q[5], 70)
    assert one[0].shape == (70,) and torch.equal(one[1], si[5, :70])
    with pytest.raises(Exception, match="1024"):
        ix.search(Q, 1025)                                   # search() keeps its bound


@pytest.mark.parametrize("bf16,d,B", [(False, 256, 40), (False, 384, 5), (True, 128, 130)])
def test_keep_and_remove_ids_compose(tt, bf16, d, B):
    N, k, off = 70_001, 10, 1000
    D = rows_on_device(31 + d, N, d, bf16)
    Q = queries(32 + d, B, d)
    S = tt.score_all(Q, D.float())
    sv, si = torch.sort(S, dim=1, descending=True, stable=True)
    av, ai = sv[:, 20].contiguous(), si[:, 20].contiguous() + off
    half = torch.from_numpy(np.random.RandomState(d).rand(N) < 0.5).cuda()
    got = tt.score_topk_after(Q, D, av, ai, k, idx_offset=off, keep=tt.pack_keep_mask(half))
    assert_same(got, expected(S, eligible(S, av, ai, off, half), k, off))
    assert bool(half[(got[1] - off).flatten()].all())
    ix = tt.BruteForceIndex(D, idx_offset=off)
    gone = (si[:, 21:24] + off).flatten()
    ix.remove_ids(gone)
    kept = torch.ones(N, dtype=torch.bool, device="cuda")
    kept[gone - off] = False
    assert_same(ix.search_after(Q, k, (av, ai)), expected(S, eligible(S, av, ai, off, kept), k, off))
    assert_same(ix.search_after(Q, k, (av, ai), keep=tt.pack_keep_mask(half)), expected(S, eligible(S, av, ai, off, kept & half), k, off))
    none = torch.zeros(N, dtype=torch.bool, device="cuda")
    got = ix.search_after(Q, k, (av, ai), keep=tt.pack_keep_mask(none))
    assert bool((got[1] == -1).all()) and bool(torch.isneginf(got[0]).all())


def test_null_cursor_is_the_masked_call(tt):
    from twotowermlretrieval_amd import _lib
    L = _lib.lib()
    B, N, d, k = 40, 5000, 128, 10
    D, Q = rows_on_device(1, N, d), queries(2, B, d)
    keep = tt.pack_keep_mask(torch.from_numpy(np.random.RandomState(1).rand(N) < 0.5).cuda())
    want = tt.score_topk(Q, D, k, keep=keep)
    v = torch.empty((B, k), device="cuda")
    i = torch.empty((B, k), dtype=torch.int64, device="cuda")
    ws = torch.empty(L.tt_score_topk_after_workspace_bytes(B, N, d, k, 0), dtype=torch.uint8, device="cuda")
    _lib.check(L.tt_score_topk_after_f32(Q.data_ptr(), B, d, D.data_ptr(), N, None, None, keep.data_ptr(), k, 0,
                                         v.data_ptr(), i.data_ptr(), ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert torch.equal(i, want[1]) and torch.equal(v, want[0])
    assert_same(tt.score_topk_after(Q, D, INF, -1, k, keep=keep), want)     # and so is the open cursor


@pytest.mark.parametrize("word", PATTERNS[1:], ids=pattern_id)
@pytest.mark.parametrize("bf16,d,B,N", [(False, 256, 130, 300_001), (False, 512, 5, 65_537), (True, 64, 33, 1000)])
def test_results_do_not_depend_on_what_the_buffers_held(tt, word, bf16, d, B, N):
    """Paced + pooled with a sample pass, the 16-query kernel, a bf16 tile: every workspace and output from a poisoned
    torch.empty gives the bits of the clean run."""
    k = 10
    D = rows_on_device(41 + d, N, d, bf16)
    Q = queries(42 + d, B, d)
    pv, pi = tt.score_topk(Q, D, k)
    args = (Q, D, pv[:, -1].contiguous(), pi[:, -1].contiguous(), k)
    clean = tt.score_topk_after(*args)
    with poisoned_empty(word) as p:
        got = tt.score_topk_after(*args)
    torch.cuda.synchronize()
    assert p.tensors >= 3                                    # values, indices, workspace
    assert_same(got, clean)
    assert not bool((got[1] == pi[:, -1:]).any()) and bool((got[0][:, 0] <= pv[:, -1]).all())


def test_graph_replay_walks_the_pages(tt):
    """One score_topk_after call with static tensors captured in a graph (a single stream: a linear capture).  Between the
    replays the output's last column is copied into the cursor buffers on the device: five replays are five pages."""
    N, d, B, k = 5000, 256, 40, 10
    D, Q = rows_on_device(17, N, d), queries(18, B, d)
    sv, si = torch.sort(tt.score_all(Q, D), dim=1, descending=True, stable=True)
    av, ai = f32(INF, B), i64(-1, B)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                            # warm-up outside capture: kernels loaded, blocks cached
        tt.score_topk_after(Q, D, av, ai, k)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = tt.score_topk_after(Q, D, av, ai, k)
    for page in range(5):
        graph.replay()
        torch.cuda.synchronize()
        assert_same(out, (sv[:, page * k:(page + 1) * k], si[:, page * k:(page + 1) * k]), f"page {page}")
        av.copy_(out[0][:, -1])
        ai.copy_(out[1][:, -1])


def test_exclude_with_k_plus_e_of_64(tt):
    N, d, B, k, E = 20_000, 256, 33, 40, 24
    D, Q = rows_on_device(51, N, d), queries(52, B, d)
    S = tt.score_all(Q, D)
    sv, si = torch.sort(S, dim=1, descending=True, stable=True)
    av, ai = sv[:, 100].contiguous(), si[:, 100].contiguous()
    excl = si[:, 101:101 + 2 * E:2].contiguous()            # every second result of the page, E of them
    excl[:, -1] = -1                                         # padding
    ix = tt.BruteForceIndex(D)
    got = ix.search_after(Q, k, (av, ai), exclude=excl)
    elig = eligible(S, av, ai)
    listed = excl >= 0
    elig[torch.arange(B, device="cuda")[:, None].expand_as(excl)[listed], excl[listed]] = False
    assert_same(got, expected(S, elig, k))
    v1, i1 = ix.search_after(Q[3], k, (av[3], ai[3]), exclude=excl[3])
    assert torch.equal(i1, got[1][3]) and torch.equal(v1, got[0][3])
    with pytest.raises(ValueError, match="k \\+ E = 65"):
        ix.search_after(Q, k + 1, (av, ai), exclude=excl)
    with pytest.raises(ValueError, match="k = 65"):
        ix.search_after(Q, 65, (av, ai))


def test_three_indexes_screened_and_bf16_resident(tt, oracle):
    """BruteForceIndex (screen=False / True, fp32 and bf16-resident), StreamedIndex and a one-rank ShardedIndex give the
    reference's bits under one cursor."""
    N, d, k, off, B = 70_000, 256, 10, 1000, 40
    Db = rows_on_device(61, N, d, bf16=True)
    D = Db.float()                                           # fp32 rows on the bf16 grid: every index scores the same values
    Q = queries(62, B, d)
    S = tt.score_all(Q, D)
    sv, si = torch.sort(S, dim=1, descending=True, stable=True)
    av, ai = sv[:, 1500].contiguous(), si[:, 1500].contiguous() + off
    want = expected(S, eligible(S, av, ai, off), k, off)
    assert torch.equal(want[1], si[:, 1501:1501 + k] + off)
    rows = four(B)
    ov, oi = cursor_ref.expected(oracle, Q.cpu().numpy(), D.cpu().numpy(), av.cpu().numpy(), ai.cpu().numpy(), k, rows, off)
    assert np.array_equal(want[1].cpu().numpy()[rows], oi) and np.array_equal(want[0].cpu().numpy()[rows], ov)
    for screen in (False, True):
        ix = tt.BruteForceIndex(D, idx_offset=off, screen=screen)
        assert_same(ix.search_after(Q, k, (av, ai)), want)
        if screen:
            assert ix._screens(B, k) and int(ix.fallback_flags.ne(0).sum()) == ix.fallback_flags.numel() == 2
        assert_same(ix.search_after(Q, k), ix.search(Q, k))  # after=None: the open cursor
        out = (torch.empty((B, k), device="cuda"), torch.empty((B, k), dtype=torch.int64, device="cuda"))
        assert ix.search_after(Q, k, (av, ai), out=out) is out
        assert_same(out, want)
        v1, i1 = ix.search_after(Q[4], k, (float(av[4]), int(ai[4])))                       # 1-D q, Python numbers
        assert v1.shape == (k,) and torch.equal(i1, want[1][4]) and torch.equal(v1, want[0][4])
    assert_same(tt.BruteForceIndex(Db, idx_offset=off).search_after(Q, k, (av, ai)), want)  # bf16-resident
    st = tt.StreamedIndex(Db.cpu(), block_docs=16_384, idx_offset=off)                      # five blocks
    assert (N + st.block - 1) // st.block >= 3
    assert_same(st.search_after(Q, k, (av, ai)), want)
    assert_same(st.deep_search(Q[:3], 100), (sv[:3, :100], si[:3, :100] + off))
    sh = tt.ShardedIndex(D, off, shard_k=50)                                                # one rank: the collective's route
    assert_same(sh.search_after(Q, k, (av, ai)), want)
    pages = list(sh.pages(Q, 64, n_pages=2))
    assert_same((torch.cat([p[0] for p in pages], 1), torch.cat([p[1] for p in pages], 1)), (sv[:, :128], si[:, :128] + off))
    with pytest.raises(ValueError, match="shard_k"):
        tt.ShardedIndex(D, off, shard_k=100).search_after(Q, k, (av, ai))


def test_mine_hard_negatives(tt):
    N, d, B, P, k, off = 4096, 256, 17, 3, 10, 50
    D, Q = rows_on_device(71, N, d), queries(72, B, d)
    S = tt.score_all(Q, D)
    sv, si = torch.sort(S, dim=1, descending=True, stable=True)
    pos = (si[:, [2, 5, 9]] + off).contiguous()              # three positives among the best ten
    pos[1, 2] = -1                                           # padding
    pos[2] = -1                                              # a query without positives
    pos[3, 1] = si[3, 60] + off                              # a positive far below the others: it sets the ceiling
    pos[4, 0] = off + N + 7                                  # not this index's: no score, not a valid positive
    Sn, posn = S.cpu().numpy(), pos.cpu().numpy()
    indexes = {"brute": tt.BruteForceIndex(D, idx_offset=off),
               "streamed": tt.StreamedIndex(D.to(torch.bfloat16).cpu(), block_docs=1024, idx_offset=off),
               "sharded": tt.ShardedIndex(D, off, shard_k=20)}
    Sb = tt.score_all(Q, D.to(torch.bfloat16).float()).cpu().numpy()                        # the streamed index's rows are bf16
    for margin, ratio in ((0.0, None), (0.05, None), (0.0, 0.9)):
        for name, ix in indexes.items():
            Sx = Sb if name == "streamed" else Sn
            (wv, wi), c = cursor_ref.mine(Sx, posn, k, margin, ratio, off)
            v, i = tt.mine_hard_negatives(ix, Q, pos, k, margin=margin, ratio=ratio)
            v, i = v.cpu().numpy(), i.cpu().numpy()
            assert np.array_equal(i, wi) and np.array_equal(v, wv), (name, margin, ratio)
            for b in range(B):
                real = i[b] >= 0
                assert not np.isin(i[b][real], posn[b]).any() and (v[b][real] <= c[b]).all()
            plain = ix.search(Q[2:3], k)
            assert np.array_equal(i[2], plain[1][0].cpu().numpy()) and np.array_equal(v[2], plain[0][0].cpu().numpy())
            if name == "brute":
                assert (v[3] <= Sn[3, posn[3, 1] - off]).all() and int(posn[3, 0]) not in i[3]
    ix = indexes["brute"]
    v1, i1 = tt.mine_hard_negatives(ix, Q[0], pos[0], k, margin=0.05)
    (wv, wi), _ = cursor_ref.mine(Sn[:1], posn[:1], k, 0.05, None, off)
    assert i1.shape == (k,) and np.array_equal(i1.cpu().numpy(), wi[0]) and np.array_equal(v1.cpu().numpy(), wv[0])
    with pytest.raises(ValueError, match="k \\+ E"):
        tt.mine_hard_negatives(ix, Q, pos, 62)
