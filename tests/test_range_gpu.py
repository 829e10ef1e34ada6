"""Threshold search on the GPU: the counting pass (tt_score_count_f32 / _bf16, score_count), the cut (tt_topk_cut_below) and
count / range_search of the indexes.

The count must agree bit for bit with the scores the searches return, so nothing here has a tolerance.  The expected count of
EVERY query is (S >= t) & kept summed per row over S = tt.score_all (contract-tested against the oracle, the same fp32 chain;
bf16 rows widened, which is exact), and for 4 spread queries S is the CPU oracle's own score_all.  Thresholds are taken from S
itself, so that documents sit exactly at the threshold: a kernel whose chain, comparison or mask differs in one bit for one
document miscounts."""
import numpy as np
import pytest
import torch

from test_masked_gpu import BS, NS, WIDTHS, host_f32, masks_for, queries, rows_on_device

pytestmark = pytest.mark.gpu

INF = float("inf")


@pytest.fixture(scope="module")
def tt():
    import twotowermlretrieval_amd as m
    from twotowermlretrieval_amd import _lib
    _lib.lib()
    assert torch.cuda.is_available()
    return m


def all_scores(tt, Q, D):
    return tt.score_all(Q, D.float() if D.dtype == torch.bfloat16 else D)


def want_counts(S, t, mask_t=None):
    hit = S >= t[:, None]
    if mask_t is not None:
        hit = hit & mask_t[None, :]
    return hit.sum(1)


def spread(B, n=4):
    return np.unique(np.linspace(0, B - 1, min(B, n)).astype(int))


def oracle_scores(oracle, Q, Dn, rows):
    """The CPU oracle's own scores of the spread queries (computed once per corpus)."""
    return oracle.score_all(np.ascontiguousarray(Q.cpu().numpy()[rows]), Dn)


def oracle_counts(So, t, mask, rows):
    hit = So >= t.cpu().numpy()[rows][:, None]
    return (hit if mask is None else hit & mask[None, :]).sum(1)


def pattern_thresholds(S, kth, nstar, shift):
    """One threshold per query, the kinds rotating with the query: -inf, +inf, a score taken from S itself (the planted tie:
    document nstar[b] sits exactly at the threshold), the next float above it, the k-th value a search returned, NaN."""
    B = S.shape[0]
    b = torch.arange(B, device=S.device)
    at = S[b, nstar]
    up = torch.nextafter(at, torch.full_like(at, INF))
    kinds = torch.stack([torch.full_like(at, -INF), torch.full_like(at, INF), at, up, kth, torch.full_like(at, float("nan"))])
    return kinds[(b + shift) % 6, b].contiguous()


CASES = [(bf, d, B, NS[(a + 2 * b) % len(NS)]) for a, (bf, d) in enumerate(WIDTHS) for b, B in enumerate(BS)]


@pytest.mark.parametrize("bf16,d,B,N", CASES)
def test_count_equals_the_scores(tt, oracle, bf16, d, B, N):
    D = rows_on_device(100 + d + N, N, d, bf16)
    Dn = host_f32(D)
    Q = queries(200 + B + d, B, d)
    S = all_scores(tt, Q, D)
    mask = masks_for(N, d + B)["half"]
    mask[N - 1] = True                                                    # (N = 1: something is kept)
    mask_t = torch.from_numpy(mask).cuda()
    keep = tt.pack_keep_mask(mask_t)
    k = min(10, N)
    nstar = (7 * torch.arange(B, device="cuda") + 3) % N
    rows = spread(B)
    So = oracle_scores(oracle, Q, Dn, rows)
    for name, m_np, m_t, kp in (("unmasked", None, None, None), ("half", mask, mask_t, keep)):
        n_kept = N if m_np is None else int(m_np.sum())
        kth = tt.score_topk(Q, D, k, keep=kp)[0][:, k - 1].contiguous()   # (-inf where fewer than k are kept)
        got = torch.empty((6, B), dtype=torch.int64, device="cuda")
        want = torch.empty_like(got)
        for shift in range(6):
            t = pattern_thresholds(S, kth, nstar, shift)
            got[shift] = tt.score_count(Q, D, t, keep=kp)
            want[shift] = want_counts(S, t, m_t)
            if shift == 0:
                oc = oracle_counts(So, t, m_np, rows)
                assert np.array_equal(got[0].cpu().numpy()[rows], oc), (name, got[0].cpu().numpy()[rows], oc)
        print(f"{name}: N={N} kept={n_kept} mismatches {int((got != want).sum())} of {got.numel()}, "
              f"counts {sorted(set(want.flatten().tolist()))[:8]}")
        assert torch.equal(got, want), name
        # the vector really asks something: a 0, every kept document, and -- where the corpus has room -- values in between
        w = want.flatten()
        assert bool((w == 0).any()) and bool((w == n_kept).any())
        if N >= 31:
            assert bool(((w > 0) & (w < n_kept)).any())
        # the planted tie: t = S[b, n*] counts n* (when kept) and everything tied with it, the next float up counts none of them
        b = torch.arange(B, device="cuda")
        at, up = got[(2 - b) % 6, b], got[(3 - b) % 6, b]
        tied = S == S[b, nstar][:, None]
        if m_t is not None:
            tied = tied & m_t[None, :]
        assert torch.equal(at - up, tied.sum(1))
        if m_t is None:
            assert bool((at - up >= 1).all())


@pytest.mark.parametrize("bf16,d", [(False, 256), (True, 64)])
def test_masks(tt, oracle, bf16, d):
    N, B = 65_537, 33
    D = rows_on_device(300 + d, N, d, bf16)
    Dn = host_f32(D)
    Q = queries(301 + d, B, d)
    S = all_scores(tt, Q, D)
    nstar = (11 * torch.arange(B, device="cuda") + 5) % N
    rows = spread(B)
    So = oracle_scores(oracle, Q, Dn, rows)
    kth = tt.score_topk(Q, D, 10)[0][:, 9].contiguous()
    t = pattern_thresholds(S, kth, nstar, 2)
    plain = tt.score_count(Q, D, t)
    assert torch.equal(plain, want_counts(S, t))
    low = torch.full((B,), -INF, device="cuda")
    for name, mask in masks_for(N, d + B).items():
        mask_t = torch.from_numpy(mask).cuda()
        keep = tt.pack_keep_mask(mask_t)
        got = tt.score_count(Q, D, t, keep=keep)
        assert torch.equal(got, want_counts(S, t, mask_t)), name
        assert np.array_equal(got.cpu().numpy()[rows], oracle_counts(So, t, mask, rows)), name
        assert tt.score_count(Q, D, low, keep=keep).tolist() == [int(mask.sum())] * B, name   # -inf: the kept documents
        if name == "ones":
            assert torch.equal(got, plain)
        if name == "zeros":
            assert int(got.abs().sum()) == 0
    one = tt.score_count(Q[4], D, float(t[4]))                             # a single query [d], a Python float
    assert one.dim() == 0 and int(one) == int(plain[4])


@pytest.mark.parametrize("bf16,d,B", [(False, 128, 40), (False, 384, 5), (True, 128, 16)])
def test_duplicate_rows_straddle_the_threshold(tt, oracle, bf16, d, B):
    """A row repeated 100 times: the whole tie group is counted at its score and none of it one float above; with 40 of the
    copies masked, 60."""
    N = 5000
    D = rows_on_device(400 + d, N, d, bf16)
    Q = queries(401 + d, B, d)
    dup = np.random.RandomState(d).choice(N, 100, replace=False)
    D[torch.from_numpy(dup).cuda()] = (Q[0] * 0.5).to(D.dtype)
    S = all_scores(tt, Q, D)
    s_dup = S[:, int(dup[0])].contiguous()                                 # every query's score of the repeated row
    up = torch.nextafter(s_dup, torch.full_like(s_dup, INF))
    mask = np.random.RandomState(d + 1).rand(N) < 0.5
    mask[dup[:40]], mask[dup[40:]] = False, True
    mask_t = torch.from_numpy(mask).cuda()
    keep = tt.pack_keep_mask(mask_t)
    at, above = tt.score_count(Q, D, s_dup), tt.score_count(Q, D, up)
    assert torch.equal(at, want_counts(S, s_dup)) and torch.equal(above, want_counts(S, up))
    assert bool((at - above >= 100).all()) and int(at[0]) == 100 and int(above[0]) == 0   # the copies are query 0's best
    at_m, above_m = tt.score_count(Q, D, s_dup, keep=keep), tt.score_count(Q, D, up, keep=keep)
    assert torch.equal(at_m, want_counts(S, s_dup, mask_t)) and torch.equal(above_m, want_counts(S, up, mask_t))
    assert bool((at_m - above_m >= 60).all()) and int(at_m[0]) == 60
    rows = spread(B)
    assert np.array_equal(at_m.cpu().numpy()[rows], oracle_counts(oracle_scores(oracle, Q, host_f32(D), rows), s_dup, mask, rows))


@pytest.mark.parametrize("bf16", (False, True))
def test_accumulate_over_two_halves(tt, bf16):
    from twotowermlretrieval_amd import _lib
    L = _lib.lib()
    N, d, B, cut = 10_001, 128, 20, 4992                                   # the split is a multiple of 32
    D = rows_on_device(500, N, d, bf16)
    Q = queries(501, B, d)
    S = all_scores(tt, Q, D)
    t = S[:, 77].contiguous()
    mask_t = torch.rand(N, device="cuda") < 0.5
    keep = tt.pack_keep_mask(mask_t)
    fn = L.tt_score_count_bf16 if bf16 else L.tt_score_count_f32
    st = torch.cuda.current_stream().cuda_stream

    def call(rows, kp, count, accumulate):
        n = rows.shape[0]
        ws = torch.empty(max(L.tt_score_count_workspace_bytes(B, n, d, int(bf16)), 16), dtype=torch.uint8, device="cuda")
        _lib.check(fn(Q.data_ptr(), B, d, rows.data_ptr(), n, None if kp is None else kp.data_ptr(), t.data_ptr(),
                      count.data_ptr(), accumulate, ws.data_ptr(), ws.numel(), st))

    for kp, m_t in ((None, None), (keep, mask_t)):
        whole = tt.score_count(Q, D, t, keep=kp)
        assert torch.equal(whole, want_counts(S, t, m_t))
        count = torch.full((B,), 12345, dtype=torch.int64, device="cuda")  # accumulate = 0 overwrites
        call(D[:cut], None if kp is None else kp[:cut // 32], count, 0)
        call(D[cut:], None if kp is None else kp[cut // 32:], count, 1)
        assert torch.equal(count, whole)
        call(D[:0], None, count, 1)                                         # an empty block adds nothing ...
        assert torch.equal(count, whole)
        call(D[:0], None, count, 0)                                         # ... and writes zeros without accumulate
        assert int(count.abs().sum()) == 0


# ---- range_search ---------------------------------------------------------------------------------------------------------------

def check_range(tt, ix, Q, t, k, S, mask_t, keep=None):
    """The contract: counts = the expected counts; the rows are search(q, k) with the entries below t replaced by the tail;
    row b holds min(counts[b], k) real entries."""
    counts, v, i = ix.range_search(Q, t, k, keep=keep)
    sv, si = ix.search(Q, k, keep=keep)
    torch.cuda.synchronize()
    assert counts.dtype == torch.int64 and torch.equal(counts, want_counts(S, t, mask_t))
    live = (sv >= t[:, None]) & (si >= 0)
    assert torch.equal(v, torch.where(live, sv, torch.full_like(sv, -INF)))
    assert torch.equal(i, torch.where(live, si, torch.full_like(si, -1)))
    real = (i >= 0).sum(1)
    assert torch.equal(real, counts.clamp(max=k))
    assert torch.equal(ix.count(Q, t, keep=keep), counts)
    return counts


@pytest.fixture(scope="module")
def range_corpus(tt):
    N, d, B = 70_000, 256, 40
    D = rows_on_device(600, N, d)
    Q = queries(601, B, d)
    D[torch.arange(B, device="cuda") * 1000 + 7] = Q                       # query q's best document is row 1000 q + 7
    out = {}
    for bf16 in (False, True):
        Dx = D.to(torch.bfloat16) if bf16 else D
        S = all_scores(tt, Q, Dx)
        top = torch.sort(S, dim=1, descending=True)[0][:, :100].contiguous()
        out[bf16] = (Dx, S, top)
    return Q, out


def range_thresholds(top, shift):
    """Per query, rotating: +inf (count 0), the 5th / 10th / 50th / 100th best score (counts below, at and above k), -inf."""
    B = top.shape[0]
    b = torch.arange(B, device=top.device)
    kinds = torch.stack([torch.full_like(top[:, 0], INF), top[:, 4], top[:, 9], top[:, 49], top[:, 99],
                         torch.full_like(top[:, 0], -INF)])
    return kinds[(b + shift) % 6, b].contiguous()


@pytest.mark.parametrize("kind", ("plain", "screen", "bf16", "screen_masked"))
@pytest.mark.parametrize("k", (10, 100))
def test_range_search_on_brute_force_index(tt, oracle, range_corpus, kind, k):
    Q, per = range_corpus
    D, S, top = per[kind == "bf16"]
    N, B = D.shape[0], Q.shape[0]
    ix = tt.BruteForceIndex(D, screen=kind in ("screen", "screen_masked"), screen_masked=kind == "screen_masked")
    if kind in ("screen", "screen_masked"):
        assert ix._screens(B, 10)                                          # k = 10 rows come from the screened route
    t = range_thresholds(top, k // 10)
    counts = check_range(tt, ix, Q, t, k, S, None)
    assert 0 in counts.tolist() and N in counts.tolist() and 5 in counts.tolist() and 50 in counts.tolist()
    rows = spread(B)
    assert np.array_equal(counts.cpu().numpy()[rows], oracle_counts(oracle_scores(oracle, Q, host_f32(D), rows), t, None, rows))
    gone = [1000 * q + 7 for q in range(0, B, 2)] + [N + 5]               # every other query loses its best document
    ix.remove_ids(gone)
    mask_t = torch.ones(N, dtype=torch.bool, device="cuda")
    mask_t[torch.tensor(gone[:-1], device="cuda")] = False
    after = check_range(tt, ix, Q, t, k, S, mask_t)
    assert N - len(gone) + 1 in after.tolist() and not torch.equal(after, counts)
    call = torch.rand(N, device="cuda") < 0.5                              # a per-call keep ANDed with the removals
    check_range(tt, ix, Q, t, k, S, mask_t & call, keep=tt.pack_keep_mask(call))
    c1, v1, i1 = ix.range_search(Q[3], float(t[3]), k)                     # a single query [d]
    c, v, i = ix.range_search(Q, t, k)
    assert c1.dim() == 0 and int(c1) == int(c[3]) and torch.equal(v1, v[3]) and torch.equal(i1, i[3])


def test_streamed_index_equals_the_resident_one(tt):
    N, d, k, B = 10_000, 128, 10, 20
    Db = rows_on_device(91, N, d, bf16=True)
    Q = queries(92, B, d)
    S = all_scores(tt, Q, Db)
    top = torch.sort(S, dim=1, descending=True)[0][:, :100].contiguous()
    t = range_thresholds(top, 1)
    mask_t = torch.rand(N, device="cuda") < 0.5
    keep = tt.pack_keep_mask(mask_t)
    ref = tt.BruteForceIndex(Db, idx_offset=50)
    st = tt.StreamedIndex(Db.cpu(), block_docs=4096, idx_offset=50)       # three blocks, the last one ragged (1808 rows)
    for kp, m_t in ((None, None), (keep, mask_t)):
        a, b = st.range_search(Q, t, k, keep=kp), ref.range_search(Q, t, k, keep=kp)
        assert all(torch.equal(x, y) for x, y in zip(a, b))
        assert torch.equal(a[0], want_counts(S, t, m_t)) and torch.equal(st.count(Q, t, keep=kp), a[0])
    ids = [50 + int(x) for x in torch.nonzero(S[0] >= t[0]).flatten()[:3].tolist()] + [7]   # (7: below the offset, ignored)
    st.remove_ids(ids)
    ref.remove_ids(ids)
    a, b = st.range_search(Q, t, k, keep=keep), ref.range_search(Q, t, k, keep=keep)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert int(st.count(Q[0], float(t[0]))) == int(ref.count(Q[0], float(t[0])))
    odd = tt.StreamedIndex(Db.cpu(), block_docs=1000, idx_offset=50)
    assert torch.equal(odd.count(Q, t), want_counts(S, t))                 # unmasked: any block size
    with pytest.raises(ValueError, match="multiple of 32"):
        odd.count(Q, t, keep=keep)


def test_count_in_a_captured_graph(tt):
    N, d, B = 70_000, 256, 48
    D = rows_on_device(81, N, d)
    Q = queries(82, B, d)
    S = all_scores(tt, Q, D)
    top = torch.sort(S, dim=1, descending=True)[0][:, :100].contiguous()
    ix = tt.BruteForceIndex(D)
    ix.remove_ids([int(x) for x in torch.argmax(S, 1)[:5].tolist()])
    thr = range_thresholds(top, 0).clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                          # warm-up outside capture
        ix.count(Q, thr)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = ix.count(Q, thr)
    for shift in (0, 3, 4):                                                # new thresholds in the same buffer
        thr.copy_(range_thresholds(top, shift))
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, ix.count(Q, thr))
        assert torch.equal(out, want_counts(S, thr, tt_mask(ix, N)))


def tt_mask(ix, N):
    """The index's persistent keep-bitmask as a bool [N] tensor."""
    words = ix.keep_mask.cpu().numpy().view(np.uint32)
    bits = np.unpackbits(words.view(np.uint8), bitorder="little")[:N].astype(bool)
    return torch.from_numpy(bits).cuda()


@pytest.mark.parametrize("B,k", [(7, 1), (5, 10), (3, 1024)])
def test_cut_below_alone(tt, B, k):
    g = torch.Generator(device="cuda").manual_seed(B + k)
    v = torch.sort(torch.randn((B, k), device="cuda", generator=g), dim=1, descending=True)[0].contiguous()
    i = torch.randint(0, 1 << 40, (B, k), device="cuda", generator=g)
    pad = k // 3                                                           # rows with padding at the tail
    if pad:
        v[1, -pad:], i[1, -pad:] = -INF, -1
    t = v[:, k // 2].clone()                                               # a threshold that is an entry's own score: it stays
    t[0] = float("nan")                                                    # NaN cuts the whole row
    if B > 2:
        t[2] = -INF                                                        # -inf keeps everything that is not padding
    if B > 3:
        t[3] = INF
    live = (v >= t[:, None]) & (i >= 0)
    want_v = torch.where(live, v, torch.full_like(v, -INF))
    want_i = torch.where(live, i, torch.full_like(i, -1))
    gv, gi = tt.topk_cut_below(v, i, t)
    torch.cuda.synchronize()
    assert gv is v and gi is i                                             # in place
    assert torch.equal(gv, want_v) and torch.equal(gi, want_i)
    assert bool((gi[0] == -1).all()) and bool(torch.isneginf(gv[0]).all())
    if B > 2:
        assert int((gi[2] >= 0).sum()) == k
    keepers = (gi >= 0).sum(1)                                             # the survivors are a prefix
    assert bool(((gi >= 0) == (torch.arange(k, device="cuda")[None, :] < keepers[:, None])).all())
