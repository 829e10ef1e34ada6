"""Tagged search (tt_score_topk_tagged_f32 / _bf16, score_topk_tagged, the indexes' tagged_search): per-query tag filters in
one exact top-k pass.

Query b sees document n iff (tags[n] & match_mask[b]) == match_value[b].  A document's score depends neither on the other
documents nor on the other queries of the batch, so the expected value of query b is what the MASKED call -- unchanged by
this feature -- returns for it under a keep-bitmask of its eligibility: one masked GPU call per distinct filter of the batch,
on the sub-batch of queries that share it.  For four queries of every case it is also the CPU oracle over the query's eligible
rows (tagged_ref).  Values and indices are compared with equality, never a tolerance."""
import numpy as np
import pytest
import torch

import synth
import tagged_ref
from poison import PATTERNS, pattern_id, poisoned_empty

pytestmark = pytest.mark.gpu

FULL = 0xFFFFFFFF


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


def i32(x):
    """32-bit patterns (ints / int64 / uint32 array) as the int32 numpy array that carries them."""
    return tagged_ref.as_u32(np.asarray(x)).view(np.int32)


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(i32(x))).cuda()


def signed(word):
    return word - (1 << 32) if word >= (1 << 31) else word


def masked_expected(tt, Q, D, tags_t, mm, mv, k, idx_offset=0, keep_bool=None):
    """One masked GPU call per distinct (mask, value) of the batch, on the queries that carry it."""
    B = Q.shape[0]
    vals = torch.empty((B, k), dtype=torch.float32, device="cuda")
    idx = torch.empty((B, k), dtype=torch.int64, device="cuda")
    N = D.shape[0]
    for m, v, rows in tagged_ref.distinct_filters(mm, mv, B):
        elig = (tags_t[:N] & signed(m)) == signed(v)
        if keep_bool is not None:
            elig = elig & keep_bool
        r = torch.from_numpy(rows).cuda()
        sv, si = tt.score_topk(Q[r].contiguous(), D, k, idx_offset, keep=tt.pack_keep_mask(elig))
        vals[r] = sv
        idx[r] = si
    return vals, idx


def assert_same(got, want):
    assert torch.equal(got[1], want[1]) and torch.equal(got[0], want[0])


def filter_patterns(N, B, seed):
    """name -> (tags [N], match_mask [B], match_value [B]) as arrays of 32-bit patterns: the issue's eight."""
    rs = np.random.RandomState(seed)
    n, b = np.arange(N, dtype=np.int64), np.arange(B, dtype=np.int64)
    full = np.full(B, FULL, dtype=np.int64)
    out = {}
    out["tenants"] = (n % 3, full, b % 3)
    out["all"] = (rs.randint(0, 1 << 16, N), np.zeros(B, dtype=np.int64), np.zeros(B, dtype=np.int64))
    out["none"] = (rs.randint(0, 1 << 16, N), np.full(B, 0x0F, dtype=np.int64), np.full(B, 0x10, dtype=np.int64))
    # within one 32-query tile: a query whose only eligible document is row N - 1, neighbours that see everything, and a
    # third that sees nothing -- a word shared across lanes gets at least one of them wrong
    t = np.zeros(N, dtype=np.int64)
    t[N - 1] = 7
    mm, mv = np.zeros(B, dtype=np.int64), np.zeros(B, dtype=np.int64)
    mm[b % 7 == 0], mv[b % 7 == 0] = FULL, 7
    mm[b % 7 == 3], mv[b % 7 == 3] = 0, 1
    out["one_tile"] = (t, mm, mv)
    # tags alternate by 32-document tile: whole tiles are dead for some lanes of a wave and live for others
    out["alt_tiles"] = ((n // 32) % 2, full, b % 2)
    out["one_percent"] = ((rs.rand(N) < 0.01).astype(np.int64), full, (b % 2 == 0).astype(np.int64))
    # two packed fields, bits 0-7 and bits 8-9: even queries match the first only, odd queries both
    fa, fb = n % 3, (n // 5) % 2
    both = b % 2 == 1
    out["two_fields"] = (fa | (fb << 8) | (rs.randint(0, 1 << 12, N).astype(np.int64) << 10),
                         np.where(both, 0x3FF, 0xFF), np.where(both, (b % 3) | (((b // 2) % 2) << 8), b % 3))
    # bit 31 in tags, masks and values: unsigned throughout
    hi = (n % 2 == 0).astype(np.int64) << 31
    out["bit31"] = (hi | (n % 3), np.where(b % 4 == 3, 1 << 31, FULL), np.where(b % 4 == 3, 1 << 31, (1 << 31) | (b % 3)))
    return out


# (dtype, d) over the support matrix x B: the 16-query tile, the 32-query tile, two tiles, paced + pooled; N and k rotate
WIDTHS = [(False, 32), (False, 256), (False, 320), (False, 512), (True, 64), (True, 256)]
BS = (1, 16, 17, 33, 130)
NS = (1, 31, 1000, 65_537, 300_001)
KS = (1, 10, 64)
CASES = [(bf, d, B, NS[(a + 2 * b) % len(NS)], KS[(a + b) % len(KS)]) for a, (bf, d) in enumerate(WIDTHS) for b, B in enumerate(BS)]


@pytest.mark.parametrize("bf16,d,B,N,k", CASES)
def test_tagged_equals_masked_per_filter(tt, oracle, bf16, d, B, N, k):
    D = rows_on_device(100 + d + N, N, d, bf16)
    Q = queries(200 + B + d, B, d)
    plain = tt.score_topk(Q, D, k)
    pats = filter_patterns(N, B, d + B)
    # the oracle takes one pattern per case (they rotate over the grid), four queries of it
    oracle_pat = sorted(pats)[CASES.index((bf16, d, B, N, k)) % len(pats)]
    for name, (tags, mm, mv) in pats.items():
        tags_t, mm_t, mv_t = dev(tags), dev(mm), dev(mv)
        got = tt.score_topk_tagged(Q, D, tags_t, mm_t, mv_t, k)
        want = masked_expected(tt, Q, D, tags_t, mm, mv, k)
        torch.cuda.synchronize()
        bad = int((got[1] != want[1]).sum()), int((got[0] != want[0]).sum())
        print(f"tagged {name}: index mismatches {bad[0]}, value mismatches {bad[1]}")
        assert_same(got, want)
        if name == "all":                                  # the unmasked call, bit for bit
            assert_same(got, plain)
        if name == "none":
            assert bool((got[1] == -1).all()) and bool(torch.isneginf(got[0]).all())
        if name == "one_tile":
            assert got[1][0].tolist() == [N - 1] + [-1] * (k - 1)
            if B > 3:
                assert bool((got[1][3] == -1).all()) and torch.equal(got[1][1], plain[1][1])
        if name == oracle_pat:
            rows = np.unique(np.linspace(0, B - 1, min(B, 4)).astype(int))
            elig = tagged_ref.eligibility(i32(tags), i32(mm), i32(mv))
            ov, oi = tagged_ref.expected(oracle, Q.cpu().numpy(), D.cpu().float().numpy(), elig, k, rows)
            gv, gi = got[0].cpu().numpy()[rows], got[1].cpu().numpy()[rows]
            assert np.array_equal(gi, oi) and np.array_equal(gv, ov)


@pytest.fixture(scope="module")
def mid():
    """One mid-sized fp32 corpus with tenant tags shared by the tests below: d = 256, 40 queries (two tiles)."""
    N, d, B = 5000, 256, 40
    D = rows_on_device(17, N, d)
    Q = queries(18, B, d)
    tags = np.random.RandomState(3).randint(0, 3, N).astype(np.int64)
    D[[100, 2500, 4999, 17]] = Q[3]                        # duplicates of query 3's best row, under different tags
    tags[[17, 2500, 4999]] = 1
    tags[100] = 2
    mv = np.arange(B) % 3
    mv[3] = 1
    return D, Q, tags, np.full(B, FULL, dtype=np.int64), mv


def test_ties_among_eligible_copies_and_offset(tt, oracle, mid):
    D, Q, tags, mm, mv = mid
    k, off = 10, 2 ** 33 + 5
    tags_t = dev(tags)
    got = tt.score_topk_tagged(Q, D, tags_t, dev(mm), dev(mv), k, idx_offset=off)
    assert_same(got, masked_expected(tt, Q, D, tags_t, mm, mv, k, off))
    assert got[1][3, :3].tolist() == [off + r for r in (17, 2500, 4999)]   # index ascending among the eligible copies
    assert not bool((got[1] == off + 100).any())                           # the copy under another tag is nobody's
    rows = np.array([0, 3, 39])
    elig = tagged_ref.eligibility(i32(tags), i32(mm), i32(mv))
    ov, oi = tagged_ref.expected(oracle, Q.cpu().numpy(), D.cpu().numpy(), elig, k, rows, off)
    assert np.array_equal(got[1].cpu().numpy()[rows], oi) and np.array_equal(got[0].cpu().numpy()[rows], ov)
    v1, i1 = tt.score_topk_tagged(Q[3], D, tags_t, FULL, 1, k, idx_offset=off)   # a 1-D q, Python ints
    assert v1.shape == (k,) and torch.equal(i1, got[1][3]) and torch.equal(v1, got[0][3])
    with pytest.raises(ValueError, match="k = 65"):
        tt.score_topk_tagged(Q, D, tags_t, 0, 0, 65)


@pytest.mark.parametrize("bf16,d,B", [(False, 256, 40), (False, 384, 5), (True, 128, 130)])
def test_keep_mask_is_anded_in(tt, bf16, d, B):
    N, k = 70_001, 10
    D = rows_on_device(31 + d, N, d, bf16)
    Q = queries(32 + d, B, d)
    tags, mm, mv = filter_patterns(N, B, 5)["tenants"]
    tags_t = dev(tags)
    half = torch.from_numpy(np.random.RandomState(d).rand(N) < 0.5).cuda()
    got = tt.score_topk_tagged(Q, D, tags_t, dev(mm), dev(mv), k, keep=tt.pack_keep_mask(half))
    assert_same(got, masked_expected(tt, Q, D, tags_t, mm, mv, k, keep_bool=half))
    assert bool(half[got[1].flatten()].all())
    none = torch.zeros(N, dtype=torch.bool, device="cuda")
    got = tt.score_topk_tagged(Q, D, tags_t, dev(mm), dev(mv), k, keep=tt.pack_keep_mask(none))
    assert bool((got[1] == -1).all()) and bool(torch.isneginf(got[0]).all())


def test_null_tags_is_the_masked_call(tt):
    from twotowermlretrieval_amd import _lib
    L = _lib.lib()
    B, N, d, k = 40, 5000, 128, 10
    D, Q = rows_on_device(1, N, d), queries(2, B, d)
    keep = tt.pack_keep_mask(torch.from_numpy(np.random.RandomState(1).rand(N) < 0.5).cuda())
    want = tt.score_topk(Q, D, k, keep=keep)
    v = torch.empty((B, k), device="cuda")
    i = torch.empty((B, k), dtype=torch.int64, device="cuda")
    ws = torch.empty(L.tt_score_topk_tagged_workspace_bytes(B, N, d, k, 0), dtype=torch.uint8, device="cuda")
    _lib.check(L.tt_score_topk_tagged_f32(Q.data_ptr(), B, d, D.data_ptr(), N, None, None, None, keep.data_ptr(), k, 0,
                                          v.data_ptr(), i.data_ptr(), ws.data_ptr(), ws.numel(),
                                          torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert torch.equal(i, want[1]) and torch.equal(v, want[0])


@pytest.mark.parametrize("word", PATTERNS[1:], ids=pattern_id)
@pytest.mark.parametrize("bf16,d,B,N", [(False, 256, 130, 300_001), (False, 512, 5, 65_537), (True, 64, 33, 1000)])
def test_results_do_not_depend_on_what_the_buffers_held(tt, word, bf16, d, B, N):
    """Paced + pooled with a sample pass, the 16-query kernel, a bf16 tile: every workspace and output from a poisoned
    torch.empty gives the bits of the clean run."""
    k = 10
    D = rows_on_device(41 + d, N, d, bf16)
    Q = queries(42 + d, B, d)
    tags, mm, mv = filter_patterns(N, B, 9)["two_fields"]
    args = (Q, D, dev(tags), dev(mm), dev(mv), k)
    clean = tt.score_topk_tagged(*args)
    with poisoned_empty(word) as p:
        got = tt.score_topk_tagged(*args)
    torch.cuda.synchronize()
    assert p.tensors >= 3                                  # values, indices, workspace
    assert_same(got, clean)


def test_graph_replay_follows_match_value(tt, mid):
    """One score_topk_tagged call with static tensors captured in a graph (a single stream: a linear capture); match_value
    is overwritten in place and the replay answers for the new filters."""
    D, Q, tags, mm, mv = mid
    k = 10
    tags_t, mm_t, mv_t = dev(np.concatenate([tags, np.zeros(-len(tags) % 32, dtype=np.int64)])), dev(mm), dev(mv)
    first = masked_expected(tt, Q, D, tags_t, mm, mv, k)
    mv2 = (mv + 1) % 3
    second = masked_expected(tt, Q, D, tags_t, mm, mv2, k)
    assert not torch.equal(first[1], second[1])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                          # warm-up outside capture: kernels loaded, blocks cached
        tt.score_topk_tagged(Q, D, tags_t, mm_t, mv_t, k)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = tt.score_topk_tagged(Q, D, tags_t, mm_t, mv_t, k)
    graph.replay()
    torch.cuda.synchronize()
    assert_same(out, first)
    mv_t.copy_(dev(mv2))
    graph.replay()
    torch.cuda.synchronize()
    assert_same(out, second)


def test_brute_force_index_screened_or_not(tt):
    """screen=True and screen=False give the same bits (the exact kernel either way), fallback_flags read as after
    search(keep=), remove_ids and keep= compose, a 1-D q works, and the refusals."""
    N, d, k, off, B = 70_000, 256, 10, 1000, 40
    D = rows_on_device(61, N, d)
    Q = queries(62, B, d)
    tags, mm, mv = filter_patterns(N, B, 11)["tenants"]
    D[torch.arange(B, device="cuda") * 3 * 500 + (torch.arange(B, device="cuda") % 3)] = Q   # query b's best: a row of its tenant
    best = [1500 * b + b % 3 for b in range(B)]
    tags_t = dev(tags)
    want = masked_expected(tt, Q, D, tags_t, mm, mv, k, off)
    assert want[1][:, 0].tolist() == [off + r for r in best]
    res = {}
    for screen in (False, True):
        ix = tt.BruteForceIndex(D, idx_offset=off, screen=screen)
        assert ix.tags is None
        with pytest.raises(ValueError, match="no tags"):
            ix.tagged_search(Q, k, dev(mm), dev(mv))
        ix.set_tags(tags_t)
        assert ix.tags.shape == (32 * ((N + 31) // 32),) and torch.equal(ix.tags[:N], tags_t)
        res[screen] = ix.tagged_search(Q, k, dev(mm), dev(mv))
        assert_same(res[screen], want)
        if screen:
            assert ix._screens(B, k) and int(ix.fallback_flags.ne(0).sum()) == ix.fallback_flags.numel() == 2
        v1, i1 = ix.tagged_search(Q[4], k, FULL, int(mv[4]))                      # 1-D q, Python ints
        assert v1.shape == (k,) and torch.equal(i1, want[1][4]) and torch.equal(v1, want[0][4])
        out = (torch.empty((B, k), device="cuda"), torch.empty((B, k), dtype=torch.int64, device="cuda"))
        assert ix.tagged_search(Q, k, dev(mm), dev(mv), out=out) is out
        assert_same(out, want)
        with pytest.raises(ValueError, match="k = 65"):
            ix.tagged_search(Q, 65, dev(mm), dev(mv))
        gone = [off + r for r in best[::2]]
        ix.remove_ids(gone + [5, off + N])                                         # ids that are not this index's are ignored
        kept = torch.ones(N, dtype=torch.bool, device="cuda")
        kept[torch.tensor(best[::2], device="cuda")] = False
        got = ix.tagged_search(Q, k, dev(mm), dev(mv))
        assert_same(got, masked_expected(tt, Q, D, tags_t, mm, mv, k, off, keep_bool=kept))
        assert not np.isin(got[1].cpu().numpy(), np.array(gone)).any()
        call = torch.from_numpy(np.random.RandomState(5).rand(N) < 0.5).cuda()   # per-call keep AND persistent mask
        got = ix.tagged_search(Q, k, dev(mm), dev(mv), keep=tt.pack_keep_mask(call))
        assert_same(got, masked_expected(tt, Q, D, tags_t, mm, mv, k, off, keep_bool=kept & call))
    assert_same(res[True], res[False])


def test_streamed_index_equals_resident(tt):
    N, d, k, B = 10_000, 128, 10, 20
    Db = rows_on_device(91, N, d, bf16=True)
    Q = queries(92, B, d)
    tags, mm, mv = filter_patterns(N, B, 13)["two_fields"]
    tags_t = dev(tags)
    ref = tt.BruteForceIndex(Db, idx_offset=50)
    ref.set_tags(tags_t)
    st = tt.StreamedIndex(Db.cpu(), block_docs=4096, idx_offset=50)               # three blocks
    assert (N + st.block - 1) // st.block >= 3 and st.tags is None
    with pytest.raises(ValueError, match="no tags"):
        st.tagged_search(Q, k, dev(mm), dev(mv))
    st.set_tags(tags_t)
    assert st.tags.is_cuda and st.tags.numel() == 32 * ((N + 31) // 32)
    a, b = st.tagged_search(Q, k, dev(mm), dev(mv)), ref.tagged_search(Q, k, dev(mm), dev(mv))
    assert_same(a, b)
    assert_same(b, masked_expected(tt, Q, Db, tags_t, mm, mv, k, 50))
    keep = tt.pack_keep_mask(torch.from_numpy(np.random.RandomState(6).rand(N) < 0.5).cuda())
    ids = [int(x) for x in b[1][:, 0].tolist() if x >= 0]
    st.remove_ids(ids)
    ref.remove_ids(ids)
    a, b = st.tagged_search(Q, k, dev(mm), dev(mv), keep=keep), ref.tagged_search(Q, k, dev(mm), dev(mv), keep=keep)
    assert_same(a, b)
    assert not np.isin(a[1].cpu().numpy(), np.array(ids)).any()
    v1, i1 = st.tagged_search(Q[2], k, int(mm[2]), int(mv[2]), keep=keep)
    assert torch.equal(i1, a[1][2]) and torch.equal(v1, a[0][2])
    odd = tt.StreamedIndex(Db.cpu(), block_docs=1000, idx_offset=50)
    odd.set_tags(tags_t)
    with pytest.raises(ValueError, match="multiple of 32"):
        odd.tagged_search(Q, k, dev(mm), dev(mv))
