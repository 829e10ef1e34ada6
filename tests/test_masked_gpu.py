"""Masked exact top-k (tt_score_topk_masked_f32 / _bf16, score_topk(..., keep=), the indexes' search(keep=) / remove_ids).

A document's score does not depend on the other documents, so a masked search over D is the plain search over the kept rows
with the indices mapped back, bit for bit, ties included.  The expected value everywhere is therefore the untouched CPU
oracle over D[kept] (on a sample of the queries), and -- for ALL queries -- the unmasked GPU kernel over D[kept]; values and
indices are compared with equality, not a tolerance."""
import ctypes as C

import numpy as np
import pytest
import torch

import synth
from test_search_aux_gpu import par_rows

pytestmark = pytest.mark.gpu

SIZE_MAX = C.c_size_t(-1).value


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


def host_f32(D):
    return D.cpu().float().numpy()


def expected(oracle, Qn, Dn, mask, k, rows, idx_offset=0):
    """The issue's expected value: the oracle over the kept rows, indices mapped back (no kept row: all tail)."""
    kept = np.flatnonzero(mask)
    if len(kept) == 0:
        return np.full((len(rows), k), -np.inf, dtype=np.float32), np.full((len(rows), k), -1, dtype=np.int64)
    Dk = np.ascontiguousarray(Dn[kept])
    v, i = par_rows(lambda q: oracle.score_topk(q, Dk, k), Qn[rows])
    return v, np.where(i >= 0, kept[np.maximum(i, 0)] + idx_offset, -1)


def compacted(tt, Q, D, mask_t, k, idx_offset=0):
    """The unmasked GPU kernel over D[kept], indices mapped back: the expected value for every query."""
    kept = torch.nonzero(mask_t, as_tuple=False).flatten()
    v, i = tt.score_topk(Q, D[kept].contiguous(), k)
    if kept.numel() == 0:
        return v, i
    return v, torch.where(i >= 0, kept[i.clamp(min=0)] + idx_offset, i)


def check(tt, oracle, Q, D, Dn, mask, k, idx_offset=0, nrows=4):
    mask_t = torch.from_numpy(mask).cuda()
    keep = tt.pack_keep_mask(mask_t)
    got = tt.score_topk(Q, D, k, idx_offset, keep=keep)
    ref = compacted(tt, Q, D, mask_t, k, idx_offset)
    torch.cuda.synchronize()
    assert torch.equal(got[1], ref[1]) and torch.equal(got[0], ref[0])
    B = Q.shape[0]
    rows = np.unique(np.linspace(0, B - 1, min(B, nrows)).astype(int))
    ov, oi = expected(oracle, Q.cpu().numpy(), Dn, mask, k, rows, idx_offset)
    gv, gi = got[0].cpu().numpy()[rows], got[1].cpu().numpy()[rows]
    print(f"masked top-k: kept {int(mask.sum())}/{len(mask)}, index mismatches {int((gi != oi).sum())}, "
          f"value mismatches {int((gv != ov).sum())}")
    assert np.array_equal(gi, oi) and np.array_equal(gv, ov)
    return got


def masks_for(N, seed):
    rs = np.random.RandomState(seed)
    last = np.zeros(N, dtype=bool)
    last[N - 1] = True                                   # a single kept bit, in the last (partial) word
    return {"half": rs.rand(N) < 0.5, "one_percent": rs.rand(N) < 0.01, "ones": np.ones(N, dtype=bool),
            "zeros": np.zeros(N, dtype=bool), "last_bit": last, "alt_words": (np.arange(N) // 32) % 2 == 1}


# (dtype, d) over the support matrix x B: the 16-query tile, the 32-query tile, two tiles, paced + pooled; N and k rotate
WIDTHS = [(False, 32), (False, 256), (False, 320), (False, 512), (True, 64), (True, 256)]
BS = (1, 16, 17, 33, 130)
NS = (1, 31, 1000, 65_537, 300_001)
KS = (1, 10, 64)
CASES = [(bf, d, B, NS[(a + 2 * b) % len(NS)], KS[(a + b) % len(KS)]) for a, (bf, d) in enumerate(WIDTHS) for b, B in enumerate(BS)]


@pytest.mark.parametrize("bf16,d,B,N,k", CASES)
def test_masked_equals_search_over_kept_rows(tt, oracle, bf16, d, B, N, k):
    D = rows_on_device(100 + d + N, N, d, bf16)
    Dn = host_f32(D)
    Q = queries(200 + B + d, B, d)
    plain = tt.score_topk(Q, D, k)
    for name, mask in masks_for(N, d + B).items():
        got = check(tt, oracle, Q, D, Dn, mask, k)
        if name == "ones":                                # all kept: the unmasked call, bit for bit
            assert torch.equal(got[1], plain[1]) and torch.equal(got[0], plain[0])
        if name == "zeros":
            assert bool((got[1] == -1).all()) and bool(torch.isneginf(got[0]).all())


def test_keep_none_is_the_unmasked_call(tt):
    from twotowermlretrieval_amd import _lib
    L = _lib.lib()
    B, N, d, k = 40, 5000, 128, 10
    D, Q = rows_on_device(1, N, d), queries(2, B, d)
    a = tt.score_topk(Q, D, k)
    b = tt.score_topk(Q, D, k, keep=None)
    v = torch.empty((B, k), device="cuda")
    i = torch.empty((B, k), dtype=torch.int64, device="cuda")
    ws = torch.empty(L.tt_score_topk_masked_workspace_bytes(B, N, d, k, 0), dtype=torch.uint8, device="cuda")
    _lib.check(L.tt_score_topk_masked_f32(Q.data_ptr(), B, d, D.data_ptr(), N, None, k, 0, v.data_ptr(), i.data_ptr(),
                                          ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert torch.equal(a[1], b[1]) and torch.equal(a[0], b[0]) and torch.equal(a[1], i) and torch.equal(a[0], v)


@pytest.mark.parametrize("bf16", (False, True))
def test_threshold_passes_see_the_mask(tt, oracle, bf16):
    """N = 300 001, B = 5, d = 256: make_plan takes the prepass (N >= 262 144 and 9376 tiles over ~2048 chunks = 5 tiles =
    160 documents per chunk < 65 536), whose sample is the first max(16 384, N / 256) = 16 384 rows, one 32-document tile per
    wave; the main pass is seeded with the k-th largest of the waves' maxima.
    (a) rows [0, 20 000) are all masked: the sample holds nothing that may be returned, so it must give no bound.
    (b) the k best documents of every query are planted in distinct tiles of the sample and masked: a bound taken from them
        (>= 2) exceeds every kept score (< 1), and a kernel that masks only the append pass returns nothing."""
    N, B, d, k = 300_001, 5, 256, 10
    D = rows_on_device(7, N, d, bf16)
    Q = queries(8, B, d)
    a = np.ones(N, dtype=bool)
    a[:20_000] = False
    got = check(tt, oracle, Q, D, host_f32(D), a, k, nrows=B)
    assert bool((got[1] >= 20_000).all())
    b = np.ones(N, dtype=bool)
    for q in range(B):
        for j in range(k):
            r = 64 * (k * q + j) + 5                      # distinct tiles, all below 16 384
            D[r] = (Q[q] * (2.0 + 0.25 * j)).to(D.dtype)
            b[r] = False
    assert int(tt.score_topk(Q, D, k)[1].max()) < 16_384   # unmasked, the planted rows ARE every query's top-k
    got = check(tt, oracle, Q, D, host_f32(D), b, k, nrows=B)
    assert bool((got[1] >= 0).all()) and bool((got[0] < 1.0).all())


@pytest.mark.parametrize("bf16,d", [(False, 256), (False, 384), (True, 128)])
def test_ties_offset_short_and_single_query(tt, oracle, bf16, d):
    N, k, off = 5000, 10, 1 << 33
    D = rows_on_device(17 + d, N, d, bf16)
    Q = queries(18 + d, 40, d)
    D[[100, 2500, 4999, 17]] = Q[3].to(D.dtype)          # duplicates of query 3's best row on both sides of a masked one
    mask = np.random.RandomState(d).rand(N) < 0.7
    mask[[17, 2500, 4999]] = True
    mask[100] = False
    got = check(tt, oracle, Q, D, host_f32(D), mask, k, idx_offset=off, nrows=40)
    assert got[1][3, :3].tolist() == [off + r for r in (17, 2500, 4999)]
    assert not bool((got[1] == off + 100).any())
    few = np.zeros(N, dtype=bool)                         # fewer kept than k: the tail is (-inf, -1)
    few[[4000, 77, 31]] = True
    got = check(tt, oracle, Q, D, host_f32(D), few, k, idx_offset=off, nrows=40)
    assert bool((got[1][:, 3:] == -1).all()) and bool(torch.isneginf(got[0][:, 3:]).all())
    assert sorted(got[1][0, :3].tolist()) == [off + 31, off + 77, off + 4000]
    keep = tt.pack_keep_mask(torch.from_numpy(mask).cuda())
    full = tt.score_topk(Q, D, k, off, keep=keep)
    v1, i1 = tt.score_topk(Q[3], D, k, off, keep=keep)    # a single query vector [d]
    assert v1.shape == (k,) and torch.equal(i1, full[1][3]) and torch.equal(v1, full[0][3])


def test_forced_give_up_redo_carries_the_mask(tt, oracle):
    """The comparison build makes every wave that did not draw a pool block itself give up (TT_DRAW_POLLS=-1): the redo flags
    are raised, the redo pass runs under the same mask and the result is still the expected value."""
    from conftest import ab_library
    from twotowermlretrieval_amd import _lib
    L = _lib.lib()
    B, N, d, k = 130, 900_000, 64, 10
    off = L.tt_score_topk_redo_flags_offset(B, N, d, k)
    assert off != SIZE_MAX                                # paced, with a shared pool
    D = rows_on_device(71, N, d)
    Q = queries(72, B, d)
    mask = np.random.RandomState(3).rand(N) < 0.5
    D[600_000] = Q[5]
    D[600_001] = Q[5]
    mask[600_000], mask[600_001] = False, True
    mask_t = torch.from_numpy(mask).cuda()
    keep = tt.pack_keep_mask(mask_t)
    ws = torch.zeros(L.tt_score_topk_masked_workspace_bytes(B, N, d, k, 0), dtype=torch.uint8, device="cuda")
    ntile = (B + 31) // 32
    v0, i0 = tt.score_topk(Q, D, k, 0, ws, keep=keep)
    torch.cuda.synchronize()
    assert int(ws[off:off + 4 * ntile].view(torch.int32).ne(0).sum()) == 0
    with ab_library(TT_DRAW_POLLS=-1):
        v1, i1 = tt.score_topk(Q, D, k, 0, ws, keep=keep)
        torch.cuda.synchronize()
        redone = int(ws[off:off + 4 * ntile].view(torch.int32).ne(0).sum())
    assert redone > 0, "the forced give-up did not happen"
    assert torch.equal(i1, i0) and torch.equal(v1, v0)
    assert int(i1[5, 0]) == 600_001
    ref = compacted(tt, Q, D, mask_t, k)
    assert torch.equal(i1, ref[1]) and torch.equal(v1, ref[0])
    rows = np.array([0, 5, 129])
    ov, oi = expected(oracle, Q.cpu().numpy(), host_f32(D), mask, k, rows)
    assert np.array_equal(i1.cpu().numpy()[rows], oi) and np.array_equal(v1.cpu().numpy()[rows], ov)


# ---- large k ------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def large_corpus():
    out = {}
    for bf16, d in ((False, 256), (True, 128)):
        D = rows_on_device(300 + d, 70_000, d, bf16)
        out[bf16] = (D, host_f32(D), d)
    return out


@pytest.mark.parametrize("bf16", (False, True))
@pytest.mark.parametrize("B", (3, 40))
@pytest.mark.parametrize("k", (65, 100, 1000))
def test_large_k_masked(tt, oracle, large_corpus, bf16, B, k):
    D, Dn, d = large_corpus[bf16]
    Q = queries(400 + B, B, d)
    mask = np.random.RandomState(k + B).rand(D.shape[0]) < 0.5
    check(tt, oracle, Q, D, Dn, mask, k, nrows=3)


def test_large_k_masked_duplicates_and_short(tt, oracle, large_corpus):
    """6000 exact duplicates of one row (more than the 4096-entry rescan buffer), half of them masked: the 3000 kept ones tie
    at the top of query 0.  They are contiguous rows, so that some wave's whole chunk (64 - 96 documents at this size) is
    kept duplicates: its list of 64 is full of entries at t_q, i.e. saturated, and the query is rescanned (tier >= 1) -- a
    scan that did not skip the masked duplicates would count 6000, overflow the buffer and return masked indices."""
    from twotowermlretrieval_amd import _lib
    L = _lib.lib()
    D0, _, d = large_corpus[False]
    D = D0.clone()
    N, B, k = D.shape[0], 40, 100
    Q = queries(500, B, d)
    dup = np.arange(30_000, 36_000)
    D[torch.from_numpy(dup).cuda()] = Q[0]
    mask = np.random.RandomState(10).rand(N) < 0.5
    mask[dup[:3000]] = False
    mask[dup[3000:]] = True
    Dn = host_f32(D)
    keep = tt.pack_keep_mask(torch.from_numpy(mask).cuda())
    ws = torch.zeros(L.tt_score_topk_masked_workspace_bytes(B, N, d, k, 0), dtype=torch.uint8, device="cuda")
    got = tt.score_topk(Q, D, k, 0, ws, keep=keep)
    torch.cuda.synchronize()
    rows = np.array([0, 1, 39])
    ov, oi = expected(oracle, Q.cpu().numpy(), Dn, mask, k, rows)
    assert np.array_equal(got[1].cpu().numpy()[rows], oi) and np.array_equal(got[0].cpu().numpy()[rows], ov)
    assert got[1][0].tolist() == sorted(dup[3000:].tolist())[:k]
    toff = L.tt_score_topk_large_tier_offset(B, N, d, k, 0)
    assert int(ws[toff:toff + 4].view(torch.int32)[0]) >= 1
    few = np.zeros(N, dtype=bool)                         # fewer kept than k at k = 1000
    few[np.random.RandomState(11).choice(N, 500, replace=False)] = True
    got = check(tt, oracle, Q, D, Dn, few, 1000, nrows=3)
    assert bool((got[1][:, 500:] == -1).all()) and bool((got[1][:, :500] >= 0).all())


# ---- host layer ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N", (1, 31, 32, 33, 1000))
def test_pack_keep_mask_equals_packbits(tt, N):
    m = np.random.RandomState(N).rand(N) < 0.5
    m[N - 1] = True
    want = np.packbits(np.concatenate([m, np.zeros(-N % 32, dtype=bool)]), bitorder="little").view(np.uint32)
    for t in (torch.from_numpy(m), torch.from_numpy(m.astype(np.uint8) * 3), torch.from_numpy(m.astype(np.float32))):
        got = tt.pack_keep_mask(t.cuda())
        assert got.dtype == torch.int32 and got.shape == ((N + 31) // 32,)
        assert np.array_equal(got.cpu().numpy().view(np.uint32), want)


def test_keep_argument_validation(tt):
    D, Q = rows_on_device(1, 1000, 64), queries(2, 3, 64)
    with pytest.raises(ValueError, match="words"):
        tt.score_topk(Q, D, 5, keep=torch.zeros(31, dtype=torch.int32, device="cuda"))
    with pytest.raises(TypeError):
        tt.score_topk(Q, D, 5, keep=torch.zeros(32, dtype=torch.int64, device="cuda"))
    with pytest.raises(ValueError, match="live on"):
        tt.score_topk(Q, D, 5, keep=torch.zeros(32, dtype=torch.int32))


def test_remove_ids_on_a_screened_index(tt, oracle):
    """A screen=True d = 256 index of 70 000 rows: screened without a mask, the masked exact kernel once it has one; ids
    outside the index are ignored; a removed id never comes back; a per-call keep is ANDed with the persistent mask."""
    N, d, k, off = 70_000, 256, 10, 1000
    D = rows_on_device(61, N, d)
    Q = queries(62, 40, d)
    D[torch.arange(40, device="cuda") * 1000 + 7] = Q      # query q's best document is row 1000 q + 7
    Dn = host_f32(D)
    ix = tt.BruteForceIndex(D, idx_offset=off, screen=True)
    assert ix.keep_mask is None and ix._screens(40, k)
    v, i = ix.search(Q, k)
    assert i[:, 0].tolist() == [off + 1000 * q + 7 for q in range(40)]
    assert int(ix.fallback_flags.ne(0).sum()) == 0         # the screened route
    gone = [off + 1000 * q + 7 for q in range(0, 40, 2)]
    ix.remove_ids(gone + [5, off + N, off - 1, 1 << 40])   # ids that are not this index's are ignored
    assert ix.keep_mask is not None and not ix._screens(40, k)
    mask = np.ones(N, dtype=bool)
    mask[[1000 * q + 7 for q in range(0, 40, 2)]] = False
    assert np.array_equal(ix.keep_mask.cpu().numpy().view(np.uint32),
                          np.packbits(np.concatenate([mask, np.zeros(-N % 32, dtype=bool)]), bitorder="little").view(np.uint32))
    got = ix.search(Q, k)
    assert int(ix.fallback_flags.ne(0).sum()) == ix.fallback_flags.numel() == 2   # the exact kernel took every tile
    rows = np.arange(0, 40, 3)
    ov, oi = expected(oracle, Q.cpu().numpy(), Dn, mask, k, rows, off)
    assert np.array_equal(got[1].cpu().numpy()[rows], oi) and np.array_equal(got[0].cpu().numpy()[rows], ov)
    assert not np.isin(got[1].cpu().numpy(), np.array(gone)).any()
    ptr = ix.keep_mask.data_ptr()
    ix.remove_ids(torch.tensor([off + 1007], device="cuda"))                     # in place: the same buffer
    mask[1007] = False
    assert ix.keep_mask.data_ptr() == ptr
    assert int(ix.search(Q, k)[1][1, 0]) != off + 1007
    call = np.random.RandomState(5).rand(N) < 0.5                                 # per-call keep AND persistent mask
    got = ix.search(Q, k, keep=tt.pack_keep_mask(torch.from_numpy(call).cuda()))
    ov, oi = expected(oracle, Q.cpu().numpy(), Dn, mask & call, k, rows, off)
    assert np.array_equal(got[1].cpu().numpy()[rows], oi) and np.array_equal(got[0].cpu().numpy()[rows], ov)
    v1, i1 = ix.search(Q[4], k)
    full = ix.search(Q, k)
    assert torch.equal(i1, full[1][4]) and torch.equal(v1, full[0][4])


def test_graphed_search_and_removals(tt):
    N, d, k = 70_000, 256, 10
    D = rows_on_device(81, N, d)
    Q = queries(82, 48, d)
    D[torch.arange(48, device="cuda") * 100 + 3] = Q
    ix = tt.BruteForceIndex(D, screen=True)
    g0 = tt.GraphedSearch(ix, 48, k)                       # captured without a mask
    assert g0(Q)[1][:, 0].tolist() == [100 * q + 3 for q in range(48)]
    ix.remove_ids([3, 103])
    with pytest.raises(RuntimeError, match="capture"):
        g0(Q)
    g1 = tt.GraphedSearch(ix, 48, k)                       # captured with one: reads the buffer at every replay
    want = ix.search(Q, k)
    got = g1(Q)
    assert torch.equal(got[1], want[1]) and torch.equal(got[0], want[0])
    assert 3 not in got[1][0].tolist() and int(got[1][2, 0]) == 203
    ix.remove_ids([203])
    got = g1(Q)
    torch.cuda.synchronize()
    want = ix.search(Q, k)
    assert torch.equal(got[1], want[1]) and torch.equal(got[0], want[0]) and int(got[1][2, 0]) != 203


def test_streamed_index_masked(tt):
    N, d, k = 10_000, 128, 10
    Db = rows_on_device(91, N, d, bf16=True)
    Q = queries(92, 20, d)
    mask = np.random.RandomState(6).rand(N) < 0.5
    keep = tt.pack_keep_mask(torch.from_numpy(mask).cuda())
    ref = tt.BruteForceIndex(Db, idx_offset=50)
    st = tt.StreamedIndex(Db.cpu(), block_docs=4096, idx_offset=50)
    a, b = st.search(Q, k, keep=keep), ref.search(Q, k, keep=keep)
    assert torch.equal(a[1], b[1]) and torch.equal(a[0], b[0])
    ids = [int(x) for x in b[1][:, 0].tolist()] + [7]     # (global ids; 7 is below the index's offset: ignored)
    st.remove_ids(ids)
    ref.remove_ids(ids)
    a, b = st.search(Q, k, keep=keep), ref.search(Q, k, keep=keep)
    assert torch.equal(a[1], b[1]) and torch.equal(a[0], b[0])
    assert not np.isin(a[1].cpu().numpy(), np.array(ids)).any()
    a, b = st.search(Q, k), ref.search(Q, k)
    assert torch.equal(a[1], b[1]) and torch.equal(a[0], b[0])
    odd = tt.StreamedIndex(Db.cpu(), block_docs=1000, idx_offset=50)
    assert odd.search(Q, k)[1].shape == (20, k)            # unmasked: any block size
    with pytest.raises(ValueError, match="multiple of 32"):
        odd.search(Q, k, keep=keep)
