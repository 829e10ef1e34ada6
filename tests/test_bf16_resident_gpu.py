"""Search over a bf16 corpus kept as bf16 in HBM (tt_score_topk_bf16, the screened bf16 calls, BruteForceIndex /
ShardedIndex / StreamedIndex.resident over bf16 rows).  bf16 -> fp32 is exact, so every result must be the fp32 kernel's over the widened
rows -- and the CPU oracle's over rows widened on the CPU -- bit for bit: values and indices, ties (score desc, index asc)
and the N < k tail included."""
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


def bf16_rows(seed, n, d):
    """n x d bf16 rows on the device (randn, rounded), generated there: the large corpora never exist as fp32 on the host."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randn((n, d), device="cuda", generator=g).div_(d ** 0.5).to(torch.bfloat16)


def queries(seed, B, d):
    return torch.from_numpy(synth.unit_rows(seed, B, d)).cuda()


def widened(Db):
    """The bf16 rows widened on the CPU (the oracle's input)."""
    return Db.cpu().float().numpy()


def oracle_rows(oracle, Q, Dw, k, rows, idx_offset=0):
    v, i = par_rows(lambda q: oracle.score_topk(q, Dw, k), Q[rows])
    return v, np.where(i >= 0, i + idx_offset, i)


def assert_same(a, b):
    assert torch.equal(a[1], b[1]) and torch.equal(a[0], b[0])


# (d, B) over the support matrix; N and k rotate through the issue's lists so every value meets every width
DS = (64, 128, 192, 256)
BS = (1, 5, 32, 33, 64, 96, 130, 1024)
NS = (1, 31, 1000, 65_537, 1_000_003)
KS = (1, 10, 50, 64)
CASES = [(d, B, NS[(a + 2 * b) % len(NS)], KS[(a + b) % len(KS)]) for a, d in enumerate(DS) for b, B in enumerate(BS)]


@pytest.mark.parametrize("d,B,N,k", CASES)
def test_exact_bf16_equals_f32_kernel_and_oracle(tt, oracle, d, B, N, k):
    Db = bf16_rows(1000 + d + N, N, d)
    Q = queries(2000 + B + d, B, d)
    got = tt.score_topk(Q, Db, k)
    ref = tt.score_topk(Q, Db.float(), k)
    torch.cuda.synchronize()
    assert_same(got, ref)
    rows = np.unique(np.linspace(0, B - 1, min(B, 6)).astype(int))
    ov, oi = oracle_rows(oracle, Q.cpu().numpy(), widened(Db), k, rows)
    assert np.array_equal(got[1].cpu().numpy()[rows], oi) and np.array_equal(got[0].cpu().numpy()[rows], ov)


@pytest.mark.parametrize("d", DS)
def test_idx_offset_ties_and_short_corpus(tt, oracle, d):
    # ties: exact duplicates of a query's best document, spread over the corpus -- the lower index must come first
    N, k = 5000, 10
    Db = bf16_rows(7 + d, N, d)
    Q = queries(8 + d, 40, d)
    Db[[100, 2500, 4999, 17]] = Q[3].to(torch.bfloat16)
    Db[[4000, 60]] = Db[1234].clone()
    got = tt.score_topk(Q, Db, k, idx_offset=1 << 33)
    ref = tt.score_topk(Q, Db.float(), k, idx_offset=1 << 33)
    torch.cuda.synchronize()
    assert_same(got, ref)
    assert got[1][3, :4].tolist() == [(1 << 33) + r for r in (17, 100, 2500, 4999)]
    ov, oi = oracle_rows(oracle, Q.cpu().numpy(), widened(Db), k, np.arange(40), 1 << 33)
    assert np.array_equal(got[1].cpu().numpy(), oi) and np.array_equal(got[0].cpu().numpy(), ov)
    # N < k: the tail is (-inf, -1)
    for N2, k2 in ((1, 10), (31, 64), (5, 50)):
        D2 = Db[:N2].contiguous()
        v, i = tt.score_topk(Q, D2, k2)
        rv, ri = tt.score_topk(Q, D2.float(), k2)
        torch.cuda.synchronize()
        assert torch.equal(i, ri) and torch.equal(v, rv)
        assert bool((i[:, N2:] == -1).all()) and bool(torch.isneginf(v[:, N2:]).all())


def test_single_query_vector(tt):
    Db = bf16_rows(5, 3000, 128)
    q = queries(6, 1, 128)[0]
    v, i = tt.score_topk(q, Db, 10)
    rv, ri = tt.score_topk(q, Db.float(), 10)
    assert v.shape == (10,) and torch.equal(i, ri) and torch.equal(v, rv)


def test_unsupported_width_is_an_error(tt):
    from twotowermlretrieval_amd import _lib
    Db = bf16_rows(3, 100, 96)
    with pytest.raises(_lib.TTError, match="d=96"):
        tt.score_topk(queries(4, 2, 96), Db, 5)


def test_forced_give_up_is_redone_and_exact(tt, oracle):
    """The comparison build forces every pool draw the wave did not make itself to give up (TT_DRAW_POLLS=-1): the redo flags
    are raised and the result is still the product run's and the oracle's."""
    from conftest import ab_library
    from twotowermlretrieval_amd import _lib
    B, N, d, k = 200, 700_000, 128, 10
    L = _lib.lib()
    off = L.tt_score_topk_redo_flags_offset(B, N, d, k)      # (B > 16: the bf16 kernel's layout is the fp32 one)
    assert off != SIZE_MAX
    Db = bf16_rows(71, N, d)
    Q = queries(72, B, d)
    Db[600_000] = Q[5].to(torch.bfloat16)
    ws = torch.zeros(L.tt_score_topk_bf16_workspace_bytes(B, N, d, k), dtype=torch.uint8, device="cuda")
    ntile = (B + 31) // 32
    v0, i0 = tt.score_topk(Q, Db, k, 0, ws)
    torch.cuda.synchronize()
    assert int(ws[off:off + 4 * ntile].view(torch.int32).ne(0).sum()) == 0
    with ab_library(TT_DRAW_POLLS=-1):
        v1, i1 = tt.score_topk(Q, Db, k, 0, ws)
        torch.cuda.synchronize()
        redone = int(ws[off:off + 4 * ntile].view(torch.int32).ne(0).sum())
    assert redone > 0, "the forced give-up did not happen"
    assert torch.equal(i1, i0) and torch.equal(v1, v0)
    assert int(i1[5, 0]) == 600_000
    rows = np.array([0, 5, 199])
    ov, oi = oracle_rows(oracle, Q.cpu().numpy(), widened(Db), k, rows)
    assert np.array_equal(i1.cpu().numpy()[rows], oi) and np.array_equal(v1.cpu().numpy()[rows], ov)


def test_index_keeps_the_callers_tensor(tt):
    """No widened copy and no shadow: building the index over a 1M x 256 bf16 matrix allocates (next to) nothing."""
    Db = bf16_rows(11, 1_000_000, 256)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    ix = tt.BruteForceIndex(Db, screen=True)
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() - before < (1 << 20)
    assert ix.docs.data_ptr() == Db.data_ptr() and ix.docs.dtype == torch.bfloat16 and ix.ntotal == 1_000_000
    Q = queries(12, 64, 256)
    assert_same(ix.search(Q, 10), tt.score_topk(Q, Db.float(), 10))


def test_stats_pass_equals_the_widening_build(tt):
    """tt_index_stats_bf16 (no copy) == tt_index_build_from_bf16's statistics, across calls and with reset."""
    from twotowermlretrieval_amd import _lib
    L = _lib.lib()
    Db = bf16_rows(9, 100_003, 256)
    Db[77, 3] = 512.0
    st = torch.cuda.current_stream().cuda_stream
    a = torch.full((2,), 7.0, device="cuda")
    b = torch.zeros(2, device="cuda")
    d32 = torch.empty((100_003, 256), device="cuda")
    _lib.check(L.tt_index_stats_bf16(Db.data_ptr(), 60_000, 256, a.data_ptr(), 1, st))
    _lib.check(L.tt_index_stats_bf16(Db[60_000:].data_ptr(), 40_003, 256, a.data_ptr(), 0, st))
    _lib.check(L.tt_index_build_from_bf16(Db.data_ptr(), 100_003, 256, d32.data_ptr(), None, b.data_ptr(), 1, st))
    torch.cuda.synchronize()
    assert torch.equal(a, b) and float(a[1]) == 512.0


@pytest.mark.parametrize("form", (0, 1, 2, 4))
@pytest.mark.parametrize("with_thr", (False, True))
def test_debug_screen_bf16_is_bitwise_the_shadow_screen(tt, form, with_thr):
    """The screen kernels over bf16 rows (converted in LDS) see exactly the fp16 shadow of the widened rows: the raw tile
    maxima of tt_debug_screen_s16_bf16 == tt_debug_screen_s16 over tt_index_build_f16(widened), bit for bit."""
    from twotowermlretrieval_amd import _lib
    L = _lib.lib()
    f = C.CDLL(L._name)
    for name in ("tt_debug_screen_s16", "tt_debug_screen_s16_bf16"):
        getattr(f, name).restype = C.c_int
        getattr(f, name).argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_float, C.c_void_p, C.c_int, C.c_void_p,
                                     C.c_void_p, C.c_size_t, C.c_void_p]
    B, N = (40 if form == 0 else 130), 20_000
    Db = bf16_rows(50 + form, N, 256)
    # bf16 -> fp16 rounds only below fp16's normal range: rows of subnormal and underflowing magnitudes, and large elements
    Db[5:37] = (torch.randn((32, 256), device="cuda") * 2.0e-5).to(torch.bfloat16)
    Db[40, :8] = 40000.0
    Q = queries(51 + form, B, 256)
    st = torch.cuda.current_stream().cuda_stream
    w = Db.float()
    d16 = torch.empty((N, 256), dtype=torch.float16, device="cuda")
    stats = torch.zeros(2, device="cuda")
    _lib.check(L.tt_index_build_f16(w.data_ptr(), N, 256, d16.data_ptr(), stats.data_ptr(), st))
    dmax = float(stats[0])
    thr = (torch.rand(B, device="cuda") * 0.2 - 0.1) if with_thr else None
    f.tt_debug_screen_s16_workspace_bytes.restype = C.c_size_t
    f.tt_debug_screen_s16_workspace_bytes.argtypes = [C.c_int, C.c_int64, C.c_int]
    ws = torch.empty(f.tt_debug_screen_s16_workspace_bytes(B, N, form), dtype=torch.uint8, device="cuda")
    outs = []
    for name, D in (("tt_debug_screen_s16", d16), ("tt_debug_screen_s16_bf16", Db)):
        out = torch.full((B, (N + 31) // 32), float("nan"), device="cuda")
        _lib.check(getattr(f, name)(Q.data_ptr(), B, D.data_ptr(), N, dmax, thr.data_ptr() if thr is not None else None,
                                    form, out.data_ptr(), ws.data_ptr(), ws.numel(), st))
        torch.cuda.synchronize()
        outs.append(out.view(torch.int32).clone())
    assert torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("B", (1, 7, 32, 64, 65, 256, 1024))
def test_index_search_equals_f32_index(tt, B):
    N = (65_536, 300_007, 1_000_003)[B % 3]
    Db = bf16_rows(20 + B, N, 256)
    Q = queries(21 + B, B, 256)
    ix = tt.BruteForceIndex(Db, screen=True)
    ref = tt.BruteForceIndex(Db.float(), screen=True)
    assert ix._screen_bf16 and ix.docs16 is None and ix.dmax_norm == ref.dmax_norm
    ix.keep_stats = ref.keep_stats = True
    got = ix.search(Q, 10)
    assert_same(got, ref.search(Q, 10))
    assert torch.equal(ix.search_stats(), ref.search_stats())
    assert torch.equal(ix.fallback_flags, ref.fallback_flags)
    out = (torch.empty((B, 10), device="cuda"), torch.empty((B, 10), dtype=torch.int64, device="cuda"))
    r = ix.search(Q, 10, out=out)
    assert r[0].data_ptr() == out[0].data_ptr() and r[1].data_ptr() == out[1].data_ptr()
    assert_same(out, got)
    v1, i1 = ix.search(Q[0], 10)
    assert torch.equal(i1, got[1][0]) and torch.equal(v1, got[0][0])


def test_clustered_corpus_rounded_to_bf16(tt, oracle):
    """bench.py's clustered corpus (near-duplicates and groups of exact ties larger than any survivor list), rounded to bf16:
    the screen must give up on the duplicate groups' tiles exactly where the shadow index does, and the exact bf16 kernel
    must take over."""
    import bench
    B = 160
    D, Q, _ = bench.make_clustered_corpus(200_000, B, torch.device("cuda"), seed=5, n_centres=1333, dup_groups=30, dup=1100)
    Db = D.to(torch.bfloat16)
    ix = tt.BruteForceIndex(Db, screen=True)
    ref = tt.BruteForceIndex(Db.float(), screen=True)
    assert ix._screen_bf16
    ix.keep_stats = ref.keep_stats = True
    for nq in (B, 40):
        got = ix.search(Q[:nq].contiguous(), 10)
        assert_same(got, ref.search(Q[:nq].contiguous(), 10))
        assert int(ix.fallback_flags.ne(0).sum()) > 0
        assert torch.equal(ix.fallback_flags, ref.fallback_flags)
        assert torch.equal(ix.search_stats(), ref.search_stats())
    got = ix.search(Q, 10)
    rows = np.arange(0, B, 11)
    ov, oi = oracle_rows(oracle, Q.cpu().numpy(), widened(Db), 10, rows)
    assert np.array_equal(got[1].cpu().numpy()[rows], oi) and np.array_equal(got[0].cpu().numpy()[rows], ov)


def test_graphed_search_and_streamed_resident(tt):
    N, d = 150_000, 256
    Db = bf16_rows(31, N, d)
    host = Db.cpu()
    Q = queries(32, 48, d)
    ix = tt.BruteForceIndex(Db, idx_offset=1000, screen=True)
    assert ix._screen_bf16
    want = ix.search(Q, 10)
    g = tt.GraphedSearch(ix, 48, 10)
    assert_same(g(Q), want)
    assert_same(tt.BruteForceIndex(Db, idx_offset=1000).search(Q, 10), want)     # the exact bf16 kernel
    st = tt.StreamedIndex(host, block_docs=1 << 16, idx_offset=1000)
    res = st.resident(dtype=torch.bfloat16)
    assert res.docs.dtype == torch.bfloat16 and res.idx_offset == 1000
    assert_same(res.search(Q, 10), want)
    assert_same(st.search(Q, 10), want)
    assert_same(st.resident().search(Q, 10), want)     # the default is unchanged: fp32 (+ shadow)


def test_full_12m5_shard(tt, oracle):
    """BASELINE configs[4]'s shard, 12.5M x 256 bf16 (6.4 GB), resident as bf16: == StreamedIndex over the same host rows ==
    the oracle (on a few queries, over the rows widened on the CPU block by block)."""
    N, d = 12_500_000, 256
    Db = bf16_rows(41, N, d)
    Q32 = queries(42, 1024, d)
    planted = {0: 0, 1: 6_250_000, 2: N - 1, 3: 123_457}       # query -> row holding (the bf16 rounding of) that query
    for q, r in planted.items():
        Db[r] = Q32[q].to(torch.bfloat16)
    host = Db.cpu()
    ix = tt.BruteForceIndex(Db, idx_offset=7, screen=True)
    assert ix._screen_bf16
    st = tt.StreamedIndex(host, idx_offset=7)
    for B in (32, 1024):
        got = ix.search(Q32[:B], 10)
        assert_same(got, st.search(Q32[:B], 10))
        for q, r in planted.items():
            assert int(got[1][q, 0]) == r + 7
    del st
    rows = np.array([0, 1, 2, 3, 500, 1023])
    Qn = Q32.cpu().numpy()
    blk = 1 << 21
    bv, bi = [], []
    for lo in range(0, N, blk):
        v, i = oracle_rows(oracle, Qn, host[lo:lo + blk].float().numpy(), 10, rows, 7 + lo)
        bv.append(v)
        bi.append(i)
    v, i = np.concatenate(bv, 1), np.concatenate(bi, 1)
    order = np.lexsort((i, -v), axis=1)[:, :10]                # score desc, index asc
    ov, oi = np.take_along_axis(v, order, 1), np.take_along_axis(i, order, 1)
    got = ix.search(Q32, 10)
    assert np.array_equal(got[1].cpu().numpy()[rows], oi) and np.array_equal(got[0].cpu().numpy()[rows], ov)
