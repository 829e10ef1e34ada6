"""The screened path (fp16 MFMA filter + exact fp32 rescoring, csrc/screen.hip) must return exactly
what the exact kernel and the oracle return: bit-identical scores, identical indices and tie order --
including when near-tie clusters force the on-device fallback to the exact kernel."""
import numpy as np
import pytest
import torch

import synth

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def screened(tt, Q, D, k, off=0):
    from twotowermlretrieval_amd import index as _index
    _index.SCREEN_MIN_DOCS = 0  # these tests exercise the screened kernels on small corpora too
    ix = tt.BruteForceIndex(dev(D), idx_offset=off, screen=True)
    assert ix.docs16 is not None
    v, i = ix.search(dev(Q), k)
    torch.cuda.synchronize()
    return v.cpu().numpy(), i.cpu().numpy(), int(ix.fallback_flags[:(len(Q) + 31) // 32].ne(0).sum().item())


@pytest.fixture(scope="module")
def tt():
    import twotowermlretrieval_amd as m
    return m


@pytest.mark.parametrize("B,N,k", [(128, 5000, 10), (200, 33333, 10), (600, 20000, 16), (97, 1000, 1), (513, 4097, 5),
                                   (130, 9000, 50), (96, 700000, 64), (33, 70000, 10), (250, 66000, 10), (256, 3000, 7),
                                   # the 384-query groups (NSET = 3): one group, a ragged last wave, two and three groups
                                   (257, 40000, 10), (384, 70001, 10), (300, 9000, 33), (768, 66000, 10), (700, 250000, 10),
                                   (1025, 30000, 8)])
def test_bit_exact_vs_oracle(tt, oracle, B, N, k):
    Q = synth.unit_rows(100 + B, B, 256)
    D = synth.unit_rows(200 + N, N, 256)
    v, i, flag = screened(tt, Q, D, k, off=7)
    ov, oi = oracle.score_topk(Q, D, k, idx_offset=7)
    assert np.array_equal(i, oi) and np.array_equal(v, ov)
    assert flag == 0


@pytest.mark.parametrize("B,N,k", [(1, 5000, 10), (7, 33333, 10), (16, 20000, 16), (17, 1000, 1), (32, 4097, 5),
                                   (33, 9000, 50), (64, 700000, 64), (1, 300000, 10), (32, 31, 8), (48, 120000, 10),
                                   (64, 250000, 50), (40, 31, 8), (49, 65600, 3)])
def test_small_batch_streaming_form_bit_exact_vs_oracle(tt, oracle, B, N, k):
    """B <= 64 runs screen_stream_kernel (one wave per query tile -- 32 queries up to B = 32, 64 above -- and document chunk)."""
    Q = synth.unit_rows(300 + B, B, 256)
    D = synth.unit_rows(400 + N, N, 256)
    k = min(k, N)
    v, i, flag = screened(tt, Q, D, k, off=11)
    ov, oi = oracle.score_topk(Q, D, k, idx_offset=11)
    assert np.array_equal(i, oi) and np.array_equal(v, ov)
    assert flag == 0


def test_single_query_vector_goes_through_the_screened_index(tt, oracle):
    D = synth.unit_rows(77, 50000, 256)
    q = synth.unit_rows(78, 1, 256)[0]
    ix = tt.BruteForceIndex(torch.from_numpy(D).cuda(), screen=True)
    v, i = ix.search(torch.from_numpy(q).cuda(), 10)
    ov, oi = oracle.score_topk(q[None], D, 10)
    assert v.shape == (10,) and np.array_equal(i.cpu().numpy(), oi[0]) and np.array_equal(v.cpu().numpy(), ov[0])


def test_non_unit_norms_and_scaled_data(tt, oracle):
    rs = np.random.RandomState(3)
    Q = (synth.unit_rows(1, 130, 256) * rs.uniform(0.1, 5.0, (130, 1))).astype(np.float32)
    D = (synth.unit_rows(2, 9000, 256) * rs.uniform(0.5, 3.0, (9000, 1))).astype(np.float32)
    v, i, flag = screened(tt, Q, D, 10)
    ov, oi = oracle.score_topk(Q, D, 10)
    assert np.array_equal(i, oi) and np.array_equal(v, ov) and flag == 0


def test_near_ties_below_fp16_resolution_are_resolved_exactly(tt, oracle):
    # 40 documents within 1e-6 of each other around every query's best score: fp16 cannot order
    # them, the exact rescoring must.
    rs = np.random.RandomState(5)
    Q = synth.unit_rows(11, 128, 256)
    D = synth.unit_rows(12, 6000, 256).copy()
    for b in range(0, 128, 4):
        for c in range(40):
            x = Q[b] + rs.standard_normal(256).astype(np.float32) * 2e-6
            D[100 + (b // 4) * 40 + c] = x / np.linalg.norm(x)
    v, i, flag = screened(tt, Q, D, 10)
    ov, oi = oracle.score_topk(Q, D, 10)
    assert np.array_equal(i, oi) and np.array_equal(v, ov)
    # (the 40-document clusters also tie for OTHER queries; where two clusters land within 2 eps of a
    # workgroup's k-th score the candidate buffer overflows and that 32-query tile is recomputed exactly)
    assert flag <= 4


def test_tie_cluster_overflow_triggers_exact_fallback_on_device(tt, oracle):
    # 1400 exact copies of one document: more tied survivors than the finish kernel's list holds (SURV_MAX = 1024) -> the flag
    # is raised on the device and the predicated exact kernel rewrites the result (index-ascending ties).  400 copies -- what
    # overflowed the round-3 list of 256 -- are rescored by the screen itself now: no fallback, same exact result.
    Q = synth.unit_rows(21, 128, 256)
    for copies, falls_back in ((1400, True), (400, False)):
        D = synth.unit_rows(22, 5000, 256).copy()
        D[1000:1000 + copies] = Q[5]
        v, i, flag = screened(tt, Q, D, 10)
        ov, oi = oracle.score_topk(Q, D, 10)
        assert (flag >= 1) == falls_back, (copies, flag)
        assert np.array_equal(i, oi) and np.array_equal(v, ov)
        assert list(i[5]) == list(range(1000, 1010))


def test_matches_exact_kernel_at_1m(tt):
    g = torch.Generator(device="cuda").manual_seed(3)
    N, B = 1_000_000, 1024
    D = torch.randn(N, 256, device="cuda", generator=g)
    D /= D.norm(dim=1, keepdim=True)
    Q = torch.randn(B, 256, device="cuda", generator=g)
    Q /= Q.norm(dim=1, keepdim=True)
    ev, ei = tt.score_topk(Q, D, 10)
    ix = tt.BruteForceIndex(D, screen=True)
    sv, si = ix.search(Q, 10)
    torch.cuda.synchronize()
    assert int(ix.fallback_flags.ne(0).sum().item()) == 0
    assert torch.equal(si, ei) and torch.equal(sv, ev)


def test_out_of_range_corpus_disables_screen(tt, oracle):
    D = synth.unit_rows(31, 3000, 256) * np.float32(1e5)
    Q = synth.unit_rows(32, 128, 256)
    ix = tt.BruteForceIndex(dev(D), screen=True)
    assert ix.docs16 is None
    v, i = ix.search(dev(Q), 10)
    ov, oi = oracle.score_topk(Q, D, 10)
    assert np.array_equal(i.cpu().numpy(), oi) and np.array_equal(v.cpu().numpy(), ov)


def test_graphed_search_replays_bit_identically(tt, oracle):
    """GraphedSearch: a whole screened search captured in a HIP graph; new queries through the static buffer."""
    from twotowermlretrieval_amd import index as _index
    _index.SCREEN_MIN_DOCS = 0
    D = synth.unit_rows(91, 70000, 256)
    ix = tt.BruteForceIndex(dev(D), screen=True)
    gs = tt.GraphedSearch(ix, batch=4, k=10)
    for seed in (92, 93):
        Q = synth.unit_rows(seed, 4, 256)
        v, i = gs(dev(Q))
        torch.cuda.synchronize()
        ov, oi = oracle.score_topk(Q, D, 10)
        assert np.array_equal(i.cpu().numpy(), oi) and np.array_equal(v.cpu().numpy(), ov)
    with pytest.raises(ValueError):
        gs(dev(synth.unit_rows(1, 5, 256)))


def test_full_baseline_size_10m_screened_equals_exact_kernel(tt, oracle):
    """BASELINE configs[3] size (10M x 256): the screened index (shared-tile form at B=1024, streaming form at
    B=32) returns exactly what the plain fp32 kernel returns, planted documents come back at rank 1, and nothing
    falls back to the exact path.  Six queries per form -- planted and not, first and last of the batch, both
    512-query groups -- are also checked against the CPU oracle over all 10M rows, which pins the bench-size launch
    geometry (255 chunks, sample pass, two query groups) to the oracle directly, not only to the other HIP kernel."""
    import sys
    from pathlib import Path
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
    import bench
    devc = torch.device("cuda:0")
    D = bench.gen_rows(0, bench.N_DOCS, devc)
    Q = bench.gen_queries(1024, devc, seed=99)
    planted = torch.tensor([0, 31, 4_999_999, 9_999_999], device=devc)
    D[planted] = Q[:4]                      # queries 0..3 have an exact copy in the corpus
    ix = tt.BruteForceIndex(D, screen=True)
    results = {}
    for B in (1024, 32):
        sv, si = ix.search(Q[:B].contiguous(), 10)
        ev, ei = tt.score_topk(Q[:B].contiguous(), D, 10)
        torch.cuda.synchronize()
        assert int(ix.fallback_flags[:(B + 31) // 32].ne(0).sum().item()) == 0
        assert torch.equal(si, ei) and torch.equal(sv, ev)
        assert si[:4, 0].tolist() == planted.tolist() and bool((sv[:4, 0] - 1.0).abs().max() < 1e-5)
        assert bool((sv[:, 1:] <= sv[:, :-1]).all())
        results[B] = (sv.cpu().numpy(), si.cpu().numpy())
    Dh = D.cpu().numpy()
    Qh = Q.cpu().numpy()
    from concurrent.futures import ThreadPoolExecutor
    checks = [(B, r) for B, rows in ((1024, [0, 3, 5, 511, 512, 1023]), (32, [0, 2, 4, 15, 16, 31])) for r in rows]
    with ThreadPoolExecutor(max_workers=12) as pool:  # one scalar fmaf chain per (query, document): ~3 s per query
        outs = list(pool.map(lambda br: oracle.score_topk(Qh[br[1]:br[1] + 1], Dh, 10), checks))
    for (B, r), (ov, oi) in zip(checks, outs):
        assert np.array_equal(results[B][1][r], oi[0]) and np.array_equal(results[B][0][r], ov[0]), f"B={B} query {r} vs oracle"
    del ix, D, Dh
    torch.cuda.empty_cache()


@pytest.mark.parametrize("B", [4, 50, 80])
def test_query_beyond_fp16_range_goes_to_the_exact_kernel(tt, oracle, B):
    """A query with an element fp16 cannot hold (|x| > 6e4) raises flag bit 2 for its 32-query tile in
    q_image_kernel; the exact kernel recomputes that tile on the device; the other tiles stay screened."""
    D = synth.unit_rows(51, 70000, 256)
    Q = synth.unit_rows(52, B, 256).copy()
    Q[1] *= 1.0e6
    v, i, flag = screened(tt, Q, D, 10)
    ov, oi = oracle.score_topk(Q, D, 10)
    assert np.array_equal(i, oi) and np.array_equal(v, ov)
    assert flag == 1     # exactly the tile holding query 1


@pytest.mark.parametrize("d,B", [(128, 100), (64, 600), (200, 40), (128, 8)])
def test_narrower_embeddings_through_the_zero_padded_screen(tt, oracle, d, B):
    """HIDDEN_DIM < 256: batches above 32 run the screen on a zero-padded copy (bit-identical: the extra chain terms
    are fmaf(0, 0, acc)); B <= 32 streams the original rows through the exact kernel."""
    from twotowermlretrieval_amd import index as _index
    _index.SCREEN_MIN_DOCS = 0
    Q = synth.unit_rows(71, B, d)
    D = synth.unit_rows(72, 30000, d)
    ix = tt.BruteForceIndex(dev(D), idx_offset=3, screen=True)
    assert ix.docs16 is not None and tuple(ix.docs16.shape) == (30000, 256)
    v, i = ix.search(dev(Q), 10)
    torch.cuda.synchronize()
    k4v, k4i = tt.score_topk(dev(Q), dev(D), 10, 3) if d in (32, 64, 96, 128, 192) else (None, None)
    ov, oi = oracle.score_topk(Q, D, 10, idx_offset=3)
    assert np.array_equal(i.cpu().numpy(), oi) and np.array_equal(v.cpu().numpy(), ov)
    if k4v is not None:
        assert torch.equal(k4v, v) and torch.equal(k4i, i)


def test_100m_rows_resident_on_one_gpu(tt):
    """BASELINE configs[4]'s whole corpus (100M x 256) on ONE 288 GB GPU: fp32 rows + fp16 shadow = 153.6 GB.  3.1 M document
    tiles per query group: the largest launch geometry any test drives.  The screened index returns exactly what the plain fp32
    kernel returns (a serving batch: all 32 queries; the bench batch: its first 64, through a second exact call), planted documents
    -- first row, last row, two in between -- come back at rank 1, nothing falls back."""
    import sys
    from pathlib import Path
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
    import bench
    devc = torch.device("cuda:0")
    torch.cuda.empty_cache()        # (blocks the earlier tests left in the caching allocator count as used)
    free_b, _ = torch.cuda.mem_get_info(devc)
    if free_b < 170e9:
        pytest.skip("needs 170 GB of free HBM")
    N = 100_000_000
    D = bench.gen_rows(0, N, devc)
    Q = bench.gen_queries(1024, devc, seed=41)
    planted = torch.tensor([0, 31, 50_000_001, N - 1], device=devc)
    D[planted] = Q[:4]
    ix = tt.BruteForceIndex(D, screen=True)
    assert ix.docs16 is not None and ix.ntotal == N
    sv, si = ix.search(Q, 10)
    assert int(ix.fallback_flags.ne(0).sum().item()) == 0
    assert si[:4, 0].tolist() == planted.tolist() and bool((sv[:4, 0] - 1.0).abs().max() < 1e-5)
    assert bool((sv[:, 1:] <= sv[:, :-1]).all()) and int(si.min()) >= 0 and int(si.max()) < N
    ev, ei = tt.score_topk(Q[:64].contiguous(), D, 10)
    assert torch.equal(si[:64], ei) and torch.equal(sv[:64], ev)
    v32, i32 = ix.search(Q[:32].contiguous(), 10)                 # the streaming form
    assert torch.equal(i32, ei[:32]) and torch.equal(v32, ev[:32])
    del ix, D
    torch.cuda.empty_cache()


# ---- one screened call site for every corpus layout (index._Screen) ----
LAYOUT_N, LAYOUT_B, LAYOUT_K, LAYOUT_OFF = 65536, 33, 10, 9


@pytest.fixture(scope="module")
def layouts(oracle):
    """layout -> (device rows, Q, the oracle's top-k over the fp32-widened rows), computed once for both search forms."""
    made = {}

    def get(layout):
        if layout not in made:
            d = 128 if layout == "f32_d128_padded" else 256
            D = synth.unit_rows(500 + d, LAYOUT_N, d)
            rows = dev(D).to(torch.bfloat16) if layout == "bf16_d256" else dev(D)
            Q = synth.unit_rows(600 + d, LAYOUT_B, d)
            made[layout] = (rows, Q, oracle.score_topk(Q, rows.float().cpu().numpy(), LAYOUT_K, idx_offset=LAYOUT_OFF))
        return made[layout]

    yield get
    made.clear()


@pytest.mark.parametrize("form", ["index", "sharded_world1"])
@pytest.mark.parametrize("layout", ["f32_d256", "f32_d128_padded", "bf16_d256"])
def test_every_layout_screens_through_the_same_calls(tt, layouts, monkeypatch, layout, form):
    """The smallest shapes that still screen with the product thresholds: N = SCREEN_MIN_DOCS rows, B = 33 (the smallest
    batch at which the padded layout screens; two 32-query tiles).  BruteForceIndex.search makes the whole-search call; a
    world-1 ShardedIndex with shard_k > k makes the seed-list + seeded calls where the seed exchange applies (d = 256) and the
    whole-search call for the padded layout.  Every result is the oracle's over the fp32-widened rows, bit for bit."""
    from twotowermlretrieval_amd import index as _index
    monkeypatch.setattr(_index, "SCREEN_MIN_DOCS", 65536)  # the product values (other tests lower them)
    monkeypatch.setattr(_index, "SCREEN_MIN_BATCH", 1)
    monkeypatch.setattr(_index, "SCREEN_PADDED_MIN_BATCH", 33)
    rows, Q, (ov, oi) = layouts(layout)
    if form == "index":
        ix = top = tt.BruteForceIndex(rows, idx_offset=LAYOUT_OFF, screen=True)
    else:
        top = tt.ShardedIndex(rows, LAYOUT_OFF, shard_k=50, screen=True)
        ix = top._index
        assert top._seed_exchange is (layout != "f32_d128_padded")
    assert ix._screens(LAYOUT_B, LAYOUT_K) and ix._screens(LAYOUT_B, 50)
    assert ix._screen_bf16 is (layout == "bf16_d256") and (ix.docs16 is None) is (layout == "bf16_d256")
    v, i = top.search(dev(Q), LAYOUT_K)
    torch.cuda.synchronize()
    assert np.array_equal(i.cpu().numpy(), oi) and np.array_equal(v.cpu().numpy(), ov)
    assert ix.fallback_flags.shape[0] == 2 and int(ix.fallback_flags.ne(0).sum().item()) == 0
