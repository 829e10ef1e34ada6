"""Threshold refresh of the shared-tile screened search (csrc/screen.hip, "Refresh"): mid-pass, every workgroup raises its queries'
thresholds to what the chip as a whole has counted on the per-query ladders.  The refresh may only ever change how many
candidates are pooled, never a result, so every comparison here is `==` on scores and indices against the exact kernel (and the
CPU oracle on a few rows).  The product gates the refresh to chunks of REFRESH_MIN_TILES = 1024 tiles; the comparison build
lowers the gate (TT_SCREEN_REFRESH_MIN_TILES=8) so that corpora of 300 007 rows take the path, and hands out the last HALF of
every chunk in pool blocks (TT_SCREEN_TAIL_DIV=2; the product's eighth would be under tt_tail_split's 16-tile minimum here), so
that the refresh in front of a pool draw runs in every form: at k = 10 a chunk is 37 tiles (B up to 512: 254 chunks), 19 of them
its own range with checkpoints 2, 4 and 8 tiles in, and the 4 550 tiles behind tile 4 826 are 569 pool blocks of 8.  plan()
mirrors make_splan's figures; every test asserts that its plan has pool blocks."""
import numpy as np
import pytest
import torch

from conftest import ab_library
from test_masked_gpu import expected, host_f32, queries, rows_on_device

pytestmark = pytest.mark.gpu

N = 300_007                      # a ragged last tile; 9 376 tiles
TAIL_DIV = 2
ON = dict(TT_SCREEN_REFRESH_MIN_TILES=8, TT_SCREEN_TAIL_DIV=TAIL_DIV)
OFF = dict(TT_SCREEN_REFRESH_MIN_TILES=8, TT_SCREEN_TAIL_DIV=TAIL_DIV, TT_SCREEN_THR_REFRESH=0)


@pytest.fixture(scope="module")
def tt():
    import twotowermlretrieval_amd as m
    from twotowermlretrieval_amd import _lib
    _lib.lib()
    assert torch.cuda.is_available()
    return m


@pytest.fixture(autouse=True)
def product_thresholds(monkeypatch):
    """The routing thresholds of the product (other test modules lower them for the rest of the session)."""
    from twotowermlretrieval_amd import index as _index
    monkeypatch.setattr(_index, "SCREEN_MIN_DOCS", 65536)
    monkeypatch.setattr(_index, "SCREEN_MIN_BATCH", 1)
    monkeypatch.setattr(_index, "SCREEN_PADDED_MIN_BATCH", 33)


def flagged(ix):
    return int(ix.fallback_flags.ne(0).sum())


def pooled_mean(ix):
    return float(ix.search_stats()[:, 0].float().mean())


def same(a, b):
    return torch.equal(a[1], b[1]) and torch.equal(a[0], b[0])


def plan(n_rows, n_qgroups, k, div=TAIL_DIV, cus=256):
    """The shared-tile plan's figures (make_splan: tt_chunks for one round of workgroups, at most 255 chunks and
    POOL_MAX / (k + 16); tt_tail_split(div, min_share 16, blocks of 8 .. 32 tiles)): tiles per chunk, the own range of a chunk,
    the tiles cut statically, tiles per pool block, pool blocks."""
    n_tiles = (n_rows + 31) // 32
    want = min((cus + n_qgroups - 1) // n_qgroups, 255, 8192 // (k + 16), n_tiles)
    per = (n_tiles + want - 1) // want
    n_chunks = (n_tiles + per - 1) // per
    share = per // div if div > 0 else 0
    if share < 16:
        return dict(per=per, own=per, static_tiles=n_tiles, tail_g=1, tail_blocks=0, n_chunks=n_chunks, n_tiles=n_tiles)
    own, g = per - share, min(max(share // 4, 8), 32)
    static = min(own * n_chunks, n_tiles)
    return dict(per=per, own=own, static_tiles=static, tail_g=g, tail_blocks=(n_tiles - static + g - 1) // g, n_chunks=n_chunks,
                n_tiles=n_tiles)


def n_qgroups(B):
    """Query groups of the shared-tile form (make_splan: 128 NSET queries per workgroup)."""
    if B <= 256:
        return 1
    groups = (B + 511) // 512
    return (B + (384 if (B + groups - 1) // groups <= 384 else 512) - 1) // (384 if (B + groups - 1) // groups <= 384 else 512)


def on_off(ix, Q, k, **kw):
    """One search with the refresh and one without (both with the lowered gate and the half-chunk pool): results, flagged tiles
    and mean pooled candidates per query of each."""
    out = []
    for env in (ON, OFF):
        with ab_library(**env):
            got = ix.search(Q, k, **kw)
            torch.cuda.synchronize()
            out.append((got, ix.fallback_flags.clone(), pooled_mean(ix)))
    return out


# ---- 1. equal to the exact kernel ----------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def corpora(tt):
    """bf16 -> (device rows, host fp32 rows, index, packed mask with holes in every tile, the mask), made once."""
    made = {}

    def get(bf16):
        if bf16 not in made:
            D = rows_on_device(4100 + int(bf16), N, 256, bf16)
            ix = tt.BruteForceIndex(D, screen=True, screen_masked=True)
            ix.keep_stats = True
            mask = np.random.RandomState(5).rand(N) < 0.7
            mask[3::32] = False                              # a hole in every 32-document tile
            keep = tt.pack_keep_mask(torch.from_numpy(mask).cuda())
            made[bf16] = (D, host_f32(D), ix, keep, mask)
        return made[bf16]

    yield get
    made.clear()
    torch.cuda.empty_cache()


# B -> NSET 1, 3 (a ragged last wave: 300 = 6 waves of 48 + 12) and 4 (two query groups)
@pytest.mark.parametrize("variant", ("f32", "bf16", "masked"))
@pytest.mark.parametrize("k", (1, 10, 64))
@pytest.mark.parametrize("B", (65, 300, 1024))
def test_refreshed_search_equals_the_exact_kernel(tt, oracle, corpora, B, k, variant):
    D, Dn, ix, keep, mask = corpora(variant == "bf16")
    if variant != "masked":
        keep, mask = None, np.ones(N, dtype=bool)
    Q = queries(4200 + B, B, 256)
    assert ix._screens(B, k, keep is not None)
    pl = plan(N, n_qgroups(B), k)
    assert pl["tail_blocks"] > 0 and pl["own"] >= 8, pl
    (got, flags, on), (off_got, _, off) = on_off(ix, Q, k, keep=keep)
    print(f"B={B} k={k} {variant}: pooled candidates per query {on:.2f} with refresh, {off:.2f} without; plan {pl}")
    assert int(flags.ne(0).sum()) == 0                       # random rows: the screen's own answer, not the fallback's
    assert on < off                                          # the refresh ran
    ref = tt.score_topk(Q, ix.docs, k, keep=keep)
    torch.cuda.synchronize()
    assert same(got, ref) and same(off_got, ref)
    rows = np.array([0, B // 2, B - 1])
    ov, oi = expected(oracle, Q.cpu().numpy(), Dn, mask, k, rows)
    assert np.array_equal(got[1].cpu().numpy()[rows], oi) and np.array_equal(got[0].cpu().numpy()[rows], ov)


# ---- 2. late arrivals behind a high threshold ----------------------------------------------------------------------------------

def test_late_arrivals_behind_a_raised_threshold(tt, oracle):
    """The k-th place arrives late, inside the ladder's span, as close above a refreshed threshold as exact scores can put it.
    Per planted query, with base = its seed (host estimate: the k-th best exact score over the 40 960 sample rows; the ladder's
    base is the seed itself), eps_q from |q| and the largest row norm, w = 4 eps_q: k - 1 strong documents at base + 10.5 w ..
    11.3 w in the first two tiles of own ranges of their own, in front of the first checkpoint; a group of 3k documents whose
    exact scores lie within 1e-4 of each other at base + 9.1 w, just above the writer's boundary of level 9 (0.1 w against an
    estimate good to ~0.02 w), which holds the k-th place: a third in tiles 2 .. 7 of own ranges, a third behind the last
    checkpoint (tiles 9 .. 18), a third in pool blocks.  Once the early third is counted, level 9 holds k documents and every
    threshold of that query stands at e_9 - 2 eps = base + 8.25 w, 0.85 w under the late members, which must come back.
    What this catches: a threshold one level too high (base + 9.25 w), counts of a wrong query or level, a lost max in the
    compaction, anything that eats more than 0.85 w = 1.7 x 2 eps of clearance.  What it cannot: a missing `- 2 eps` alone or an
    edge a quarter level up alone (0.35 w of clearance left): those protect against fp16 errors near eps_q, and exact scores
    planted as multiples of the query err by ~1e-5.  One row of norm 3, orthogonal to the planted queries, widens eps_q so that
    the ladder's span (15 w = 0.2) reaches above every random score (<= 0.29)."""
    B, k = 300, 10
    pl = plan(N, 1, k)
    own, static = pl["own"], pl["static_tiles"]
    assert pl["tail_blocks"] > 0 and own == 19, pl            # checkpoints 2, 4, 8 tiles into an own range
    D = rows_on_device(4300, N, 256)
    Q = queries(4301, B, 256)
    planted = (0, 151, 299)
    rs = np.random.RandomState(6)
    big = torch.from_numpy(rs.standard_normal(256).astype(np.float32)).cuda()
    for _ in range(2):                                       # orthogonal to the planted queries (their scores with it: ~1e-8)
        for q in planted:
            big -= (big @ Q[q]) * Q[q]
    D[N - 5] = 3.0 * big / big.norm()
    dmax = float(torch.linalg.vector_norm(D, dim=1).max())
    assert 2.99 < dmax < 3.01
    s_rows = 40_960
    first_chunk = s_rows // (32 * own) + 2                   # own ranges past the sample: the seed stays the random rows'
    kth = {}
    for a, q in enumerate(planted):
        base = float((D[:s_rows] @ Q[q]).topk(k).values[-1])
        eps = 1.10e-3 * float(Q[q].norm()) * dmax + 1e-6 * (float(Q[q].norm()) + dmax)
        w = 4.0 * eps
        chunks = first_chunk + 60 * a + np.arange(4 * k)
        assert chunks.max() < pl["n_chunks"] - 1
        rows = [(c * own + int(rs.randint(0, 2))) * 32 + int(rs.randint(0, 32)) for c in chunks[:k - 1]]
        scores = [base + (10.5 + 0.1 * j) * w for j in range(k - 1)]
        for j, c in enumerate(chunks[k - 1:k - 1 + 3 * k]):
            t = (c * own + int(rs.randint(2, 8)), c * own + int(rs.randint(9, own)),
                 int(rs.randint(static, pl["n_tiles"] - 1)))[j % 3]
            rows.append(t * 32 + int(rs.randint(0, 32)))
            scores.append(base + 9.1 * w + 1e-4 * float(rs.rand()))
        assert len(set(rows)) == 4 * k - 1 and max(rows) < N - 32 and min(rows) >= s_rows
        assert scores[-1] < base + 9.2 * w and max(scores) < base + 14 * w
        for r, sc in zip(rows, scores):
            D[r] = Q[q] * (sc / float(Q[q] @ Q[q]))
        kth[q] = (base + 9.1 * w, base + 10.4 * w)
    ix = tt.BruteForceIndex(D, screen=True)
    ix.keep_stats = True
    (got, flags, on), (off_got, _, off) = on_off(ix, Q, k)
    print(f"late arrivals: pooled candidates per query {on:.2f} with refresh, {off:.2f} without; plan {pl}")
    assert int(flags.ne(0).sum()) == 0                       # no tile may fall back
    assert on < off
    ref = tt.score_topk(Q, D, k)
    torch.cuda.synchronize()
    assert same(got, ref) and same(off_got, ref)
    ov, oi = expected(oracle, Q.cpu().numpy(), host_f32(D), np.ones(N, dtype=bool), k, np.array(planted))
    assert np.array_equal(got[1].cpu().numpy()[list(planted)], oi) and np.array_equal(got[0].cpu().numpy()[list(planted)], ov)
    for q in planted:                                        # the k-th place IS a member of the group, the strong ones above it
        lo, hi = kth[q]
        assert lo - 1e-5 <= float(got[0][q, k - 1]) <= lo + 1.1e-4 and float(got[0][q, k - 2]) >= hi, (q, got[0][q].tolist(), kth[q])


# ---- 3. a tie group larger than any buffer -------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", (10, 64))
def test_tie_group_larger_than_any_buffer_flags_the_same_tiles(tt, k):
    """test_clustered_corpus_gpu.py's corpus: 1 100 exact duplicates at the top of a query's list overflow the survivor list with
    or without the refresh; the flagged tiles and the results must not depend on it.  k = 10 are that test's parameters: 25-tile
    chunks, too short for pool blocks at any divisor that leaves an own range.  k = 64 (102 chunks of 62 tiles) has them."""
    import bench
    dev = torch.device("cuda:0")
    n, B = 200_000, 160
    pl = plan(n, 1, k)
    assert (pl["tail_blocks"] > 0) == (k == 64), pl
    D, Q, members = bench.make_clustered_corpus(n, B, dev, seed=5, n_centres=1333, dup_groups=30, dup=1100)
    ix = tt.BruteForceIndex(D, screen=True)
    ix.keep_stats = True
    (on, on_flags, on_mean), (off, off_flags, off_mean) = on_off(ix, Q, k)
    print(f"tie group k={k}: flagged tiles {int(on_flags.ne(0).sum())}/{on_flags.numel()} with refresh, {int(off_flags.ne(0).sum())} "
          f"without; pooled candidates per query {on_mean:.2f} / {off_mean:.2f}; plan {pl}")
    assert torch.equal(on_flags.ne(0), off_flags.ne(0)) and int(on_flags.ne(0).sum()) >= 1
    # k = 10: nothing can tighten, and the counts are equal.  The sample is a fifth of this corpus, so a query's seed already
    # is the 10th best of its own cluster (or the duplicates' common score), and every member of the cluster or tie group lies
    # within w = 4 eps of it: level 0, the initial threshold.  k = 64 seeds lower (64th of the sample) and the ladder climbs.
    assert on_mean < off_mean if k == 64 else on_mean <= off_mean
    assert same(on, off)
    assert same(on, tt.score_topk(Q, D, k))


# ---- 4. the ladder counts kept documents only ----------------------------------------------------------------------------------

@pytest.mark.parametrize("bf16", (False, True))
def test_refresh_sees_the_mask(tt, oracle, bf16):
    """The planting of test_threshold_passes_see_the_mask, moved behind the sample: every query's k best documents (scores >= 2)
    sit in the first tiles of chunks of their own and are masked, every kept score is < 1.  A ladder that counted masked
    documents would stand at 2 from the first checkpoint on and the kept documents scored behind it would be dropped."""
    B, k = 70, 10
    pl = plan(N, 1, k)
    assert pl["tail_blocks"] > 0, pl
    per = pl["own"]                                          # chunk c's own range starts at tile c * own
    D = rows_on_device(4400, N, 256, bf16)
    Q = queries(4401, B, 256)
    mask = np.ones(N, dtype=bool)
    first_chunk = 40_960 // (32 * per) + 2
    n_chunks = pl["n_chunks"] - first_chunk - 1
    assert n_chunks * 4 >= B * k
    for q in range(B):
        for j in range(k):
            i = k * q + j
            r = (first_chunk + i % n_chunks) * per * 32 + (i // n_chunks) * 7 + 1   # tile 0 of the chunk, distinct rows
            assert r % (32 * per) < 32 and mask[r]
            D[r] = (Q[q] * (2.0 + 0.25 * j)).to(D.dtype)
            mask[r] = False
    ix = tt.BruteForceIndex(D, screen=True, screen_masked=True)
    keep = tt.pack_keep_mask(torch.from_numpy(mask).cuda())
    ix.keep_stats = True
    with ab_library(**ON):
        assert float(ix.search(Q, k)[0].min()) >= 1.9           # unmasked, the planted rows ARE every query's top-k
    (got, flags, on), (off_got, _, off) = on_off(ix, Q, k, keep=keep)
    print(f"masked plantings: pooled candidates per query {on:.2f} with refresh, {off:.2f} without; plan {pl}")
    assert int(flags.ne(0).sum()) == 0
    assert on < off
    assert same(got, off_got)
    ref = tt.score_topk(Q, ix.docs, k, keep=keep)
    torch.cuda.synchronize()
    assert same(got, ref)
    assert bool((got[1] >= 0).all()) and bool((got[0] < 1.0).all())
    rows = np.array([0, B // 2, B - 1])
    ov, oi = expected(oracle, Q.cpu().numpy(), host_f32(D), mask, k, rows)
    assert np.array_equal(got[1].cpu().numpy()[rows], oi) and np.array_equal(got[0].cpu().numpy()[rows], ov)


# ---- 5. the effect exists (product build) --------------------------------------------------------------------------------------

def test_product_build_pools_fewer_candidates(tt):
    """N = 4 194 304, B = 1024, k = 10: 128 chunks of 1 024 tiles, the product's gate; pool blocks are active (the last eighth)."""
    n, B, k = 4_194_304, 1024, 10
    pl = plan(n, 2, k, div=8)                                # the product's split: the last eighth is the pool
    assert pl["per"] == 1024 and pl["tail_blocks"] > 0, pl
    D = torch.nn.functional.normalize(rows_on_device(4500, n, 256), dim=1)
    Q = queries(4501, B, 256)
    ix = tt.BruteForceIndex(D, screen=True)
    ix.keep_stats = True
    runs, means = [], []
    for _ in range(5):
        runs.append(tuple(t.clone() for t in ix.search(Q, k)))
        torch.cuda.synchronize()
        means.append(pooled_mean(ix))
        assert flagged(ix) == 0
    with ab_library(TT_SCREEN_THR_REFRESH=0):
        off = ix.search(Q, k)
        torch.cuda.synchronize()
        off_mean = pooled_mean(ix)
        assert flagged(ix) == 0
    print(f"pooled candidates per query: {[round(m, 2) for m in means]} with refresh, {off_mean:.2f} without")
    assert all(same(r, runs[0]) for r in runs[1:])
    assert same(runs[0], off)
    assert max(means) < off_mean


# ---- 6. the seeded phase -------------------------------------------------------------------------------------------------------

def test_seeded_phase_refreshes_against_the_list_length(tt):
    """The sharded step's form of the search (bench.screen_kernel_ms): lists of k = 50 seeded for the final k_seed = 10.  The
    refresh compares the ladder with k = 50, which is valid and conservative; the first 10 of every list are the top-10."""
    from twotowermlretrieval_amd.index import _local_seed
    B, k, k_seed = 300, 50, 10
    D = rows_on_device(4600, N, 256)
    Q = queries(4601, B, 256)
    pl = plan(N, 1, k)
    assert pl["tail_blocks"] > 0, pl
    ix = tt.BruteForceIndex(D, screen=True)
    ix.keep_stats = True
    ((v, i), flags, on), (off_got, _, off) = on_off(ix, Q, k, _seed_union=_local_seed, _k_seed=k_seed)
    print(f"seeded k=50 for 10: pooled candidates per query {on:.2f} with refresh, {off:.2f} without; plan {pl}")
    assert int(flags.ne(0).sum()) == 0
    # (<=, not <: the seed is the 10th best of the sample and the ladder waits for 50 counts, so little may tighten here)
    assert on <= off
    assert same((v, i), off_got)
    plain = ix.search(Q, k_seed)
    ref = tt.score_topk(Q, D, k_seed)
    torch.cuda.synchronize()
    cut = (v[:, :k_seed].contiguous(), i[:, :k_seed].contiguous())
    assert same(cut, plain) and same(cut, ref)
