"""Results must not depend on what workspaces and outputs held on entry (DESIGN.md "What a workspace may hold on entry").

libtt.so allocates nothing: the Python host hands it workspaces, outputs, flag, status and count words and seed lists, nearly all
of them from torch.empty -- which in a test process returns fresh (zero) memory or the block of the previous identical call.
Here every case runs once per pattern of poison.PATTERNS with torch.empty and torch.empty_like (the host's gradient outputs,
the table gradient among them) patched to fill what they return (tests/poison.py), through the public Python surface, so that
the host's own buffers are the poisoned ones.  Every pattern's answer is compared
the way the existing test of that entry compares it -- searches bit for bit with the CPU oracle (all rows, or sample_queries
rows where the corpus is large), encoder outputs and gradients with the float64 references at conftest's FWD_ATOL / GRAD_TOL --
and bit for bit with the control pattern's answer.  Of the diagnostics only the deterministic ones are compared: redo flags
(zero), tier words, fallback flags.  Every case asserts from the library's own offset queries (or the diagnostics themselves)
that its shape reaches the mechanism it is named for.  The last two tests pass ONE never-cleared workspace through a sequence of
calls of different shapes: the allocator's real behaviour, a block that holds another call's end state."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

import synth
from conftest import FWD_ATOL, GRAD_TOL, ab_library, assert_fwd_close, assert_grad_close
from poison import CONTROL, PATTERNS, pattern_id, poisoned_empty
from test_masked_gpu import expected, host_f32, queries, rows_on_device
from test_search_aux_gpu import OracleTopk, par_rows, sample_queries

pytestmark = pytest.mark.gpu

SIZE_MAX = C.c_size_t(-1).value
NEG_INF = np.float32(-np.inf)


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
    monkeypatch.setattr(_index, "SCREEN_PADDED_MIN_BATCH", 33)


_CORPORA = {}


def corpus(key, make):
    """Large inputs and their oracle answers, made once and shared by the tests that use them (read-only)."""
    if key not in _CORPORA:
        _CORPORA[key] = make()
    return _CORPORA[key]


@pytest.fixture(scope="module", autouse=True)
def drop_corpora():
    yield
    _CORPORA.clear()
    torch.cuda.empty_cache()


def host(x):
    if isinstance(x, torch.Tensor):
        return x.detach().cpu().numpy()
    return np.asarray(x)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def every_pattern(run, check=None, unordered=()):
    """run() -> {name: tensor} under every pattern; check(results as numpy, word) per pattern; then every pattern's results
    against the control's, bit for bit (but for the names in `unordered`: sums of float atomics, whose last bits follow the
    order of arrival).  Returns the control's results."""
    control = None
    for word in PATTERNS:
        with poisoned_empty(word) as p:
            got = run()
            torch.cuda.synchronize()
        assert p.tensors > 0 and p.bytes > 0, "nothing was poisoned: the case does not allocate with torch.empty"
        got = {name: host(x) for name, x in got.items()}
        if check is not None:
            check(got, word)
        if word == CONTROL:
            control = got
        else:
            for name, x in got.items():
                if name in unordered:
                    continue
                assert same_bits(x, control[name]), f"pattern {pattern_id(word)}: {name} differs from the control pattern's"
    return control


def ws_words(ws, off, n):
    return ws[off:off + 4 * n].view(torch.int32).clone()


def assert_topk(got, want, rows=None, what=""):
    v, i = got["vals"], got["idx"]
    if rows is not None:
        v, i = v[rows], i[rows]
    wv, wi = want
    assert np.array_equal(i, wi), f"{what}: indices differ from the oracle's in {int((i != wi).sum())} places"
    assert same_bits(v, wv), f"{what}: scores differ from the oracle's"


# ---------------------------------------------------------------------------------------------------------------------------
# exact k <= 64
# ---------------------------------------------------------------------------------------------------------------------------

def exact_run(tt, L, Qt, Dt, k, keep=None, off=0, diag=()):
    """One score_topk on a workspace the test allocates (torch.empty: poisoned like the host's own) so that the diagnostics can
    be read; diag: (name, byte offset, words) triples."""
    B, d = Qt.shape
    N = Dt.shape[0]
    bf = int(Dt.dtype == torch.bfloat16)
    if keep is not None or k > 64:
        need = L.tt_score_topk_large_workspace_bytes(B, N, d, k, bf)
    else:
        need = (L.tt_score_topk_bf16_workspace_bytes if bf else L.tt_score_topk_workspace_bytes)(B, N, d, k)
    ws = torch.empty(max(need, 16), dtype=torch.uint8, device="cuda")
    v, i = tt.score_topk(Qt, Dt, k, off, ws, keep)
    out = {"vals": v, "idx": i}
    for name, o, n in diag:
        out[name] = ws_words(ws, o, n)
    return out


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("B,N,d,k", [(5, 3000, 256, 10),      # partial lists and merge
                                     (1, 9, 64, 64),          # N < k: the tail comes back as (-inf, -1) over the poison
                                     (16, 3000, 128, 10),     # one 16-query tile (fp32 rows): the first workspace layout
                                     (17, 3000, 128, 10)])    # two tiles of 16 / one of 32: the second
def test_exact_small_shapes(tt, L, oracle, bf16, B, N, d, k):
    if (B, N, d) in ((16, 3000, 128), (17, 3000, 128)):
        # fp32 rows: B <= 16 is one 16-query tile (16 workspace rows, as B = 1), B = 17 one 32-query tile (32 rows, as B = 32);
        # bf16 rows know 32-query tiles only: ONE layout for both (the sizes say so), run all the same
        ws = L.tt_score_topk_bf16_workspace_bytes if bf16 else L.tt_score_topk_workspace_bytes
        sizes = [ws(b, N, d, k) for b in (1, 16, 17, 32)]
        assert sizes[2] == sizes[3] and sizes[0] == sizes[1] and (sizes[1] == sizes[2]) is bf16, sizes
    Q = synth.unit_rows(11 + B, B, d)
    Dt = torch.from_numpy(synth.unit_rows(12 + N, N, d)).cuda()
    if bf16:
        Dt = Dt.to(torch.bfloat16)
    want = oracle.score_topk(Q, host_f32(Dt), k)
    Qt = torch.from_numpy(Q).cuda()

    def run():
        v, i = tt.score_topk(Qt, Dt, k)         # the host's own workspace and outputs
        return {"vals": v, "idx": i}

    def check(got, word):
        assert_topk(got, want, what=pattern_id(word))
        if N < k:
            assert (got["idx"][:, N:] == -1).all() and np.isneginf(got["vals"][:, N:]).all()

    every_pattern(run, check)


def paced_corpus(oracle):
    """(160, 1 500 000, 64, 10): three or more query tiles -> paced chunks, chunks long enough for a shared pool."""
    def make():
        B, N, d, k = 160, 1_500_000, 64, 10
        Qt, Dt = queries(31 + B, B, d), rows_on_device(32 + B, N, d)
        return Qt, Dt, OracleTopk(oracle, host(Qt), host_f32(Dt), k), k
    return corpus("paced", make)


def pool_corpus(oracle):
    """(200, 700 000, 128, 10) with query 5's best document planted at row 600 000, deep in the pool's part of the corpus."""
    def make():
        B, N, d, k = 200, 700_000, 128, 10
        Qt, Dt = queries(71, B, d), rows_on_device(72, N, d)
        Dt[600_000] = Qt[5]
        return Qt, Dt, OracleTopk(oracle, host(Qt), host_f32(Dt), k), k
    return corpus("pool", make)


@pytest.mark.parametrize("which", ["paced_160x1500000x64", "pool_200x700000x128"])
def test_exact_paced_chunks_and_shared_pool(tt, L, oracle, which):
    Qt, Dt, orc, k = (paced_corpus if which.startswith("paced") else pool_corpus)(oracle)
    B, d = Qt.shape
    N = Dt.shape[0]
    redo_off = L.tt_score_topk_redo_flags_offset(B, N, d, k)
    pace_off = L.tt_score_topk_pace_timeouts_offset(B, N, d, k)
    assert redo_off != SIZE_MAX, "this shape should draw from a shared pool"
    assert pace_off != SIZE_MAX, "this shape should be paced"
    ntile = (B + 31) // 32
    rows = sample_queries(B) + ([5] if which.startswith("pool") else [])
    want = orc.rows(rows)

    def check(got, word):
        assert_topk(got, want, rows, pattern_id(word))
        assert not got["redo"].any(), f"pattern {pattern_id(word)}: redo flags {got['redo']}"   # an ordinary run redoes nothing
        assert int(got["idx"].max()) < N and np.isfinite(got["vals"]).all()
        if which.startswith("pool"):
            assert got["idx"][5, 0] == 600_000

    every_pattern(lambda: exact_run(tt, L, Qt, Dt, k, diag=[("redo", redo_off, ntile)]), check)


def test_exact_16_query_tiles_with_the_sample_pass(tt, L, oracle):
    """(97, 300 000, 512, 10): wide embeddings on 16-query tiles; N >= 262 144 with short chunks: the sample pass seeds the
    main pass from the workspace's threshold row."""
    B, N, d, k = 97, 300_000, 512, 10
    # 16-query tiles: the workspace has 7 x 16 = 112 rows -- B = 112 is the same plan, B = 113 another (32-query tiles: 128 rows
    # from B = 97 on).  Never paced (pacing is the 32-query tiles').
    ws = L.tt_score_topk_workspace_bytes
    assert ws(B, N, d, k) == ws(112, N, d, k) != ws(113, N, d, k) and L.tt_score_topk_pace_timeouts_offset(B, N, d, k) == SIZE_MAX
    # the sample pass has no query of its own; its gate (make_plan) is N >= 262 144 and chunks shorter than 65 536 documents,
    # a chunk being the corpus's 32-document tiles over 8 waves per CU shared by the 7 query tiles
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    chunks = (8 * cus + 6) // 7
    assert N >= 262_144 and -(-((N + 31) // 32) // chunks) * 32 < 65_536
    Qt, Dt = queries(500 + d + B, B, d), rows_on_device(600 + N, N, d)
    Dt[N // 2] = Dt[7]                                   # an exact tie: the lower index must come first
    Qt[0] = Dt[7]
    rows = sample_queries(B, tile=16)
    Dn = host_f32(Dt)
    want = par_rows(lambda q: oracle.score_topk(q, Dn, k, 5), host(Qt)[rows])
    assert list(want[1][0][:2]) == [12, N // 2 + 5]

    def run():
        v, i = tt.score_topk(Qt, Dt, k, 5)
        return {"vals": v, "idx": i}

    every_pattern(run, lambda got, word: assert_topk(got, want, rows, pattern_id(word)))


# ---------------------------------------------------------------------------------------------------------------------------
# large k (tt_score_topk_large_* through score_topk)
# ---------------------------------------------------------------------------------------------------------------------------
OFF = 12_345


def large_case(tt, L, oracle, Q, Dt, k, tier0, what):
    """tier0: the tier query 0 must end in; 0: every query's.  (The other queries' words are held to the control pattern's.)"""
    Qt = torch.from_numpy(Q).cuda()
    B, d = Q.shape
    N = Dt.shape[0]
    bf = int(Dt.dtype == torch.bfloat16)
    tier_off = L.tt_score_topk_large_tier_offset(B, N, d, k, bf)
    assert tier_off != SIZE_MAX
    Dn = host_f32(Dt)
    want = par_rows(lambda q: oracle.score_topk(q, Dn, k, OFF), Q)

    def check(got, word):
        assert_topk(got, want, what=f"{what} {pattern_id(word)}")
        assert got["tier"][0] == tier0 and (tier0 or not got["tier"].any()), f"{what} {pattern_id(word)}: tier words {got['tier']}"

    every_pattern(lambda: exact_run(tt, L, Qt, Dt, k, off=OFF, diag=[("tier", tier_off, B)]), check)


@pytest.mark.parametrize("dt,d,k,B,N", [("f32", 256, 100, 5, 65_537), ("bf16", 64, 1000, 33, 65_537)])
def test_large_k_tier0(tt, L, oracle, dt, d, k, B, N):
    """Two shapes of test_large_k_gpu.GRID (k = 100 and k = 1000): chunks of at most 64 documents never saturate a list."""
    seed = d * 7 + k + B * 3 + N % 1000
    Q = synth.unit_rows(seed, B, d)
    Dt = rows_on_device(seed + 1, N, d, bf16=dt == "bf16")
    large_case(tt, L, oracle, Q, Dt, k, 0, f"tier 0 {dt}")


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_large_k_tier1_near_duplicate_block(tt, L, oracle, bf16):
    """test_tier1_near_duplicate_block's corpus: ~3000 near-duplicates of query 0's best neighbour in one contiguous block, each
    pushed off it by a growing amount orthogonal to the query, so that the best 1000 documents sit in a few chunks whose lists
    are all above t_q.  bf16 rows: the same construction with pushes a bf16 row can resolve (its 8 mantissa bits move a score
    by up to ~1e-3, which would shuffle the fp32 corpus's score steps of ~1e-7 across chunks): eps from 0.05 to 0.5, i.e. scores
    1 - eps^2 / 2 falling by >= 1.5e-3 per 160-document chunk."""
    d, N, k = 256, 300_007, 1000
    Q = synth.unit_rows(21, 3, d)
    D = synth.unit_rows(22, N, d)
    j = int(np.argmax(D @ Q[0]))
    rs = np.random.RandomState(23)
    n_dup, lo = 3000, 120_000
    R = rs.standard_normal((n_dup, d)).astype(np.float32)
    for u in (Q[0], D[j]):  # orthogonal to the query and to the neighbour
        un = u / np.linalg.norm(u)
        R -= np.outer(R @ un, un).astype(np.float32)
    R /= np.linalg.norm(R, axis=1, keepdims=True)
    e0, e1 = (5e-2, 4.5e-1) if bf16 else (1e-3, 2e-2)
    eps = (e0 + e1 * np.arange(n_dup) / n_dup).astype(np.float32)
    blk = D[j][None, :] + eps[:, None] * R
    D[lo:lo + n_dup] = (blk / np.linalg.norm(blk, axis=1, keepdims=True)).astype(np.float32)
    Dt = torch.from_numpy(D).cuda()
    large_case(tt, L, oracle, Q, Dt.to(torch.bfloat16) if bf16 else Dt, k, 1, "tier 1")


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_large_k_tier2_twenty_thousand_exact_duplicates(tt, L, oracle, bf16):
    """test_tier2_twenty_thousand_exact_duplicates, contiguous layout: a tie group five times the per-query buffer; the 1024
    lowest indices win.  (bf16: the rows and query 0 rounded to bf16, so that the copies stay exact copies.)"""
    d, N, k = 128, 300_007, 1024
    Q = synth.unit_rows(31, 2, d)
    D = synth.unit_rows(32, N, d)
    if bf16:
        Q[0] = torch.from_numpy(Q[0]).to(torch.bfloat16).float().numpy()
    D[50_000:70_000] = Q[0]
    Dt = torch.from_numpy(D).cuda()
    large_case(tt, L, oracle, Q, Dt.to(torch.bfloat16) if bf16 else Dt, k, 2, "tier 2")


# ---------------------------------------------------------------------------------------------------------------------------
# masked search, count and range
# ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_masked_search_holes_in_every_tile_and_fewer_than_k_kept(tt, L, oracle, bf16):
    B, N, d, k = 17, 20_001, 128, 10
    Dt, Qt = rows_on_device(800 + bf16, N, d, bf16), queries(801, B, d)
    Dn, Qn = host_f32(Dt), host(Qt)
    holes = np.random.RandomState(5).rand(N) < 0.7
    holes[3::32] = False                                 # a hole in every 32-document tile
    few = np.zeros(N, dtype=bool)
    few[[5, 4000, 4001, 9999, 12_345, 20_000, 19_999]] = True   # 7 kept documents < k
    rows = np.arange(B)
    tier_off = L.tt_score_topk_large_tier_offset(B, N, d, k, int(bf16))
    assert tier_off != SIZE_MAX
    ix = tt.BruteForceIndex(Dt, idx_offset=9)
    for name, mask in (("holes", holes), ("few", few)):
        keep = tt.pack_keep_mask(torch.from_numpy(mask).cuda())
        want = expected(oracle, Qn, Dn, mask, k, rows, 9)

        def run():
            out = exact_run(tt, L, Qt, Dt, k, keep=keep, off=9, diag=[("tier", tier_off, B)])
            v, i = ix.search(Qt, k, keep=keep)  # the index's route to the same call, on the host's own buffers
            out.update(ix_vals=v, ix_idx=i)
            return out

        def check(got, word):
            assert_topk(got, want, what=f"{name} {pattern_id(word)}")
            assert same_bits(got["ix_vals"], got["vals"]) and same_bits(got["ix_idx"], got["idx"])
            assert not got["tier"].any(), f"{name} {pattern_id(word)}: tier words {got['tier']}"   # k <= 64: the exact call's own
            if name == "few":
                assert (got["idx"][:, 7:] == -1).all() and np.isneginf(got["vals"][:, 7:]).all() and (got["idx"][:, :7] >= 9).all()

        every_pattern(run, check)


def threshold_kinds(S, k):
    """One threshold per query, rotating: -inf, +inf, a score of the query's own row (a tie at the threshold), the next float
    above it, its k-th best score, NaN."""
    B, N = S.shape
    b = np.arange(B)
    at = S[b, (7 * b + 3) % N]
    kinds = np.stack([np.full(B, -np.inf, np.float32), np.full(B, np.inf, np.float32), at, np.nextafter(at, np.float32(np.inf)),
                      -np.sort(-S, axis=1)[:, min(k, N) - 1], np.full(B, np.nan, np.float32)])
    return np.ascontiguousarray(kinds[b % 6, b])


def counts_of(S, t, mask=None):
    with np.errstate(invalid="ignore"):
        hit = S >= t[:, None]
    return (hit if mask is None else hit & mask[None, :]).sum(1).astype(np.int64)


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_count_with_one_threshold_per_query_on_the_paced_counting_pass(tt, L, oracle, bf16):
    """B = 130 on 32-query tiles: five query tiles, so the counting pass is paced and zeroes its own slots."""
    B, N, d = 130, 65_537, 64
    assert L.tt_score_topk_pace_timeouts_offset(B, N, d, 1) != SIZE_MAX         # (the query knows fp32 plans only)
    # ... and the bf16 plan cuts the same chunks: a counting workspace of the same size holds the same counts + pacing slots
    assert L.tt_score_count_workspace_bytes(B, N, d, 1) == L.tt_score_count_workspace_bytes(B, N, d, 0)
    Dt, Qt = rows_on_device(810 + bf16, N, d, bf16), queries(811, B, d)
    Dn = host_f32(Dt)
    S = par_rows(lambda q: oracle.score_all(q, Dn), host(Qt))
    t = threshold_kinds(S, 10)
    mask = np.random.RandomState(6).rand(N) < 0.5
    keep = tt.pack_keep_mask(torch.from_numpy(mask).cuda())
    td = torch.from_numpy(t).cuda()
    ix = tt.BruteForceIndex(Dt)
    want, want_m = counts_of(S, t), counts_of(S, t, mask)
    assert 0 in want and N in want and ((want > 0) & (want < N)).any()

    def check(got, word):
        assert np.array_equal(got["counts"], want) and np.array_equal(got["masked"], want_m), pattern_id(word)

    every_pattern(lambda: {"counts": ix.count(Qt, td), "masked": ix.count(Qt, td, keep=keep)}, check)


def test_range_search_and_the_streamed_count_across_blocks(tt, oracle):
    """range_search on the resident index, and StreamedIndex.count: three blocks (the last one ragged) accumulate into one
    tensor, masked and unmasked; the streamed index is built under the pattern too (its staging buffers are torch.empty)."""
    N, d, k, B = 10_000, 128, 10, 20
    Db, Qt = rows_on_device(91, N, d, bf16=True), queries(92, B, d)
    Dn, Qn = host_f32(Db), host(Qt)
    S = oracle.score_all(Qn, Dn)
    t = threshold_kinds(S, k)
    td = torch.from_numpy(t).cuda()
    mask = np.random.RandomState(7).rand(N) < 0.5
    keep = tt.pack_keep_mask(torch.from_numpy(mask).cuda())
    want_c, want_cm = counts_of(S, t), counts_of(S, t, mask)
    ov, oi = oracle.score_topk(Qn, Dn, k, 50)
    with np.errstate(invalid="ignore"):
        live = (ov >= t[:, None]) & (oi >= 0)
    want_v, want_i = np.where(live, ov, NEG_INF), np.where(live, oi, -1)
    host_rows = Db.cpu()

    def run():
        ref = tt.BruteForceIndex(Db, idx_offset=50)
        st = tt.StreamedIndex(host_rows, block_docs=4096, idx_offset=50)
        c, v, i = ref.range_search(Qt, td, k)
        sc, sv, si = st.range_search(Qt, td, k)
        return {"counts": c, "vals": v, "idx": i, "st_counts": sc, "st_vals": sv, "st_idx": si,
                "st_masked": st.count(Qt, td, keep=keep), "masked": ref.count(Qt, td, keep=keep)}

    def check(got, word):
        w = pattern_id(word)
        assert np.array_equal(got["counts"], want_c) and np.array_equal(got["st_counts"], want_c), w
        assert np.array_equal(got["masked"], want_cm) and np.array_equal(got["st_masked"], want_cm), w
        for pre in ("", "st_"):
            assert np.array_equal(got[pre + "idx"], want_i) and same_bits(got[pre + "vals"], want_v), w

    every_pattern(run, check)


# ---------------------------------------------------------------------------------------------------------------------------
# candidate search and exclusion lists: no workspace, only their outputs are poisoned
# ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_score_ids_and_candidate_search(tt, oracle, bf16):
    from test_score_ids_gpu import N as N_IDS, dev_rows, expected_scores, expected_topk, id_lists, reference
    d, B, Cn, off, k = 256, 33, 257, 1000, 10
    D, Q, S = reference(oracle, d, bf16)
    docs, Qd = dev_rows(D, bf16), torch.from_numpy(Q).cuda()
    ids = id_lists(np.random.RandomState(d + bf16), B, Cn, off)
    idd = torch.from_numpy(ids).cuda()
    want_v, want_i = expected_scores(S[:B], ids, off)
    want_top = expected_topk(want_v, want_i, k)
    assert (want_i == -1).any() and (want_i >= 0).any() and (want_i[1] == -1).all() and N_IDS == D.shape[0]
    ix = tt.BruteForceIndex(docs, idx_offset=off)

    def run():
        v, i = ix.search(Qd, k, candidates=idd)
        return {"scores": ix.score_ids(Qd, idd), "free": tt.score_ids(Qd, docs, idd, idx_offset=off), "vals": v, "idx": i}

    def check(got, word):
        assert same_bits(got["scores"], want_v) and same_bits(got["free"], want_v), pattern_id(word)
        assert_topk(got, want_top, what=pattern_id(word))

    every_pattern(run, check)


def test_search_with_exclusion_lists(tt, oracle):
    """search(exclude=): every query excludes its own top entries but one; k + E = 15 runs the k <= 64 search, k + E = 110 the
    large one, each followed by the filter launch."""
    B, N, d = 33, 5000, 64
    Q, D = synth.unit_rows(401, B, d), synth.unit_rows(402, N, d)
    Qt = torch.from_numpy(Q).cuda()
    ix = tt.BruteForceIndex(torch.from_numpy(D).cuda(), idx_offset=7)
    for k, E in ((10, 5), (10, 100)):
        ov, oi = oracle.score_topk(Q, D, k + E + 1, 7)
        excl = oi[:, 1:E + 1].copy()
        excl[:, ::3] = -1                                # padding entries; the others are the query's ranks 2 .. E + 1
        listed = np.zeros_like(oi, dtype=bool)
        listed[:, 1:E + 1] = excl >= 0
        want_v = np.stack([ov[b][~listed[b]][:k] for b in range(B)])
        want_i = np.stack([oi[b][~listed[b]][:k] for b in range(B)])
        ed = torch.from_numpy(excl).cuda()

        def run():
            v, i = ix.search(Qt, k, exclude=ed)
            return {"vals": v, "idx": i}

        every_pattern(run, lambda got, word: assert_topk(got, (want_v, want_i), what=f"E={E} {pattern_id(word)}"))


# ---------------------------------------------------------------------------------------------------------------------------
# screened search
# ---------------------------------------------------------------------------------------------------------------------------
VARIANTS = [("f32", False), ("bf16", False), ("f32", True), ("bf16", True)]
VARIANT_IDS = ["f32", "bf16", "f32_masked", "bf16_masked"]


def screened_results(ix, Qt, k, keep=None, **kw):
    """One search of a keep_stats index: results, fallback flags and the per-query (pooled, survivors) statistics."""
    v, i = ix.search(Qt, k, keep=keep, **kw)
    return {"vals": v, "idx": i, "flags": ix.fallback_flags.clone(), "stats": ix.search_stats()}


def stats_are_written(got, B, N, k, what):
    """The statistics are not compared (with the pool and the refresh they depend on timing), but they must be COUNTS: at least
    the k documents of the answer were pooled and rescored, at most the corpus."""
    st = got.pop("stats")
    assert st.shape == (B, 2), what
    assert (st >= min(k, N)).all() and (st <= N).all(), f"{what}: statistics {st.min()} .. {st.max()}"


def screened_corpus(oracle, dt, N, B, seed):
    def make():
        Dt, Qt = rows_on_device(seed, N, 256, dt == "bf16"), queries(seed + 1, B, 256)
        return Dt, Qt, host_f32(Dt), host(Qt)
    return corpus(("screened", dt, N, B, seed), make)


@pytest.mark.parametrize("B", [7, 128, 600])
@pytest.mark.parametrize("dt,masked", VARIANTS, ids=VARIANT_IDS)
def test_screened_streaming_and_shared_tile_forms(tt, oracle, monkeypatch, dt, masked, B):
    """N = 33 333, below the sample pass: B = 7 is the streaming form, B = 128 and 600 the shared-tile form (one and two query
    groups); every workgroup of the main pass starts without thresholds, so every candidate count and pool counter matters."""
    from twotowermlretrieval_amd import index as _index
    monkeypatch.setattr(_index, "SCREEN_MIN_DOCS", 0)
    N, k = 33_333, 10
    Dt, Qall, Dn, Qn = screened_corpus(oracle, dt, N, 600, 900)
    Qt = Qall[:B].contiguous()
    mask = np.ones(N, dtype=bool)
    keep = None
    if masked:
        mask = np.random.RandomState(8).rand(N) < 0.7
        mask[3::32] = False
        keep = tt.pack_keep_mask(torch.from_numpy(mask).cuda())
    rows = np.array(sample_queries(B))
    want = expected(oracle, Qn[:B], Dn, mask, k, rows, 7)
    exact = tuple(host(x) for x in tt.score_topk(Qt, Dt, k, 7, keep=keep))

    def run():
        ix = tt.BruteForceIndex(Dt, idx_offset=7, screen=True, screen_masked=masked)   # (the fp16 shadow is torch.empty too)
        ix.keep_stats = True
        assert ix._screens(B, k, masked) and ix._screen_bf16 is (dt == "bf16")
        return screened_results(ix, Qt, k, keep)

    def check(got, word):
        w = f"{dt} masked={masked} B={B} {pattern_id(word)}"
        stats_are_written(got, B, N, k, w)
        assert_topk(got, want, rows, w)
        assert same_bits(got["vals"], exact[0]) and np.array_equal(got["idx"], exact[1]), w
        assert got["flags"].shape == ((B + 31) // 32,) and not got["flags"].any(), f"{w}: fallback flags {got['flags']}"

    every_pattern(run, check)


REFRESH_N = 300_007
REFRESH_ON = dict(TT_SCREEN_REFRESH_MIN_TILES=8, TT_SCREEN_TAIL_DIV=2)


@pytest.mark.parametrize("B", [65, 300])
@pytest.mark.parametrize("dt,masked", VARIANTS, ids=VARIANT_IDS)
def test_screened_mid_pass_refresh_and_pool(tt, oracle, dt, masked, B):
    """The shared threshold ladders and the pool counters, reached the way test_screen_thr_refresh_gpu.py reaches them: the
    comparison build with the refresh gate lowered to 8 tiles and the last half of every chunk handed out in pool blocks, over
    300 007 rows (sample pass: the seed comes from the on-chip sample maxima, which live in the candidate buffers)."""
    from test_screen_thr_refresh_gpu import n_qgroups, plan
    k = 10
    pl = plan(REFRESH_N, n_qgroups(B), k)
    assert pl["tail_blocks"] > 0 and pl["own"] >= 8, pl      # pool blocks, and own ranges long enough for a checkpoint
    Dt, Qall, Dn, Qn = screened_corpus(oracle, dt, REFRESH_N, 300, 4100)
    Qt = Qall[:B].contiguous()
    mask = np.ones(REFRESH_N, dtype=bool)
    keep = None
    if masked:
        mask = np.random.RandomState(5).rand(REFRESH_N) < 0.7
        mask[3::32] = False
        keep = tt.pack_keep_mask(torch.from_numpy(mask).cuda())
    rows = np.array([0, B // 2, B - 1])
    want = expected(oracle, Qn[:B], Dn, mask, k, rows)
    exact = tuple(host(x) for x in tt.score_topk(Qt, Dt, k, keep=keep))

    def make_index():
        with poisoned_empty(0xFFFFFFFF):                 # built once: 150 MB of shadow per build
            ix = tt.BruteForceIndex(Dt, screen=True, screen_masked=masked)
        ix.keep_stats = True
        return ix
    ix = corpus(("refresh_index", dt, masked), make_index)
    assert ix._screens(B, k, masked)

    def run():
        with ab_library(**REFRESH_ON):
            got = screened_results(ix, Qt, k, keep)
            torch.cuda.synchronize()
        return got

    def check(got, word):
        w = f"{dt} masked={masked} B={B} {pattern_id(word)}"
        stats_are_written(got, B, REFRESH_N, k, w)
        assert_topk(got, want, rows, w)
        assert same_bits(got["vals"], exact[0]) and np.array_equal(got["idx"], exact[1]), w
        assert not got["flags"].any(), f"{w}: fallback flags {got['flags']}"

    every_pattern(run, check)


@pytest.mark.parametrize("dt,masked", VARIANTS, ids=VARIANT_IDS)
def test_screened_survivor_overflow_and_the_device_fallback(tt, oracle, monkeypatch, dt, masked):
    """test_tie_cluster_overflow_triggers_exact_fallback_on_device's corpus: 1400 exact copies of one document overflow the
    finish kernel's survivor list, the flag is raised on the device and the predicated exact kernel -- in the workspace BEHIND
    the screen's -- rewrites the flagged tiles.  The flags must be the same tiles under every pattern.  (Masked: a hole in every
    tile leaves ~1356 of the copies; the fallback is then the masked exact kernel.)"""
    from twotowermlretrieval_amd import index as _index
    monkeypatch.setattr(_index, "SCREEN_MIN_DOCS", 0)
    N, k = 5000, 10
    Q = synth.unit_rows(21, 128, 256)
    D = synth.unit_rows(22, N, 256).copy()
    D[1000:2400] = Q[5]
    Qt, Dt = torch.from_numpy(Q).cuda(), torch.from_numpy(D).cuda()
    if dt == "bf16":
        Dt = Dt.to(torch.bfloat16)
    mask, keep = np.ones(N, dtype=bool), None
    if masked:
        mask[3::32] = False
        keep = tt.pack_keep_mask(torch.from_numpy(mask).cuda())
    want = expected(oracle, Q, host_f32(Dt), mask, k, np.arange(128))
    assert list(want[1][5]) == list(range(1000, 1010))             # the copies, index-ascending

    def run():
        ix = tt.BruteForceIndex(Dt, screen=True, screen_masked=masked)
        assert ix._screens(128, k, masked)
        v, i = ix.search(Qt, k, keep=keep)
        return {"vals": v, "idx": i, "flags": ix.fallback_flags.ne(0)}

    def check(got, word):
        assert_topk(got, want, what=f"{dt} masked={masked} {pattern_id(word)}")
        assert got["flags"][0], (pattern_id(word), got["flags"])

    every_pattern(run, check)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_screened_seed_list_then_seeded_through_a_world_1_sharded_index(tt, oracle, dt):
    """ShardedIndex at world 1 with shard_k > k: seed_list into a torch.empty list, the union seed, then the seeded call on the
    same workspace -- whose query image, pool counters and ladders are the seed call's (the one place a call relies on what an
    earlier call left in the workspace)."""
    N, B, k, off = 65_536, 33, 10, 9
    Dt, Qt, Dn, Qn = screened_corpus(oracle, dt, N, B, 500)
    want = oracle.score_topk(Qn, Dn, k, off)

    def run():
        top = tt.ShardedIndex(Dt, off, shard_k=50, screen=True)
        assert top._seed_exchange and top._index._screens(B, 50)
        v, i = top.search(Qt, k)
        return {"vals": v, "idx": i, "flags": top._index.fallback_flags.clone()}

    def check(got, word):
        assert_topk(got, want, what=f"{dt} {pattern_id(word)}")
        assert got["flags"].shape == (2,) and not got["flags"].any(), (pattern_id(word), got["flags"])

    every_pattern(run, check)


@pytest.mark.parametrize("dt,masked", VARIANTS, ids=VARIANT_IDS)
def test_screened_graphed_search_warm_up_and_two_replays(tt, oracle, dt, masked):
    """GraphedSearch: the warm-up searches allocate under the pattern (nothing is filled while the stream captures), then two
    replays with different queries.  Masked: documents removed before the capture (a hole in every tile), so that the captured
    launches are the masked screened search's."""
    N, B, k = 70_000, 4, 10
    Dt, _, Dn, _ = screened_corpus(oracle, dt, N, B, 91)
    Qs = [synth.unit_rows(seed, B, 256) for seed in (92, 93)]
    mask = np.ones(N, dtype=bool)
    if masked:
        mask[3::32] = False
    gone = torch.from_numpy(np.flatnonzero(~mask)).cuda()
    wants = [expected(oracle, Q, Dn, mask, k, np.arange(B)) for Q in Qs]

    def run():
        ix = tt.BruteForceIndex(Dt, screen=True, screen_masked=masked)
        if masked:
            ix.remove_ids(gone)
        assert ix._screens(B, k) and ix._screen_bf16 is (dt == "bf16")
        gs = tt.GraphedSearch(ix, batch=B, k=k)
        out = {}
        for n, Q in enumerate(Qs):
            v, i = gs(torch.from_numpy(Q).cuda())
            torch.cuda.synchronize()
            out[f"vals{n}"], out[f"idx{n}"] = v.clone(), i.clone()
        out["flags"] = ix.fallback_flags.clone()                           # the captured search's buffer, as the last replay left it
        return out

    def check(got, word):
        assert not got["flags"].any(), (pattern_id(word), got["flags"])    # the screen answered, not the exact fallback
        for n, want in enumerate(wants):
            assert_topk({"vals": got[f"vals{n}"], "idx": got[f"idx{n}"]}, want, what=f"replay {n} {pattern_id(word)}")

    every_pattern(run, check)


# ---------------------------------------------------------------------------------------------------------------------------
# encoder and training
# ---------------------------------------------------------------------------------------------------------------------------
ENCODER_CASES = ["a2", "r1_17", "r3",   # gru16x4 exchange area, one and two directions
                 "r4",                  # gru16, three-kernel prep (the status block is cleared by the call's zero launch)
                 "r5",                  # three-kernel prep below B = 1024
                 "a3",                  # fp32 recurrence
                 "b3",                  # two layers, bidirectional LSTM
                 "b2",                  # wgrad16 scale words
                 "r8_256",              # split-K projection gradient
                 "g1",                  # trainable table: g_table (torch.empty_like: poisoned) is zeroed, then added into
                 "f2"]                  # arith="f32"


@pytest.mark.parametrize("cid", ENCODER_CASES)
def test_encoder_forward_and_backward(cid):
    """RNNEncoder's eval forward (deriving its weights in the workspace: no prepared cache), training forward and backward on
    poisoned workspaces, outputs and status words, against the float64 reference of the case (test_encoder_f64_gpu.reference,
    computed once per session)."""
    from test_encoder_f64_gpu import BY_ID, build, reference
    ids_np, table, sd, d_out, want, wg, wt = reference(cid)
    trainable = bool(BY_ID[cid][8].get("trainable"))
    d_out_t = torch.from_numpy(d_out.copy()).cuda()

    def run():
        enc, ids = build(cid, False)
        enc.cache_prepared = False
        with torch.no_grad():
            out = {"eval": enc(ids)}
        enc, ids = build(cid, True)
        y = enc(ids)
        y.backward(d_out_t)
        out["train"] = y.detach()
        for name, prm in enc.named_parameters():
            if prm.requires_grad:
                out["grad:" + name] = prm.grad
        return out

    def check(got, word):
        assert_fwd_close(got["eval"], want, atol=FWD_ATOL, what="_eval_" + pattern_id(word))
        assert_fwd_close(got["train"], want, atol=FWD_ATOL, what="_train_" + pattern_id(word))
        checked = set()
        for name, g in got.items():
            if not name.startswith("grad:"):
                continue
            name = name[5:]
            if name == "embedding.weight":
                assert trainable
                assert_grad_close(g, wt, tol=GRAD_TOL, what=name, floor=1e-6)
                assert not g[0].any()                                      # padding_idx: exactly zero, not the pattern
                continue
            key = name[len("rnn."):] if name.startswith("rnn.") else name
            assert_grad_close(g, wg[key], tol=GRAD_TOL, what=name, floor=1e-6)
            checked.add(key)
        assert checked == set(wg) and ("grad:embedding.weight" in got) == trainable

    every_pattern(run, check, unordered=("grad:embedding.weight",))   # (table_scatter_kernel adds with float atomics)


def test_encoder_prepared_and_projected_inference_forms(oracle):
    """tt_encoder_prepare_f32 + the prepared forward, and the projected-table forward of test_projected_gpu.py (config.json's
    shape: both directions of layer 0 gather, layer 1 projects as before): the prepared blob and the projected table are
    torch.empty buffers that live across calls, so both are built under the pattern."""
    from test_encoder_gpu import make_encoder
    B, T, E, H, layers, bi = 33, 17, 200, 256, 2, True
    V, seed = 700, 4000 + B + H
    ids_np = synth.make_ids(seed + 3, B, T, V, zero_inside=0.05)
    ids_np[0, 0] = V - 1
    ids = torch.from_numpy(ids_np).cuda()
    _, table, sd = make_encoder(V, E, H, seed, layers, bi)
    want = oracle.encoder_forward(ids_np, table, synth.weight_quads(sd, layers, bi), H, layers, bi, sd.get("projection.weight"),
                                  sd.get("projection.bias"), True)

    def run():
        enc = make_encoder(V, E, H, seed, layers, bi)[0]
        out = {}
        with torch.no_grad():
            enc.cache_prepared = False
            out["plain"] = enc(ids).clone()
            enc.cache_prepared = True
            enc.projected_table = False
            out["prepared"] = enc(ids).clone()
            assert ids.device in enc._prep, "the prepared weights were not built"
            enc.projected_table = True
            out["projected"] = enc(ids).clone()
            assert ids.device in enc._proj, "the projected table was not built"
        return out

    def check(got, word):
        assert same_bits(got["prepared"], got["plain"]) and same_bits(got["projected"], got["plain"]), pattern_id(word)
        assert_fwd_close(got["projected"], want, what="_projected_" + pattern_id(word))

    every_pattern(run, check)


def test_triplet_loss_and_fused_clip_adam():
    """triplet_loss_cosine at (B, H) = (5, 512): the loss word (a 0-dim torch.empty) and the per-row scratch; FusedClipAdam, three
    steps at n = 131 073 (the first size with two elements per thread): its scratch of partial sums.  Bounds: test_train_f64_gpu.py's."""
    from f64_ref import clip_adam_f64, triplet_f64
    from twotowermlretrieval_amd.model import triplet_loss_cosine
    from twotowermlretrieval_amd.trainer import FusedClipAdam
    B, H, margin, n = 5, 512, 0.2, 131_073
    q, p, neg = (synth.unit_rows(7 * B + s, B, H) for s in range(3))
    want_t = triplet_f64(q, p, neg, margin)
    rs = np.random.RandomState(n % 1000 + 3)
    p0 = rs.standard_normal(n).astype(np.float32)
    grads = []
    for target in (10.0, 0.01, 10.0):
        z = rs.standard_normal(n)
        grads.append((z / np.linalg.norm(z) * target).astype(np.float32))
    want_a = clip_adam_f64(p0, grads, lr=1e-3, max_norm=1.0)
    gd = [torch.from_numpy(g).cuda() for g in grads]

    def run():
        t = [torch.from_numpy(a).cuda().requires_grad_(True) for a in (q, p, neg)]
        loss = triplet_loss_cosine(tuple(t), margin=margin)
        loss.backward()
        out = {"loss": loss.detach(), "dq": t[0].grad, "dp": t[1].grad, "dn": t[2].grad}
        prm = torch.nn.Parameter(torch.from_numpy(p0).cuda())
        opt = FusedClipAdam([prm], lr=1e-3, max_norm=1.0)
        for step, g in enumerate(gd):
            opt.zero_grad()
            prm.grad.copy_(g)
            out[f"norm{step}"] = opt.step().clone()
            out[f"params{step}"] = prm.detach().clone()
        return out

    def check(got, word):
        assert got["loss"].shape == () and abs(float(got["loss"]) - want_t[0]) < 1e-6, pattern_id(word)
        for name, w in zip(("dq", "dp", "dn"), want_t[1:]):
            np.testing.assert_allclose(got[name], w, atol=2e-7, rtol=1e-4, err_msg=pattern_id(word))
        for step, (wp, wn) in enumerate(want_a):
            assert abs(float(got[f"norm{step}"][0]) - wn) / wn < 1e-6, (pattern_id(word), step)
            np.testing.assert_allclose(got[f"params{step}"], wp, atol=1e-8, rtol=2e-6, err_msg=pattern_id(word))

    every_pattern(run, check)


def test_gated_step_after_a_bad_batch(tt):
    """test_a_bad_batch_raises_and_leaves_the_weights_untouched under the patterns: the towers' status words (torch.empty(1)) are
    folded into the gate; a poisoned word that the prep kernels did not overwrite would veto, or let through, the wrong steps."""
    V, E, H, B = 300, 300, 256, 32
    table = synth.make_table(4, V, E)
    ids = [torch.from_numpy(synth.make_ids(70 + s, B, T, V)).cuda() for s, T in enumerate((7, 20, 25))]
    bad_id = [t.clone() for t in ids]
    bad_id[1][3, 0] = V + 5                            # a positive passage with an id out of range
    empty = [t.clone() for t in ids]
    empty[0][5, :] = 0                                 # a query of padding only
    torch.manual_seed(3)
    proto = tt.TwoTowerModel({"VOCAB_SIZE": V, "EMBED_DIM": E, "HIDDEN_DIM": H}, table)

    def run():
        m = copy.deepcopy(proto).cuda().train()
        opt = tt.FusedClipAdam(m.parameters(), lr=1e-3, max_norm=1.0)
        l0 = tt.train_step(m, opt, *ids, margin=0.5)
        torch.cuda.synchronize()
        before = (opt.flat_params.clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone(), opt.step_count)
        with pytest.raises(IndexError):
            tt.train_step(m, opt, *bad_id, margin=0.5)
        with pytest.raises(RuntimeError):
            tt.train_step(m, opt, *empty, margin=0.5)
        torch.cuda.synchronize()
        assert torch.equal(opt.flat_params, before[0]) and torch.equal(opt.exp_avg, before[1]) and torch.equal(opt.exp_avg_sq, before[2])
        assert opt.step_count == before[3] == 1
        l1 = tt.train_step(m, opt, *ids, margin=0.5)
        assert opt.step_count == 2
        return {"loss0": l0.clone(), "loss1": l1.clone(), "after_one": before[0], "params": opt.flat_params.clone(),
                "exp_avg_sq": opt.exp_avg_sq.clone()}

    def check(got, word):
        assert np.isfinite(got["params"]).all() and not same_bits(got["params"], got["after_one"]), pattern_id(word)

    got = every_pattern(run, check)
    # the control's two steps are the two steps of an optimizer that never saw the bad batches
    m = copy.deepcopy(proto).cuda().train()
    opt = tt.FusedClipAdam(m.parameters(), lr=1e-3, max_norm=1.0)
    for _ in range(2):
        tt.train_step(m, opt, *ids, margin=0.5)
    assert same_bits(host(opt.flat_params), got["params"]) and same_bits(host(opt.exp_avg_sq), got["exp_avg_sq"])


def test_graphed_train_step_replayed_twice(tt):
    """GraphedTrainStep: warm-up and capture under the pattern, then two replays with batches of different widths, each equal --
    bit for bit -- to the eager train_step (run without a pattern) on the ids padded to the captured widths."""
    V, E, H, B = 300, 300, 256, 64
    table = synth.make_table(4, V, E)
    torch.manual_seed(9)
    proto = tt.TwoTowerModel({"VOCAB_SIZE": V, "EMBED_DIM": E, "HIDDEN_DIM": H}, table)
    batches = [[torch.from_numpy(synth.make_ids(200 + 3 * i + s, B, T, V)).cuda() for s, T in enumerate(widths)]
               for i, widths in enumerate(((7, 20, 25), (16, 48, 31)))]

    def padded(t, w):
        out = torch.zeros((t.shape[0], w), dtype=torch.int64, device=t.device)
        out[:, : t.shape[1]] = t
        return out

    ref = copy.deepcopy(proto).cuda().train()
    ref_opt = tt.FusedClipAdam(ref.parameters(), lr=1e-3, max_norm=1.0)
    want = []
    for ids in batches:
        loss = tt.train_step(ref, ref_opt, padded(ids[0], 16), padded(ids[1], 48), padded(ids[2], 48), margin=0.5)
        torch.cuda.synchronize()
        want.append((host(loss).copy(), host(ref_opt.flat_params).copy(), host(ref_opt.exp_avg_sq).copy()))

    def run():
        m = copy.deepcopy(proto).cuda().train()
        opt = tt.FusedClipAdam(m.parameters(), lr=1e-3, max_norm=1.0)
        start = opt.flat_params.clone()
        step = tt.GraphedTrainStep(m, opt, batch=B, q_width=16, doc_width=48, margin=0.5)
        torch.cuda.synchronize()
        assert torch.equal(opt.flat_params, start) and opt.step_count == 0     # warm-up and capture: all-padding ids, gate closed
        out = {}
        for n, ids in enumerate(batches):
            out[f"loss{n}"] = step(*ids).clone()
            torch.cuda.synchronize()
            out[f"params{n}"], out[f"exp_avg_sq{n}"] = opt.flat_params.clone(), opt.exp_avg_sq.clone()
            assert opt.step_count == n + 1
        return out

    def check(got, word):
        for n, (wl, wp, wv) in enumerate(want):
            assert same_bits(got[f"loss{n}"], wl) and same_bits(got[f"params{n}"], wp) and same_bits(got[f"exp_avg_sq{n}"], wv), \
                (pattern_id(word), n)

    every_pattern(run, check)


# ---------------------------------------------------------------------------------------------------------------------------
# the previous call's end state: one never-cleared workspace through calls of different shapes
# ---------------------------------------------------------------------------------------------------------------------------

def test_exact_search_on_one_workspace_through_a_sequence_of_shapes(tt, L, oracle):
    """score_topk(..., workspace=ws) on ONE ws sized for the largest call: pool + pacing, a small merge, the paced corpus, the
    tier-2 corpus at k = 1000, the smoke shape, a masked call -- each plan lays its regions over what the previous call left
    (counters at their end values, redo flags, tier words, lists of another k).  Every answer is the oracle's."""
    Qp, Dp, orc_p, k = pool_corpus(oracle)
    Qc, Dc, orc_c, _ = paced_corpus(oracle)
    small = [(synth.unit_rows(11 + B, B, d), synth.unit_rows(12 + N, N, d)) for B, N, d in ((33, 1000, 256), (5, 3000, 256))]
    Q2 = synth.unit_rows(31, 2, 128)
    D2 = synth.unit_rows(32, 300_007, 128)
    D2[50_000:70_000] = Q2[0]
    mask = np.random.RandomState(5).rand(3000) < 0.7
    mask[3::32] = False
    keep = tt.pack_keep_mask(torch.from_numpy(mask).cuda())
    dev = lambda a: torch.from_numpy(a).cuda()
    calls = [  # (name, Q, D, k, keep, oracle rows, expected values / indices)
        ("pool", Qp, Dp, k, None, sample_queries(200) + [5], None),
        ("small", dev(small[0][0]), dev(small[0][1]), 10, None, None, oracle.score_topk(*small[0], 10)),
        ("paced", Qc, Dc, k, None, sample_queries(160), None),
        ("tier2", dev(Q2), dev(D2), 1000, None, None, par_rows(lambda q: oracle.score_topk(q, D2, 1000), Q2)),
        ("smoke", dev(small[1][0]), dev(small[1][1]), 10, None, None, oracle.score_topk(*small[1], 10)),
        ("masked", dev(small[1][0]), dev(small[1][1]), 10, keep, None,
         expected(oracle, small[1][0], small[1][1], mask, 10, np.arange(5))),
    ]
    need = 0
    for name, Qt, Dt, kk, kp, rows, want in calls:
        B, d = Qt.shape
        fn = L.tt_score_topk_large_workspace_bytes if (kp is not None or kk > 64) else None
        need = max(need, fn(B, Dt.shape[0], d, kk, 0) if fn else L.tt_score_topk_workspace_bytes(B, Dt.shape[0], d, kk))
    with poisoned_empty(0xFFFFFFFF):
        ws = torch.empty(need, dtype=torch.uint8, device="cuda")     # never cleared from here on
    for rnd in range(2):                                             # the second round starts from the masked call's end state
        for name, Qt, Dt, kk, kp, rows, want in calls:
            v, i = tt.score_topk(Qt, Dt, kk, 0, ws, kp)
            torch.cuda.synchronize()
            got = {"vals": host(v), "idx": host(i)}
            if want is None:
                want = (orc_p if name == "pool" else orc_c).rows(rows)
            assert_topk(got, want, rows, f"round {rnd} {name}")
            B, d = Qt.shape
            off = L.tt_score_topk_redo_flags_offset(B, Dt.shape[0], d, min(kk, 64))
            if off != SIZE_MAX and kp is None:
                assert not ws_words(ws, off, (B + 31) // 32).any(), f"round {rnd} {name}: redo flags"
            if name == "tier2":
                tier = ws_words(ws, L.tt_score_topk_large_tier_offset(B, Dt.shape[0], d, kk, 0), B)
                assert int(tier[0]) == 2, tier


def test_screened_search_on_one_workspace_through_the_c_abi(tt, L, oracle):
    """In the manner of the seed_corpus tests of test_search_aux_gpu.py: shadow built with tt_index_build_f16, then
    tt_score_topk_screened_f32 for B = 600, 65 and 7 over the same corpus on ONE workspace and ONE flags buffer, neither ever
    cleared: two query groups of the shared-tile form, one, then the streaming form, each laid over the previous call's
    candidates, counts, pool counters, ladders and flags."""
    from twotowermlretrieval_amd import _lib
    N, k = 70_000, 10
    Dt, Qall, Dn, Qn = screened_corpus(oracle, "f32", N, 600, 7000)
    st = torch.cuda.current_stream().cuda_stream
    d16 = torch.zeros((N, 256), dtype=torch.float16, device="cuda")
    stats = torch.zeros(2, dtype=torch.float32, device="cuda")
    _lib.check(L.tt_index_build_f16(Dt.data_ptr(), N, 256, d16.data_ptr(), stats.data_ptr(), st))
    dmax = float(stats[0])
    sizes = (600, 65, 7, 600)
    need = max(L.tt_score_topk_screened_workspace_bytes(B, N, 256, k) for B in sizes)
    with poisoned_empty(0x3F800000):
        ws = torch.empty(need, dtype=torch.uint8, device="cuda")
        flags = torch.empty((max(sizes) + 31) // 32, dtype=torch.int32, device="cuda")
    orc = OracleTopk(oracle, Qn, Dn, k)
    for B in sizes:
        q = Qall[:B].contiguous()
        v = torch.full((B, k), float("nan"), dtype=torch.float32, device="cuda")
        i = torch.full((B, k), -7, dtype=torch.int64, device="cuda")
        _lib.check(L.tt_score_topk_screened_f32(q.data_ptr(), B, 256, Dt.data_ptr(), d16.data_ptr(), N, k, dmax, 0, v.data_ptr(),
                                                i.data_ptr(), flags.data_ptr(), ws.data_ptr(), ws.numel(), None, st))
        torch.cuda.synchronize()
        rows = sample_queries(B)
        assert_topk({"vals": host(v), "idx": host(i)}, orc.rows(rows), rows, f"B={B}")
        ev, ei = tt.score_topk(q, Dt, k)
        assert torch.equal(i, ei) and torch.equal(v, ev), B
        assert not flags[:(B + 31) // 32].any(), (B, flags)            # this call's tiles; the words behind them are the last call's


# ---------------------------------------------------------------------------------------------------------------------------
# lexical search and the in-batch loss
# ---------------------------------------------------------------------------------------------------------------------------

def lexical_corpora(L):
    """The `main` corpus of test_lexical_gpu.py (3 C + 17 rows: the direct merge) and a corpus of 65 C + 3 short rows (more than 64
    chunks: the two-step merge), with two queries each and their reference scores; N = 5 and N = 0 are prefixes of main."""
    def make():
        import lexical_ref as ref
        C_ = L.tt_lexical_chunk_docs()
        m = ref.MainCorpus(C_)
        rng = np.random.default_rng(41)
        N = 65 * C_ + 3
        lens = rng.integers(0, 9, size=N)
        allc = np.cumsum(rng.integers(1, 31, size=(N, 8)), axis=1) - 1
        ip = np.zeros(N + 1, dtype=np.int64)
        np.cumsum(lens, out=ip[1:])
        cols = allc[np.arange(8)[None, :] < lens[:, None]].astype(np.int32)
        vals = (rng.integers(1, 9, size=cols.size) / 8.0).astype(np.float32)         # few distinct values: large tie groups
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        big_q = [(rng.permutation(241)[:40], (rng.integers(1, 5, size=40) / 4.0).astype(np.float32)) for _ in range(3)]
        out = {"C": C_, "F": ref.MAIN_F, "ref": ref,
               "main": ((dev(m.indptr), dev(m.cols), dev(m.vals)), [m.queries[n] for n in ("random", "every", "tie")],
                        [m.S[n] for n in ("random", "every", "tie")]),
               "big": ((dev(ip), dev(cols), dev(vals)), big_q,
                       [ref.ref_scores32(ip, cols, vals, ref.dense_query(*q, ref.MAIN_F)) for q in big_q])}
        return out
    return corpus("lexical", make)


def lexical_abi(L, t, N, F, q, k, ws):
    """tt_lexical_score_topk_f32 over the first N rows of the corpus t on the caller's workspace -> (vals, idx) as numpy."""
    from twotowermlretrieval_amd import _lib
    qi, qc, qv = q
    B = qi.numel() - 1
    ov = torch.full((B, k), float("nan"), dtype=torch.float32, device="cuda")
    oi = torch.full((B, k), -7, dtype=torch.int64, device="cuda")
    _lib.check(L.tt_lexical_score_topk_f32(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), N, F, qi.data_ptr(), qc.data_ptr(),
                                           qv.data_ptr(), B, None, None, None, 0, 0.0, 1.0, k, 0, ov.data_ptr(), oi.data_ptr(),
                                           ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return host(ov), host(oi)


def test_lexical_search_on_one_workspace_through_the_c_abi(L):
    """ONE workspace sized for the largest call, filled once with -1 words and never cleared, through (B, N, k) = (3, 65 C + 3,
    1024), (1, 5, 100), (2, 3 C + 17, 10), (3, 65 C + 3, 64), (1, 0, 7): two-step and direct merge in turn, each plan's lists
    laid over the previous call's lists of another k.  Every answer is ref_topk's, and bit for bit the answer of the same call
    on a fresh zeroed workspace."""
    lx = lexical_corpora(L)
    ref, C_, F = lx["ref"], lx["C"], lx["F"]
    calls = [("big", 3, 65 * C_ + 3, 1024), ("main", 1, 5, 100), ("main", 2, 3 * C_ + 17, 10), ("big", 3, 65 * C_ + 3, 64),
             ("main", 1, 0, 7)]
    need = max(L.tt_lexical_workspace_bytes(B, N, k) for _, B, N, k in calls)
    assert L.tt_lexical_workspace_bytes(3, 65 * C_ + 3, 1024) > 3 * 1024 * 12 * 65 + 3 * 1024 * 12      # (it holds the first merge's lists)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    ws.view(torch.int32).fill_(-1)                                     # never cleared from here on
    for which, B, N, k in calls:
        t, queries_, S = lx[which]
        q = tuple(torch.from_numpy(a).cuda() for a in ref.queries_csr(queries_[:B]))
        v, i = lexical_abi(L, t, N, F, q, k, ws)
        fresh = torch.zeros(max(L.tt_lexical_workspace_bytes(B, N, k), 16), dtype=torch.uint8, device="cuda")
        fv, fi = lexical_abi(L, t, N, F, q, k, fresh)
        assert same_bits(v, fv) and np.array_equal(i, fi), (which, B, N, k)
        for b in range(B):
            wv, wi = ref.ref_topk(S[b][:N], k)
            assert np.array_equal(i[b], wi) and same_bits(v[b], wv), (which, B, N, k, b)


def test_lexical_forms_under_every_pattern(tt, L):
    """lexical_score_topk (its workspace and outputs are torch.empty) at k = 10 and 100 on the direct merge, k = 10 and 1024 on
    the two-step merge, under a keep-bitmask; lexical_score_all's output; a LexicalIndex search after remove_ids."""
    lx = lexical_corpora(L)
    ref, C_, F = lx["ref"], lx["C"], lx["F"]
    t, queries_, S = lx["main"]
    tb, big_q, big_S = lx["big"]
    N, Nb = 3 * C_ + 17, 65 * C_ + 3
    q = tuple(torch.from_numpy(a).cuda() for a in ref.queries_csr(queries_))
    qb = tuple(torch.from_numpy(a).cuda() for a in ref.queries_csr(big_q[:2]))
    keep_host = np.arange(N) % 3 != 0
    keep = tt.pack_keep_mask(torch.from_numpy(keep_host).cuda())
    gone = [int(ref.ref_topk(big_S[0], 1)[1][0]), 0, Nb - 1]
    kept_b = np.ones(Nb, dtype=bool)
    kept_b[gone] = False
    ix = tt.LexicalIndex((*tb, F), idx_offset=9)
    ix.remove_ids([g + 9 for g in gone])

    def run():
        out = {"all": tt.lexical_score_all(t, F, q)}
        for k in (10, 100):
            out[f"v{k}"], out[f"i{k}"] = tt.lexical_score_topk(t, F, q, k, keep=keep)
        for k in (10, 1024):
            out[f"bv{k}"], out[f"bi{k}"] = tt.lexical_score_topk(tb, F, qb, k)
        out["xv"], out["xi"] = ix.search(qb, 100)
        return out

    def check(got, word):
        w = pattern_id(word)
        for b in range(3):
            assert same_bits(got["all"][b], S[b]), w
            for k in (10, 100):
                wv, wi = ref.ref_topk(S[b], k, keep=keep_host)
                assert np.array_equal(got[f"i{k}"][b], wi) and same_bits(got[f"v{k}"][b], wv), (w, k, b)
        for b in range(2):
            for k in (10, 1024):
                wv, wi = ref.ref_topk(big_S[b], k)
                assert np.array_equal(got[f"bi{k}"][b], wi) and same_bits(got[f"bv{k}"][b], wv), (w, k, b)
            wv, wi = ref.ref_topk(big_S[b], 100, keep=kept_b, idx_offset=9)
            assert np.array_equal(got["xi"][b], wi) and same_bits(got["xv"][b], wv), (w, b)

    every_pattern(run, check)


def test_in_batch_loss_on_one_workspace_through_the_c_abi(L):
    """ONE workspace sized for B = 1025, H = 512, filled once with 0xFF bytes and never cleared, through (B, H) = (1025, 256),
    (65, 96), (449, 32), (3, 32), (513, 20), (1025, 256): images, partial maxima and sums and the per-slice gradient partials of
    each plan (3 to 8 slices, other paddings) lie over the previous call's.  Every result is finite and bit for bit that of the
    same call on a zeroed workspace; the first and the last call agree bit for bit."""
    from twotowermlretrieval_amd import _lib
    shapes = [(1025, 256), (65, 96), (449, 32), (3, 32), (513, 20), (1025, 256)]
    need = L.tt_in_batch_loss_workspace_bytes(1025, 512)
    assert need >= max(L.tt_in_batch_loss_workspace_bytes(B, H) for B, H in shapes)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    ws.fill_(0xFF)                                                     # never cleared from here on
    st = torch.cuda.current_stream().cuda_stream

    def call(t, B, H, work):
        loss = torch.full((1,), float("nan"), device="cuda")
        g = [torch.full_like(x, float("nan")) for x in t]
        _lib.check(L.tt_in_batch_loss_f32(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), B, H, 0.05, loss.data_ptr(),
                                          g[0].data_ptr(), g[1].data_ptr(), g[2].data_ptr(), work.data_ptr(), work.numel(), st))
        torch.cuda.synchronize()
        return [host(loss)] + [host(x) for x in g]

    results = []
    for B, H in shapes:
        t = [torch.from_numpy(synth.unit_rows(300 + B + s, B, H)).cuda() for s in range(3)]
        got = call(t, B, H, ws)
        want = call(t, B, H, torch.zeros(L.tt_in_batch_loss_workspace_bytes(B, H), dtype=torch.uint8, device="cuda"))
        for name, x, y in zip(("loss", "dq", "dp", "dn"), got, want):
            assert np.isfinite(x).all(), (B, H, name)
            assert same_bits(x, y), (B, H, name)
        results.append(got)
    assert all(same_bits(x, y) for x, y in zip(results[0], results[-1]))
