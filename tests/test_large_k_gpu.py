"""Exact search for 64 < k <= 1024 (tt_score_topk_large_f32 / _bf16, tt_topk_merge_large and the package paths that route to
them): bit for bit the CPU oracle's top-k -- values, indices, the (score desc, index asc) tie order and the N < k tail --
across the shape grid, the seeded (sample prepass) and paced multi-tile main passes, and the three tiers of the large-k
path, each forced by the data it exists for."""
import ctypes as C

import numpy as np
import pytest
import torch

import synth
from test_search_aux_gpu import par_rows

pytestmark = pytest.mark.gpu

OFF = 12_345


@pytest.fixture(scope="module")
def tt():
    import twotowermlretrieval_amd as m
    from twotowermlretrieval_amd import _lib
    _lib.lib()
    assert torch.cuda.is_available()
    return m


def _oracle_topk(oracle, Q, D, k, off=0):
    return par_rows(lambda q: oracle.score_topk(q, D, k, off), Q)


def _same(got, want, what=""):
    gv, gi = (t.cpu().numpy() for t in got)
    wv, wi = want
    assert gv.shape == wv.shape, what
    assert np.array_equal(gi, wi), f"{what}: indices differ in {int((gi != wi).sum())} places"
    assert np.array_equal(gv.view(np.uint32), wv.view(np.uint32)), f"{what}: scores differ"


def _large(tt, Q, D, k, off=0, keep_ws=None):
    """One tt_score_topk_large_* call; returns (vals, idx, tier per query).  keep_ws: a list that receives the workspace."""
    from twotowermlretrieval_amd import _lib
    L = _lib.lib()
    B, d = Q.shape
    N = D.shape[0]
    bf = int(D.dtype == torch.bfloat16)
    ws = torch.empty(max(L.tt_score_topk_large_workspace_bytes(B, N, d, k, bf), 16), dtype=torch.uint8, device=Q.device)
    v = torch.empty((B, k), dtype=torch.float32, device=Q.device)
    i = torch.empty((B, k), dtype=torch.int64, device=Q.device)
    fn = L.tt_score_topk_large_bf16 if bf else L.tt_score_topk_large_f32
    _lib.check(fn(Q.data_ptr(), B, d, D.data_ptr(), N, k, off, v.data_ptr(), i.data_ptr(), ws.data_ptr(), ws.numel(),
                  torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    o = L.tt_score_topk_large_tier_offset(B, N, d, k, bf)
    tier = ws[o:o + 4 * B].view(torch.int32).cpu().numpy().copy()
    if keep_ws is not None:
        keep_ws.append(ws)
    return v, i, tier


def _bf16_rows(seed, n, d):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randn((n, d), device="cuda", generator=g).div_(d ** 0.5).to(torch.bfloat16)


# (dtype, d, k, B, N): every k, B, N and d of the grid appears, each oracle call <= ~3e9 FMAs
GRID = [
    ("f32", 32, 65, 1, 1), ("f32", 32, 1024, 33, 999), ("f32", 32, 256, 100, 65_537), ("f32", 32, 1000, 5, 300_007),
    ("f32", 128, 100, 17, 1), ("f32", 128, 65, 16, 999), ("f32", 128, 1024, 32, 65_537), ("f32", 128, 256, 1, 300_007),
    ("f32", 256, 1000, 100, 999), ("f32", 256, 100, 5, 65_537), ("f32", 256, 65, 33, 65_537), ("f32", 256, 1024, 16, 300_007),
    ("f32", 320, 256, 5, 999), ("f32", 320, 1000, 17, 65_537), ("f32", 320, 100, 1, 300_007),
    ("f32", 512, 1024, 1, 999), ("f32", 512, 65, 32, 65_537), ("f32", 512, 1000, 16, 300_007),
    ("bf16", 64, 65, 1, 999), ("bf16", 64, 1000, 33, 65_537), ("bf16", 64, 1024, 5, 300_007), ("bf16", 64, 256, 100, 1),
    ("bf16", 256, 100, 17, 999), ("bf16", 256, 1024, 100, 65_537), ("bf16", 256, 256, 16, 300_007), ("bf16", 256, 65, 1, 65_537),
]


@pytest.mark.parametrize("dt,d,k,B,N", GRID)
def test_large_k_grid_equals_oracle(tt, oracle, dt, d, k, B, N):
    seed = d * 7 + k + B * 3 + N % 1000
    Q = synth.unit_rows(seed, B, d)
    if dt == "bf16":
        Dt = _bf16_rows(seed + 1, N, d)
        D = Dt.float().cpu().numpy()
    else:
        D = synth.unit_rows(seed + 1, N, d)
        Dt = torch.from_numpy(D).cuda()
    got = tt.score_topk(torch.from_numpy(Q).cuda(), Dt, k, idx_offset=OFF)
    torch.cuda.synchronize()
    _same(got, _oracle_topk(oracle, Q, D, k, OFF), f"{dt} d={d} k={k} B={B} N={N}")


def test_large_k_with_the_sample_prepass(tt, oracle):
    """N = 2M: the main pass is seeded from the sample -- with the k-th, not the 64th, sample maximum."""
    Q = synth.unit_rows(5, 3, 128)
    D = synth.unit_rows(6, 2_000_003, 128)
    got = _large(tt, torch.from_numpy(Q).cuda(), torch.from_numpy(D).cuda(), 1000, OFF)
    _same(got[:2], _oracle_topk(oracle, Q, D, 1000, OFF), "N=2M k=1000")


def test_large_k_paced_multi_tile(tt, oracle):
    """B = 1024: 32 query tiles on the paced main pass with the shared pool."""
    Q = synth.unit_rows(7, 1024, 128)
    D = synth.unit_rows(8, 100_003, 128)
    got = _large(tt, torch.from_numpy(Q).cuda(), torch.from_numpy(D).cuda(), 1000, OFF)
    _same(got[:2], _oracle_topk(oracle, Q, D, 1000, OFF), "B=1024 k=1000")


@pytest.mark.parametrize("bf16", [False, True])
def test_large_k_pool_give_up_is_redone_before_t_q(tt, oracle, bf16):
    """The give-up trap: a wave that gives up its bounded wait for a pool draw marks its lists (+inf, TT_TOPK_INVALID_INDEX + t).
    The large path must find those lists and redo their query tiles on the static split BEFORE it takes t_q from the union: a
    marker taken as t_q would flag nothing and put the markers themselves into the answer.  The comparison build forces the
    give-up for every wave that did not draw itself (TT_DRAW_POLLS=-1): the redo flags (the k = 64 main pass's, at the same
    offset in the large workspace) are raised, and the result is still the ordinary run's and the oracle's, bit for bit."""
    from conftest import ab_library
    from twotowermlretrieval_amd import _lib
    B, N, d, k = 200, 700_000, 128, 1000
    L = _lib.lib()
    off = L.tt_score_topk_redo_flags_offset(B, N, d, 64)
    assert off != C.c_size_t(-1).value, "this shape should draw from a shared pool"
    ntile = (B + 31) // 32
    Q = synth.unit_rows(91, B, d)
    if bf16:
        Dt = _bf16_rows(92, N, d)
        D = Dt.float().cpu().numpy()
    else:
        D = synth.unit_rows(92, N, d)
        Dt = torch.from_numpy(D).cuda()
    Q[5] = D[600_000]                                  # a document deep in the pool's part of the corpus is query 5's best
    Qt = torch.from_numpy(Q).cuda()
    ws0, ws1 = [], []
    v0, i0, _ = _large(tt, Qt, Dt, k, 0, ws0)
    assert int(ws0[0][off:off + 4 * ntile].view(torch.int32).ne(0).sum()) == 0     # an ordinary run redoes nothing
    with ab_library(TT_DRAW_POLLS=-1):
        v1, i1, _ = _large(tt, Qt, Dt, k, 0, ws1)
        redone = int(ws1[0][off:off + 4 * ntile].view(torch.int32).ne(0).sum())
    assert redone > 0, "the forced give-up did not happen"
    assert int(i1.max()) < N and int(i1.min()) >= 0 and bool(torch.isfinite(v1).all())
    assert int(i1[5, 0]) == 600_000
    assert torch.equal(i1, i0) and torch.equal(v1.view(torch.int32), v0.view(torch.int32))
    qs = [0, 5, 199]
    _same((v1[qs], i1[qs]), _oracle_topk(oracle, Q[qs], D, k), "forced give-up")


def test_large_entry_point_at_k64_is_the_exact_call_and_prefixes_agree(tt):
    from twotowermlretrieval_amd import _lib
    L = _lib.lib()
    for B, d in ((5, 256), (40, 128), (7, 512)):
        Q = torch.from_numpy(synth.unit_rows(11 + B, B, d)).cuda()
        D = torch.from_numpy(synth.unit_rows(12 + B, 70_001, d)).cuda()
        v64, i64, tier = _large(tt, Q, D, 64, OFF)
        assert not tier.any()
        ws = torch.empty(L.tt_score_topk_workspace_bytes(B, 70_001, d, 64), dtype=torch.uint8, device="cuda")
        v = torch.empty((B, 64), dtype=torch.float32, device="cuda")
        i = torch.empty((B, 64), dtype=torch.int64, device="cuda")
        _lib.check(L.tt_score_topk_f32(Q.data_ptr(), B, d, D.data_ptr(), 70_001, 64, OFF, v.data_ptr(), i.data_ptr(),
                                       ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        assert torch.equal(i, i64) and torch.equal(v.view(torch.int32), v64.view(torch.int32))
        v1000, i1000, _ = _large(tt, Q, D, 1000, OFF)
        v100, i100, _ = _large(tt, Q, D, 100, OFF)
        assert torch.equal(i1000[:, :100], i100) and torch.equal(v1000[:, :100], v100)
        assert torch.equal(i1000[:, :64], i64)


def test_tier1_near_duplicate_block(tt, oracle):
    """~3000 near-duplicates of query 0's best neighbour in one contiguous block, each pushed off it by a growing amount
    orthogonal to the query: the best 1000 documents sit in a few chunks, whose lists (64 entries) are all above t_q."""
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
    eps = (1e-3 + 2e-2 * np.arange(n_dup) / n_dup).astype(np.float32)
    blk = D[j][None, :] + eps[:, None] * R
    D[lo:lo + n_dup] = (blk / np.linalg.norm(blk, axis=1, keepdims=True)).astype(np.float32)
    v, i, tier = _large(tt, torch.from_numpy(Q).cuda(), torch.from_numpy(D).cuda(), k, OFF)
    assert tier[0] == 1, tier
    _same((v, i), _oracle_topk(oracle, Q, D, k, OFF), "tier 1")


@pytest.mark.parametrize("layout", ["contiguous", "scattered"])
def test_tier2_twenty_thousand_exact_duplicates(tt, oracle, layout):
    """20 000 exact copies of query 0 (a tie group five times the per-query buffer of 4096): the 1024 lowest indices win."""
    d, N, k = 128, 300_007, 1024
    Q = synth.unit_rows(31, 2, d)
    D = synth.unit_rows(32, N, d)
    # scattered: every other row of a 40 000-row stretch, at random (a chunk's list then holds nothing but copies)
    rows = (np.arange(50_000, 70_000) if layout == "contiguous"
            else np.sort(100_000 + np.random.RandomState(33).choice(40_000, 20_000, replace=False)))
    D[rows] = Q[0]
    v, i, tier = _large(tt, torch.from_numpy(Q).cuda(), torch.from_numpy(D).cuda(), k, OFF)
    assert tier[0] == 2, tier
    assert np.array_equal(i[0].cpu().numpy(), rows[:k] + OFF)
    _same((v, i), _oracle_topk(oracle, Q, D, k, OFF), f"tier 2 {layout}")


def test_tier2_bf16_ties(tt, oracle):
    d, N, k = 64, 100_003, 700
    Qb = _bf16_rows(41, 2, d)
    Db = _bf16_rows(42, N, d)
    Db[10_000:16_000] = Qb[0]
    Q = Qb.float()
    v, i, tier = _large(tt, Q.contiguous(), Db, k, 0)
    assert tier[0] == 2, tier
    _same((v, i), _oracle_topk(oracle, Q.cpu().numpy(), Db.float().cpu().numpy(), k), "tier 2 bf16")


def test_clustered_corpus_k1000(tt, oracle):
    import bench
    dev = torch.device("cuda")
    D, Q, _ = bench.make_clustered_corpus(200_000, 48, dev)
    v, i, tier = _large(tt, Q.contiguous(), D.contiguous(), 1000, 0)
    _same((v, i), _oracle_topk(oracle, Q.cpu().numpy(), D.cpu().numpy(), 1000), "clustered corpus")
    print("clustered corpus tiers:", np.bincount(tier, minlength=3).tolist())


@pytest.mark.parametrize("M", [65, 1024, 8192, 131_072])
def test_large_merge_equals_oracle(tt, oracle, M):
    rs = np.random.RandomState(M)
    B = 4
    vals = rs.choice(np.linspace(-1, 1, 97).astype(np.float32), size=(B, M))  # many equal values
    idx = np.stack([rs.permutation(M * 3)[:M] for _ in range(B)]).astype(np.int64)
    idx[rs.random_sample((B, M)) < 0.1] = -1                                    # padding
    vals[0, :5] = -np.inf                                                       # valid -inf entries
    for k in (65, 100, 1000, 1024):
        got = tt.topk_merge(torch.from_numpy(vals).cuda(), torch.from_numpy(idx).cuda(), k)
        torch.cuda.synchronize()
        _same(got, oracle.topk_merge(vals, idx, k), f"M={M} k={k}")


def test_large_merge_shards_in_place(tt, oracle):
    from twotowermlretrieval_amd import _lib
    rs = np.random.RandomState(5)
    world, B, kp, k = 3, 5, 300, 500
    vals = rs.choice(np.linspace(0, 1, 50).astype(np.float32), size=(world, B, kp))
    idx = rs.permutation(world * B * kp * 2)[:world * B * kp].reshape(world, B, kp).astype(np.int64)
    idx[:, :, -20:] = -1
    nv = B * kp * 4
    stride = nv + B * kp * 8
    buf = np.zeros((world, stride), dtype=np.uint8)
    buf[:, :nv] = vals.reshape(world, -1).view(np.uint8)
    buf[:, nv:] = idx.reshape(world, -1).view(np.uint8)
    g = torch.from_numpy(buf).cuda()
    ov = torch.empty((B, k), dtype=torch.float32, device="cuda")
    oi = torch.empty((B, k), dtype=torch.int64, device="cuda")
    _lib.check(_lib.lib().tt_topk_merge_shards_large(g.data_ptr(), world, stride, nv, B, kp, k, ov.data_ptr(), oi.data_ptr(),
                                                     torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    cat_v = np.concatenate(list(vals), axis=1)
    cat_i = np.concatenate(list(idx), axis=1)
    _same((ov, oi), oracle.topk_merge(cat_v, cat_i, k), "shards")


def test_package_paths_at_large_k(tt, oracle):
    from twotowermlretrieval_amd import index as _index
    d = 256
    D = synth.unit_rows(51, 66_000, d)
    Q = synth.unit_rows(52, 70, d)
    Dt, Qt = torch.from_numpy(D).cuda(), torch.from_numpy(Q).cuda()
    # screened index: k = 100 takes the exact path
    ix = tt.BruteForceIndex(Dt, screen=True)
    _same(ix.search(Qt, 100), _oracle_topk(oracle, Q, D, 100), "BruteForceIndex(screen=True) k=100")
    # streamed (a host bf16 corpus), small blocks, k = 300
    Db = torch.from_numpy(D).to(torch.bfloat16)
    sx = tt.StreamedIndex(Db, block_docs=20_000, idx_offset=OFF)
    _same(sx.search(Qt[:9], 300), _oracle_topk(oracle, Q[:9], Db.float().numpy(), 300, OFF), "StreamedIndex k=300")
    # captured search, k = 500
    ref = ix.search(Qt[:12], 500)
    gs = _index.GraphedSearch(ix, 12, k=500)
    for _ in range(2):
        v, i = gs(Qt[:12])
        torch.cuda.synchronize()
        assert torch.equal(v, ref[0]) and torch.equal(i, ref[1])
    _same(ref, _oracle_topk(oracle, Q[:12], D, 500), "GraphedSearch k=500")


def test_evaluators_at_large_top_k(tt, oracle):
    from test_evaluators_gpu import _TextStub, _TextTok
    from twotowermlretrieval_amd.evaluators import CorpusEvaluator, corpus_recall_hit
    import random
    # corpus_recall_hit against a full numpy sort of the oracle's scores
    q = synth.unit_rows(61, 1, 64)
    D = synth.unit_rows(62, 5000, 64)
    S = oracle.score_all(q, D)[0]
    order = np.lexsort((np.arange(len(S)), -S.astype(np.float64)))
    pos = [int(x) for x in np.random.RandomState(63).choice(5000, 40, replace=False)]
    top_k = [1, 10, 100, 1000]
    got = corpus_recall_hit(torch.from_numpy(q[0]).cuda(), torch.from_numpy(D).cuda(), pos, top_k)
    for k in top_k:
        found = len(set(order[:k].tolist()) & set(pos))
        assert got[f"Recall@{k}"] == found / len(pos) and got[f"Hit@{k}"] == (1 if found else 0), k
    # CorpusEvaluator over 1200 candidates with top_k up to 1000, against metrics recomputed from a full numpy sort of
    # oracle.score_all: several random positives per query, so the tail of every top-1000 list counts
    rs = np.random.RandomState(66)
    n_q, n_d = 8, 1200
    qe = synth.unit_rows(64, n_q, 32)
    de = synth.unit_rows(65, n_d, 32)
    positives = {i: [int(x) for x in rs.choice(n_d, 6, replace=False)] for i in range(n_q)}
    val = [(f"q{i}", f"d{p}", f"d{j}") for i in range(n_q) for p in positives[i] for j in range(i, n_d, n_q)]
    random.seed(3)
    m = CorpusEvaluator(top_k=top_k, max_candidates=5000, max_queries=50).evaluate(_TextStub(qe.tolist(), de.tolist()), val,
                                                                                 _TextTok(), torch.device("cuda"))
    # the evaluator's own order: candidates = the set of documents as built from val, queries = random.sample after seed 3
    query_to_positives, all_docs = {}, set()
    for qn, pn, nn in val:
        query_to_positives.setdefault(qn, set()).add(pn)
        all_docs.add(pn)
        all_docs.add(nn)
    unique_docs = list(all_docs)
    random.seed(3)
    sample = random.sample(list(query_to_positives), min(50, len(query_to_positives)))
    doc_pos = {doc: i for i, doc in enumerate(unique_docs)}
    D_c = de[[int(x[1:]) for x in unique_docs]]
    Q_s = qe[[int(x[1:]) for x in sample]]
    S = oracle.score_all(Q_s, D_c)
    want = {f"{n}@{k}": [] for n in ("Recall", "Hit") for k in top_k}
    for qi, qn in enumerate(sample):
        order = np.lexsort((np.arange(S.shape[1]), -S[qi].astype(np.float64)))
        pos_idx = {doc_pos[doc] for doc in query_to_positives[qn]}
        for k in top_k:
            found = len([i for i in order[:k].tolist() if i in pos_idx])
            want[f"Recall@{k}"].append(found / len(pos_idx))
            want[f"Hit@{k}"].append(1 if found else 0)
    want = {name: float(np.mean(v)) for name, v in want.items()}
    assert m == want, (m, want)
    assert m["Recall@100"] <= m["Recall@1000"] < 1.0
