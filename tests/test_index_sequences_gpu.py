"""The stateful layer above the kernels, driven through SEQUENCES of calls and compared with tests/index_model.py.

An answer of this layer depends on the history of calls: which slot a pipelined step was given and who wrote it since,
what had been removed when a step was enqueued, whether a graph was captured before the first removal.  Every test here
makes a sequence of calls on a real index and on the model, and compares every answer with equality of values and indices
(the scores are the contract's fp32 chain: oracle.score_all, computed once per corpus for a pool of 130 queries, of which
every call takes rows).  The corpora are the smallest at which each route exists; the thresholds are the product's."""
import numpy as np
import pytest
import torch

import index_model as im
import synth
from test_search_aux_gpu import par_rows

pytestmark = pytest.mark.gpu

OFF = 1000       # idx_offset of every index here
SHARD_K = 50


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


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def same(got, want, what=""):
    torch.cuda.synchronize()
    gv, gi = got[0].cpu().numpy(), got[1].cpu().numpy()
    bad_i, bad_v = int((gi != want[1]).sum()), int((gv != want[0]).sum())
    print(f"{what}: index mismatches {bad_i}, value mismatches {bad_v} of {gi.size}")
    assert gi.shape == want[1].shape and gi.dtype == np.int64 and gv.dtype == np.float32, what
    assert bad_i == 0 and bad_v == 0, what


# ---- corpora, made once --------------------------------------------------------------------------------------------------------

# corpus name -> the pool's score matrix, kept for the process: the modules that import `corpora` make the same corpora again.
# The name alone is the key: `corpora` makes every named corpus from fixed seeds, so one name is one matrix.
_POOL_SCORES = {}


class Corpus:
    """Rows (as the index takes them), their fp32 widening on the host, the query pool and its score matrix."""

    def __init__(self, oracle, rows, pool, screen=False, screen_masked=False, streamed=False, name=None):
        self.rows, self.screen, self.screen_masked, self.streamed = rows, screen, screen_masked, streamed
        self.wide = rows.float().cpu().numpy()
        self.N, self.d = self.wide.shape
        self.pool, self.Qd = pool, dev(pool)
        if name is None or name not in _POOL_SCORES:
            S = im.IndexModel(self.wide, OFF, lambda Q, D: par_rows(lambda q: oracle.score_all(q, D), Q)).scores(pool)
            if name is not None:
                _POOL_SCORES[name] = S
        self.S = S if name is None else _POOL_SCORES[name]
        self.shapes = [(1, 10), (33, 10), (33, 50), (33, 100)]
        if screen:
            self.shapes.insert(3, (130, 10))

    def model(self):
        return im.IndexModel(self.wide, OFF)

    def sharded(self, tt):
        if self.streamed:
            return tt.ShardedIndex(self.rows, OFF, shard_k=SHARD_K, block_docs=1024)
        return tt.ShardedIndex(self.rows, OFF, shard_k=SHARD_K, screen=self.screen, screen_masked=self.screen_masked)

    def single(self, tt):
        if self.streamed:
            return tt.StreamedIndex(self.rows, block_docs=1024, idx_offset=OFF, screen=False)
        return tt.BruteForceIndex(self.rows, idx_offset=OFF, screen=self.screen, screen_masked=self.screen_masked)

    def pack(self, tt, mask):
        return tt.pack_keep_mask(dev(mask))


def pool_with_ties(seed, rows_f32, twins):
    """130 unit queries; the first 20 ARE one of a pair of identical rows each, so their two best documents tie."""
    Q = synth.unit_rows(seed, im.POOL, rows_f32.shape[1])
    Q[:20] = rows_f32[twins[:20]]
    return np.ascontiguousarray(Q)


def rows_with_twins(seed, N, d):
    """Unit rows of which 40 are copies of 40 others (pairs that tie for every query)."""
    D = synth.unit_rows(seed, N, d)
    pick = np.random.RandomState(seed).choice(N, 80, replace=False)
    D[pick[40:]] = D[pick[:40]]
    return D, pick


NAMES = ("small_f32", "small_bf16", "screened", "screened_masked", "streamed")


@pytest.fixture(scope="module")
def corpora(tt, oracle):
    made = {}

    def get(name):
        base = "screened" if name == "screened_masked" else name
        if base not in made:
            if base in ("small_f32", "small_bf16"):
                D, pick = rows_with_twins(51, 3000, 64)
                rows = torch.from_numpy(D).cuda()
                rows = rows.to(torch.bfloat16) if base == "small_bf16" else rows
                made[base] = Corpus(oracle, rows, pool_with_ties(52, rows.float().cpu().numpy(), pick), name=base)
            elif base == "screened":
                D, pick = rows_with_twins(53, 65536, 256)
                made[base] = Corpus(oracle, torch.from_numpy(D).cuda(), pool_with_ties(54, D, pick), screen=True, name=base)
            else:
                D, pick = rows_with_twins(55, 3 * 1024 - 5, 64)
                rows = torch.from_numpy(D).to(torch.bfloat16)               # stays on the host: three blocks, the last ragged
                made[base] = Corpus(oracle, rows, pool_with_ties(56, rows.float().numpy(), pick), streamed=True, name=base)
        c = made[base]
        if name == "screened_masked":                                       # the same rows and scores, the other index
            if name not in made:
                m = Corpus.__new__(Corpus)
                m.__dict__.update(c.__dict__)
                m.screen_masked = True
                made[name] = m
            c = made[name]
        return c

    yield get
    made.clear()
    torch.cuda.empty_cache()


def top_lists(model, S, E, rs, keep=None):
    """exclude [B,E]: each query's own best E - 2 live documents (so a search for k alone would come back short), then two
    random ids."""
    top = model.search(S, E - 2, keep)[1]
    return np.concatenate([top, rs.randint(0, model.N, size=(S.shape[0], 2)) + OFF], axis=1).astype(np.int64)


# ---- a. the pipeline ------------------------------------------------------------------------------------------------------------

class Pipe:
    """One ShardedIndex (world 1) and its PipelineModel, given the same calls."""

    def __init__(self, tt, c):
        self.tt, self.c = tt, c
        self.ix = c.sharded(tt)
        self.model = c.model()
        self.pm = im.PipelineModel(self.model, SHARD_K)
        self.pending, self.n_results, self.shapes_used = [], 0, set()

    def take(self, start, B):
        rows = im.pool_rows(start, B)
        return self.c.Qd[dev(rows)].contiguous(), self.c.S[rows]

    def submit(self, B, k, start, extra="plain", E=0, draw=0):
        q, S = self.take(start, B)
        rs = np.random.RandomState(draw)
        on_model, on_gpu = {}, {}
        if extra == "keep":
            mask = rs.rand(self.c.N) < 0.5
            on_model["keep"], on_gpu["keep"] = mask, self.c.pack(self.tt, mask)
        elif extra == "exclude":
            on_model["exclude"] = top_lists(self.model, S, E, rs)
            on_gpu["exclude"] = dev(on_model["exclude"])
        elif extra == "candidates":
            on_model["candidates"] = im.random_candidates(rs, B, 200, self.c.N, OFF)
            on_gpu["candidates"] = dev(on_model["candidates"])
        h = self.pm.submit(S, k, **on_model)
        self.pending.append(self.ix.submit(q, k, **on_gpu))
        self.shapes_used.add(im.step_shape(B, k, E, SHARD_K))
        assert h == len(self.pending) - 1
        return h

    def result(self, h):
        got = self.pending[h].result()
        same(got, self.pm.result(h), f"result of step {h}")
        self.n_results += 1
        return got

    def expired(self, h):
        assert not self.pm.valid(h)
        with pytest.raises(RuntimeError, match="two more submits of the same shape"):
            self.pending[h].result()

    def search(self, B, k, start):
        q, S = self.take(start, B)
        same(self.ix.search(q, k), self.pm.search(S, k), f"search({B}, {k})")

    def remove(self, start, n):
        """The n best live documents of pool query `start`, an id beyond the corpus, one below the offset and padding."""
        ids = self.model.search(self.c.S[start:start + 1], n)[1].ravel()
        ids = np.concatenate([ids[ids >= 0], [OFF + self.c.N + 3, OFF - 1, -1]]).astype(np.int64)
        self.ix.remove_ids(dev(ids))
        self.model.remove(ids)
        return ids[:-3]


def a_b(c):
    """(A, B) pairs of different (B, k) for the scripted sequences of corpus c."""
    pairs = [((33, 10), (33, 50)), ((1, 10), (33, 100))]
    return pairs + [((130, 10), (33, 10))] if c.screen else pairs


@pytest.mark.parametrize("name", NAMES)
def test_a_b_a_and_the_first_a_collected_last(tt, corpora, name):
    """submit(A), submit(B), submit(A') with different queries at every step; the first A's result() is taken last, after
    ONE further submit of its shape: it must still be its own rows."""
    c = corpora(name)
    for A, B in a_b(c):
        p = Pipe(tt, c)
        h0 = p.submit(*A, start=0)
        h1 = p.submit(*B, start=40)
        h2 = p.submit(*A, start=80)
        assert not np.array_equal(p.pm.result(h0)[1], p.pm.result(h2)[1])
        p.result(h2)
        p.result(h1)
        p.result(h0)


@pytest.mark.parametrize("name", NAMES)
def test_three_shapes_collected_two_steps_late(tt, corpora, name):
    c = corpora(name)
    p = Pipe(tt, c)
    shapes = [c.shapes[0], c.shapes[-2], c.shapes[-1]]              # (1, 10), then (33, 50) / (130, 10), then (33, 100)
    hs = []
    for t in range(6):
        hs.append(p.submit(*shapes[t % 3], start=17 * t))
        if t >= 2:
            p.result(hs[t - 2])
    p.result(hs[4])
    p.result(hs[5])


@pytest.mark.parametrize("name", NAMES)
def test_search_between_submit_and_result_and_result_twice(tt, corpora, name):
    c = corpora(name)
    p = Pipe(tt, c)
    h = p.submit(33, 10, start=5)
    p.search(33, 10, start=60)                                      # the step's own shape: search() has a slot of its own
    p.search(1, 10, start=7)
    a = p.result(h)
    p.search(33, 10, start=90)
    b = p.result(h)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    h2 = p.submit(33, 10, start=9)
    p.result(h)                                                     # one further submit of its shape: still its rows
    p.result(h2)


@pytest.mark.parametrize("name", NAMES)
def test_steps_with_exclude_candidates_and_keep(tt, corpora, name):
    c = corpora(name)
    p = Pipe(tt, c)
    hs = [p.submit(33, 10, start=3, extra="exclude", E=5, draw=1), p.submit(33, 10, start=50, extra="exclude", E=60, draw=2),
          p.submit(33, 10, start=20, extra="candidates", draw=3), p.submit(1, 10, start=2, extra="candidates", draw=4),
          p.submit(33, 10, start=70, extra="keep", draw=5), p.submit(33, 100, start=11, extra="keep", draw=6)]
    # six steps in flight over five shapes ((33, 50, 10) twice: candidates, then keep), collected last first
    for h in reversed(hs):
        p.result(h)
    first = p.result(hs[0])
    assert first[0] is p.pending[hs[0]].result()[0]                 # a filtered step keeps its own tensors
    for start in (1, 2):                                            # ... also once two more steps of its shape have gone by
        p.submit(33, 10, start=start, extra="exclude", E=5, draw=7)
    assert not p.pm.history.valid(hs[0])
    p.result(hs[0])


@pytest.mark.parametrize("name", NAMES)
def test_remove_ids_between_a_submit_and_its_result(tt, corpora, name):
    """The submitted step was enqueued first on the same stream: it keeps its pre-removal answer.  The next step sees the
    removal.  Once for the first removal (which allocates the mask), once with the mask in place."""
    c = corpora(name)
    p = Pipe(tt, c)
    for round_ in range(2):
        h0 = p.submit(33, 10, start=0)
        gone = np.concatenate([p.remove(start, 3) for start in (0, 5, 32)])
        h1 = p.submit(33, 10, start=0)                              # the same queries
        before, after = p.result(h0), p.result(h1)
        assert np.isin(gone, before[1].cpu().numpy()).all() and not np.isin(after[1].cpu().numpy(), gone).any()
        p.search(33, 10, start=0)
        assert p.ix.keep_mask is not None


@pytest.mark.parametrize("name", NAMES)
def test_a_step_whose_slot_set_was_retired_returns_its_own_answer(tt, corpora, name):
    c = corpora(name)
    p = Pipe(tt, c)
    hx = p.submit(33, 10, start=3)
    key = next(iter(p.ix._slots))
    assert key[:3] == (33, 50, 10)
    for k in range(11, 11 + p.ix._MAX_SLOT_SHAPES + 1):             # more shapes than slot sets are kept
        p.result(p.submit(1, k, start=k))
    assert key not in p.ix._slots and len(p.ix._slots) == p.ix._MAX_SLOT_SHAPES
    p.result(hx)
    hy = p.submit(33, 10, start=30)                                 # the shape again: a new set, the count goes on
    p.result(hx)
    p.result(hy)


@pytest.mark.parametrize("name", NAMES)
def test_steps_that_are_never_collected(tt, corpora, name):
    c = corpora(name)
    p = Pipe(tt, c)
    p.submit(33, 10, start=0)
    p.submit(1, 10, start=1)
    p.submit(33, 10, start=2)
    p.search(33, 10, start=3)
    for start in (4, 5, 6):
        h = p.submit(33, 10, start=start)
    p.result(h)
    p.result(p.submit(1, 10, start=8))


@pytest.mark.parametrize("name", NAMES)
def test_result_of_a_step_whose_slot_was_taken_raises(tt, corpora, name):
    c = corpora(name)
    p = Pipe(tt, c)
    hs = [p.submit(33, 10, start=s) for s in (0, 40, 80)]
    p.submit(1, 10, start=0)
    p.expired(hs[0])
    p.result(hs[1])
    p.result(hs[2])
    p.expired(hs[0])


@pytest.mark.parametrize("seed", (1, 2, 3))
@pytest.mark.parametrize("name", NAMES)
def test_random_pipelined_sequences(tt, corpora, name, seed):
    c = corpora(name)
    p = Pipe(tt, c)
    for op in im.sequence(seed, 40, c.shapes, SHARD_K):
        print(op)
        getattr(p, op[0])(*op[1:])
    print(f"{p.n_results} results over {len(p.shapes_used)} shapes")
    assert p.n_results >= im.MIN_RESULTS and len(p.shapes_used) >= 3


# ---- b. one index, many calls ---------------------------------------------------------------------------------------------------

K_E = ((10, 0), (64, 0), (65, 0), (100, 0), (10, 5), (10, 54), (10, 55), (60, 10), (64, 5))   # k, and k + E, on both sides of 64


class One:
    """One BruteForceIndex / StreamedIndex and its IndexModel, given the same calls."""

    def __init__(self, tt, c):
        self.tt, self.c = tt, c
        self.ix = c.single(tt)
        self.model = c.model()
        self.gone = np.zeros(0, dtype=np.int64)

    def take(self, start, B):
        rows = im.pool_rows(start, B)
        return self.c.Qd[dev(rows)].contiguous(), self.c.S[rows]

    def keep(self, rs, p=0.5):
        if rs.rand() >= p:
            return None, None
        mask = rs.rand(self.c.N) < 0.5
        return mask, self.c.pack(self.tt, mask)

    def search(self, rs):
        k, E = K_E[rs.randint(len(K_E))]
        B = (0, 1, 33)[rs.randint(3)]                                # 0: a single query vector
        q, S = self.take(rs.randint(im.POOL), max(B, 1))
        mask, keep = self.keep(rs, 0.4)
        ex = top_lists(self.model, S, E, rs, mask) if E else None
        cand = im.random_candidates(rs, S.shape[0], 200, self.c.N, OFF) if rs.rand() < 0.3 else None
        kw = {"keep": keep, "exclude": None if ex is None else dev(ex), "candidates": None if cand is None else dev(cand)}
        what = f"search B={B} k={k} E={E} keep={mask is not None} candidates={cand is not None}"
        if B == 0:
            got = self.ix.search(q[0], k, **{n: (v[0] if v is not None and n != "keep" else v) for n, v in kw.items()})
            assert got[0].shape == (k,) and got[1].shape == (k,)
            got = (got[0][None], got[1][None])
        elif rs.rand() < 0.5:
            out = (torch.full((B, k), 7.0, device="cuda"), torch.full((B, k), 7, dtype=torch.int64, device="cuda"))
            got = self.ix.search(q, k, out=out, **kw)
            assert got[0] is out[0] and got[1] is out[1]
            what += " out="
        else:
            got = self.ix.search(q, k, **kw)
        want = self.model.search(S, k, mask, ex, cand)
        same(got, want, what)
        # what was returned is consistent with the index's other calls
        vals, idx = got[0].contiguous(), got[1].contiguous()
        assert torch.equal(self.ix.score_ids(q, idx, keep=keep), vals), "score_ids of the returned ids"
        n_real = (idx >= 0).sum(1)
        kth = torch.where(n_real > 0, vals.gather(1, (n_real - 1).clamp(min=0)[:, None])[:, 0], torch.full_like(vals[:, 0], float("inf")))
        cnt = self.ix.count(q, kth, keep=keep)
        assert bool((cnt >= n_real).all()), "count at the last returned value"
        assert np.array_equal(cnt.cpu().numpy(), self.model.count(S, kth.cpu().numpy(), mask))
        if ex is None and cand is None:
            thr = vals[:, k // 2].contiguous()
            rc, rv, ri = self.ix.range_search(q, thr, k, keep=keep)
            assert torch.equal(rc, self.ix.count(q, thr, keep=keep))
            cut = ~(vals >= thr[:, None])
            assert torch.equal(rv, vals.masked_fill(cut, float("-inf"))) and torch.equal(ri, idx.masked_fill(cut, -1))
            wc, wv, wi = self.model.range_search(S, thr.cpu().numpy(), k, mask)
            assert np.array_equal(rc.cpu().numpy(), wc)
            same((rv, ri), (wv, wi), "range_search at the middle value")

    def count(self, rs):
        B = (0, 1, 33)[rs.randint(3)]
        q, S = self.take(rs.randint(im.POOL), max(B, 1))
        mask, keep = self.keep(rs)
        thr = (0.1, -0.05, float("nan"), float("-inf"), None)[rs.randint(5)]
        if thr is None:                                               # one threshold per query: a score of its own row
            t = np.ascontiguousarray(S[:, rs.randint(self.c.N)])
            got, want = self.ix.count(q, dev(t), keep=keep), self.model.count(S, t, mask)
        else:
            got, want = self.ix.count(q[0] if B == 0 else q, thr, keep=keep), self.model.count(S, thr, mask)
            got = got[None] if B == 0 else got
        assert got.dtype == torch.int64 and np.array_equal(got.cpu().numpy(), want), f"count thr={thr}"

    def score_ids(self, rs):
        B = (0, 1, 33)[rs.randint(3)]
        q, S = self.take(rs.randint(im.POOL), max(B, 1))
        mask, keep = self.keep(rs)
        ids = im.random_candidates(rs, S.shape[0], 77, self.c.N, OFF)
        got = self.ix.score_ids(q[0], dev(ids[0]), keep=keep)[None] if B == 0 else self.ix.score_ids(q, dev(ids), keep=keep)
        assert np.array_equal(got.cpu().numpy(), self.model.score_ids(S, ids, mask)), "score_ids"

    def range_search(self, rs):
        B = (0, 1, 33)[rs.randint(3)]
        k = (10, 64, 100)[rs.randint(3)]
        q, S = self.take(rs.randint(im.POOL), max(B, 1))
        mask, keep = self.keep(rs)
        thr = (0.2, 0.0, float("nan"), float("inf"))[rs.randint(4)]
        got = self.ix.range_search(q[0] if B == 0 else q, thr, k, keep=keep)
        got = tuple(g[None] for g in got) if B == 0 else got
        wc, wv, wi = self.model.range_search(S, thr, k, mask)
        assert np.array_equal(got[0].cpu().numpy(), wc), f"range_search counts thr={thr}"
        same(got[1:], (wv, wi), f"range_search thr={thr} k={k}")

    def remove(self, rs):
        """Withdraw the best documents of a few pool queries; the NEXT answer of every route is without them."""
        starts = rs.randint(0, im.POOL, size=3)
        ids = np.concatenate([self.model.search(self.c.S[s:s + 1], 2)[1].ravel() for s in starts])
        ids = np.concatenate([ids[ids >= 0], [OFF + self.c.N, OFF - 1, -1]]).astype(np.int64)
        self.ix.remove_ids(dev(ids) if rs.rand() < 0.5 else ids.tolist())
        self.model.remove(ids)
        self.gone = np.union1d(self.gone, ids[:-3])
        s = int(starts[0])
        for B, k in self.c.shapes:
            q, S = self.take(s, B)
            got = self.ix.search(q, k)
            same(got, self.model.search(S, k), f"after remove_ids: search({B}, {k})")
            assert not np.isin(got[1].cpu().numpy(), self.gone).any()
        q, S = self.take(s, 33)
        cand = np.tile(np.concatenate([self.gone, self.model.search(S[:1], 5)[1].ravel()]), (33, 1))
        got = self.ix.search(q, 10, candidates=dev(cand))
        same(got, self.model.search(S, 10, candidates=cand), "after remove_ids: candidates that name the removed")
        assert not np.isin(got[1].cpu().numpy(), self.gone).any()
        assert bool(torch.isneginf(self.ix.score_ids(q, dev(np.tile(self.gone, (33, 1))))).all())


@pytest.mark.parametrize("seed", (1, 2))
@pytest.mark.parametrize("name", NAMES)
def test_random_calls_on_one_index(tt, corpora, name, seed):
    o = One(tt, corpora(name))
    rs = np.random.RandomState(100 * seed + NAMES.index(name))
    kinds = ["search", "remove"] + list(rs.choice(["search", "count", "score_ids", "range_search", "remove"], size=16,
                                                  p=[0.5, 0.12, 0.12, 0.12, 0.14]))
    for kind in kinds:
        print(kind)
        getattr(o, kind)(rs)
    assert len(o.gone) >= 2 and o.ix.keep_mask is not None


# ---- graphs ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ("small_f32", "small_bf16", "screened", "screened_masked"))
def test_graph_captured_under_a_mask_follows_later_removals(tt, corpora, name):
    o = One(tt, corpora(name))
    rs = np.random.RandomState(7)
    o.remove(rs)                                                    # the mask exists before the capture
    g = tt.GraphedSearch(o.ix, 33, 10)
    for step in range(3):
        q, S = o.take(40 * step, 33)
        got = g(q)
        same(got, o.model.search(S, 10), f"replay {step}")
        assert not np.isin(got[1].cpu().numpy(), o.gone).any()
        ids = o.model.search(S, 2)[1].ravel()                       # every query's two best go, for the next replay
        o.ix.remove_ids(dev(ids))
        o.model.remove(ids)
        o.gone = np.union1d(o.gone, ids)
        same(g(q), o.model.search(S, 10), f"replay {step} after its best were removed")


@pytest.mark.parametrize("name", ("small_f32", "screened"))
def test_graph_captured_before_the_first_removal_raises_after_it(tt, corpora, name):
    o = One(tt, corpora(name))
    g = tt.GraphedSearch(o.ix, 33, 10)
    q, S = o.take(11, 33)
    same(g(q), o.model.search(S, 10), "replay before any removal")
    o.remove(np.random.RandomState(8))
    with pytest.raises(RuntimeError, match="captured before the index had a keep-bitmask"):
        g(q)
    same(tt.GraphedSearch(o.ix, 33, 10)(q), o.model.search(S, 10), "a new capture")
