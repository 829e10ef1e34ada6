"""The index model (tests/index_model.py) checked before it checks anything: on corpora small enough to enumerate, its
selections against an independent formulation -- Python's sorted() over (-score, id) tuples after explicit filtering --
and its pipeline bookkeeping, together with the product's host-only slot helper (index._SlotTurns), against a simulation
of which step's rows every slot holds.  The search flavours of the model (tagged, biased, cursor, mining, collapsed,
diverse) are held to the *_ref modules' `expected` over the oracle, or to a full sort, with removals and a call keep in
force, and the generators of tests/test_index_flavour_sequences_gpu.py to the floor that test relies on.  No GPU."""
import numpy as np
import pytest

import biased_ref
import collapse_ref
import cursor_ref
import index_model as im
import mmr_ref
import tagged_ref


def scores_f64(Q, D):
    """Integer-valued rows: every product and partial sum is a small integer, exact in fp32 in any order."""
    return (Q.astype(np.float64) @ D.astype(np.float64).T).astype(np.float32)


def tiny(seed, N=37, d=8, B=6, off=1000):
    rs = np.random.RandomState(seed)
    D = rs.randint(-2, 3, size=(N, d)).astype(np.float32)
    D[N // 2:N // 2 + 6] = D[:6]                                   # duplicated rows: tied scores for every query
    Q = rs.randint(-2, 3, size=(B, d)).astype(np.float32)
    m = im.IndexModel(D, off, scores_f64)
    return rs, m, m.scores(Q)


def by_sorting(m, s, k, keep=None, exclude=(), candidates=None):
    """One row, the long way: every document with its global id, filtered one condition at a time, sorted, cut."""
    pairs = []
    for n in range(m.N):
        gid = n + m.idx_offset
        if m.removed[n] or (keep is not None and not keep[n]) or gid in set(int(x) for x in exclude):
            continue
        if candidates is not None and gid not in set(int(x) for x in candidates):
            continue
        pairs.append((-float(s[n]), gid))
    pairs = sorted(pairs)[:k]
    v = [-p[0] for p in pairs] + [-np.inf] * (k - len(pairs))
    i = [p[1] for p in pairs] + [-1] * (k - len(pairs))
    return np.array(v, dtype=np.float32), np.array(i, dtype=np.int64)


def lists(rs, m, B, C):
    """[B,C] global ids with everything a list may hold: documents, repeats, negatives, other indexes' ids."""
    c = rs.randint(-3, m.N + 5, size=(B, C)).astype(np.int64) + m.idx_offset
    c[:, :2] = rs.randint(0, m.idx_offset, size=(B, 2))            # below the offset: another index's documents
    c[:, 2] = -1
    c[:, 3] = c[:, 4]                                              # a repeat
    return c


def test_the_oracle_chain_on_integer_rows_is_the_exact_product(oracle):
    rs, m, S = tiny(0)
    assert np.array_equal(oracle.score_all(rs.randint(-2, 3, size=(4, 8)).astype(np.float32), m.rows).shape, (4, m.N))
    Q = rs.randint(-2, 3, size=(5, 8)).astype(np.float32)
    assert np.array_equal(oracle.score_all(Q, m.rows), scores_f64(Q, m.rows))
    assert m.scores(Q) is m.scores(Q.copy()) and not m.scores(Q).flags.writeable    # cached per query batch


@pytest.mark.parametrize("seed", range(4))
def test_search_equals_sorted_tuples(seed):
    rs, m, S = tiny(seed)
    B = S.shape[0]
    assert any(len(np.unique(S[b])) < m.N // 2 for b in range(B))  # ties abound
    m.remove(np.concatenate([rs.randint(0, m.N, size=5) + m.idx_offset, [-4, 3, m.idx_offset + m.N]]))   # + three ignored
    assert 1 <= m.removed.sum() <= 5
    keep = rs.rand(m.N) < 0.6
    ex, cand = lists(rs, m, B, 9), lists(rs, m, B, 14)
    pad = np.full((B, 7), -1, dtype=np.int64)
    pad[:, 1] = 5                                                  # a local number: not an id of this index
    for k in (1, 5, m.N, m.N + 9):
        for kw in ({}, {"keep": keep}, {"exclude": ex}, {"candidates": cand}, {"keep": keep, "exclude": ex, "candidates": cand},
                   {"candidates": pad}, {"exclude": pad}):
            v, i = m.search(S, k, **kw)
            assert v.dtype == np.float32 and i.dtype == np.int64 and v.shape == i.shape == (B, k)
            for b in range(B):
                wv, wi = by_sorting(m, S[b], k, kw.get("keep"), kw["exclude"][b] if "exclude" in kw else (),
                                    kw["candidates"][b] if "candidates" in kw else None)
                assert np.array_equal(v[b], wv) and np.array_equal(i[b], wi), (k, sorted(kw), b)
        v, i = m.search(S, k, candidates=pad)
        assert (i == -1).all() and np.isneginf(v).all()            # an all-padding list: the tail only
        live = int((~m.removed).sum())
        assert ((m.search(S, k)[1] >= 0).sum(1) == min(k, live)).all()
        # the pieces test_exclude_gpu.py states its expectations with say the same
        mask = m.live(keep)
        a = im.idiom(S, ex, k, m.idx_offset, mask)
        b_ = m.search(S, k, keep=keep, exclude=ex)
        assert np.array_equal(a[0], b_[0]) and np.array_equal(a[1], b_[1])
        E = ex.shape[1]
        wide = m.search(S, k + E, keep=keep)                       # submit(exclude=): the search for k + E, filtered
        c = im.filter_ref(wide[0], wide[1], ex, k)
        assert np.array_equal(c[0], b_[0]) and np.array_equal(c[1], b_[1])


@pytest.mark.parametrize("seed", range(3))
def test_count_score_ids_and_range_search_by_enumeration(seed):
    rs, m, S = tiny(10 + seed)
    B = S.shape[0]
    m.remove(rs.randint(0, m.N, size=4) + m.idx_offset)
    keep = rs.rand(m.N) < 0.7
    for kp in (None, keep):
        live = [n for n in range(m.N) if not m.removed[n] and (kp is None or kp[n])]
        for thr in (0.0, 3.0, -np.inf, np.inf, np.nan, S[:, 3].copy()):
            t = np.broadcast_to(np.asarray(thr, dtype=np.float32), (B,))
            want = [sum(1 for n in live if S[b, n] >= t[b]) for b in range(B)]
            got = m.count(S, thr, kp)
            assert got.dtype == np.int64 and got.tolist() == want
            if isinstance(thr, float) and thr != thr:
                assert not got.any()                               # a NaN threshold counts nothing
            for k in (4, m.N + 2):
                c, v, i = m.range_search(S, thr, k, kp)
                assert c.tolist() == want
                for b in range(B):
                    pairs = sorted((-float(S[b, n]), n + m.idx_offset) for n in live if S[b, n] >= t[b])[:k]
                    assert i[b].tolist() == [p[1] for p in pairs] + [-1] * (k - len(pairs))
                    assert v[b].tolist() == [-p[0] for p in pairs] + [-np.inf] * (k - len(pairs))
        ids = lists(rs, m, B, 11)
        got = m.score_ids(S, ids, kp)
        assert got.dtype == np.float32
        for b in range(B):
            for c in range(ids.shape[1]):
                n = int(ids[b, c]) - m.idx_offset
                real = ids[b, c] >= 0 and n in live
                assert got[b, c] == (S[b, n] if real else -np.inf)
    v, i = m.search(S, 5)                                          # what search returns, score_ids returns for its ids
    assert np.array_equal(m.score_ids(S, i), v)


def test_removals_are_seen_by_every_method_and_k_beyond_the_corpus_pads():
    rs, m, S = tiny(20)
    v0, i0 = m.search(S, m.N + 3)
    assert (i0[:, m.N:] == -1).all() and (i0[:, :m.N] >= 0).all()
    gone = np.unique(i0[:, :2])
    m.remove(gone)
    v1, i1 = m.search(S, m.N + 3)
    assert not np.isin(i1, gone).any() and ((i1 >= 0).sum(1) == m.N - len(gone)).all()
    assert np.isneginf(m.score_ids(S, np.tile(gone, (S.shape[0], 1)))).all()
    assert (m.count(S, -np.inf) == m.N - len(gone)).all()
    m.remove(np.arange(m.N) + m.idx_offset)
    v2, i2 = m.search(S, 3)
    assert (i2 == -1).all() and np.isneginf(v2).all() and not m.count(S, -np.inf).any()


# ---- the slots of ShardedIndex.submit() ---------------------------------------------------------------------------------------

A, B_, C_ = (33, 50, 10), (1, 50, 10), (33, 100, 100)


def drive_turns(shapes, turns=None):
    """Submit `shapes` in order through the product's helper, keeping which step's rows every slot holds.  After every
    submit, for EVERY earlier step: the model's history, the helper's holds() and the slot's actual holder agree."""
    from twotowermlretrieval_amd.index import _SlotTurns
    turns = _SlotTurns() if turns is None else turns
    hist, holder, taken = im.SubmitHistory(), {}, []
    for shape in shapes:
        which, generation = turns.take(shape)
        assert which in (0, 1)
        h = hist.submit(shape)
        holder[(shape, which)] = h
        taken.append((shape, which, generation))
        for e, (s, w, g) in enumerate(taken):
            intact = holder[(s, w)] == e
            assert hist.valid(e) == intact, (f"step {e} of shape {s}: the rule says "
                                             f"{'valid' if hist.valid(e) else 'expired'}, its slot holds step {holder[(s, w)]}")
            assert turns.holds(s, g) == intact, (e, s)
    return taken


def test_slots_alternate_per_shape_a_b_a():
    """submit(A), submit(B), submit(A'): the first A must still own its slot (ONE further submit of its shape).  A parity
    shared by all shapes gives both A steps slot 0."""
    taken = drive_turns([A, B_, A])
    assert [t[1] for t in taken] == [0, 0, 1] and [t[2] for t in taken] == [0, 0, 1]


@pytest.mark.parametrize("seed", range(5))
def test_slots_over_mixed_sequences(seed):
    rs = np.random.RandomState(seed)
    pool = [A, B_, C_, (130, 50, 10), (33, 50, 15)][:2 + seed % 4]
    taken = drive_turns([pool[rs.randint(len(pool))] for _ in range(60)] + [A, B_, A, A, B_, C_, A, B_, C_])
    per_shape = {}
    for s, w, g in taken:                                          # per shape: generations 0, 1, 2, ... on slots 0, 1, 0, ...
        assert g == per_shape.get(s, 0) and w == g % 2
        per_shape[s] = g + 1


def test_pipeline_model_expiry_and_collected_exclude_steps():
    rs, m, S = tiny(30)
    pm = im.PipelineModel(m, shard_k=50)
    ex = lists(rs, m, S.shape[0], 5)
    h0 = pm.submit(S, 4)
    he = pm.submit(S, 4, exclude=ex)                                # (B, 50, 9): another shape
    m.remove(pm.result(h0)[1][:, 0])                                # after the submits: they keep their answers
    h1 = pm.submit(S, 4)
    assert not np.array_equal(pm.result(h1)[1], pm.result(h0)[1]) and not np.isin(pm.result(h1)[1], pm.result(h0)[1][:, 0]).any()
    got = pm.result(he)
    assert pm.search(S[:2], 3)[0].shape == (2, 3)                   # search() expires nothing
    h2 = pm.submit(S, 4)
    assert not pm.valid(h0) and pm.valid(h1) and pm.valid(h2) and pm.valid(he)
    with pytest.raises(AssertionError):
        pm.result(h0)
    pm.submit(S, 4, exclude=ex), pm.submit(S, 4, exclude=ex)
    assert pm.valid(he) and pm.result(he) is got                    # collected once: its own rows, for good
    hu = pm.submit(S, 5, exclude=ex)
    pm.submit(S, 5, exclude=ex), pm.submit(S, 5, exclude=ex)
    assert not pm.valid(hu)                                         # never collected: expired like any step


SEQUENCE_CASES = [(seed, shapes) for seed in (1, 2, 3)
                  for shapes in (((1, 10), (33, 10), (33, 50), (33, 100)), ((1, 10), (33, 10), (33, 50), (130, 10), (33, 100)))]


@pytest.mark.parametrize("seed,shapes", SEQUENCE_CASES)
def test_random_sequences_collect_enough_and_stay_judgeable(seed, shapes):
    """What tests/test_index_sequences_gpu.py relies on: 40 calls collect at least 15 results over at least three shapes,
    every result() is of a step the history calls valid at that point, every "expired" one of a step it calls expired."""
    ops = im.sequence(seed, 40, shapes, 50)
    assert len(ops) == 40 and ops == im.sequence(seed, 40, shapes, 50)
    hist, n_results, used, filtered, kept = im.SubmitHistory(), 0, set(), set(), set()
    for op in ops:
        if op[0] == "submit":
            _, B, k, start, extra, E, draw = op
            assert (B, k) in shapes and 0 <= start < im.POOL and (E > 0) == (extra == "exclude") and k + E <= 1024
            used.add(im.step_shape(B, k, E, 50))
            h = hist.submit(im.step_shape(B, k, E, 50))
            filtered |= {h} if E else set()
        elif op[0] == "result":
            assert hist.valid(op[1]) or op[1] in kept
            kept |= {op[1]} & filtered
            n_results += 1
        elif op[0] == "expired":
            assert not hist.valid(op[1]) and op[1] not in kept
        else:
            assert op[0] in ("search", "remove")
    assert n_results >= im.MIN_RESULTS and len(used) >= 3 and len({(s[0], s[2]) for s in used}) >= 3
    assert {o[0] for seed_, sh in SEQUENCE_CASES for o in im.sequence(seed_, 40, sh, 50)} == {"submit", "result", "expired",
                                                                                               "search", "remove"}


# ---- the search flavours ------------------------------------------------------------------------------------------------------

def small(oracle, seed, N=300, d=16, B=9, off=1000):
    """Integer-valued rows with duplicates (ties for every query), the oracle's own scores, some removals and a call keep."""
    rs = np.random.RandomState(seed)
    D = rs.randint(-2, 3, size=(N, d)).astype(np.float32)
    D[N // 2:N // 2 + 30] = D[:30]
    Q = rs.randint(-2, 3, size=(B, d)).astype(np.float32)
    m = im.IndexModel(D, off, oracle.score_all)
    S = m.scores(Q)
    m.remove(np.concatenate([rs.randint(0, N, size=25) + off, [-2, 7, off + N]]))
    keep = rs.rand(N) < 0.6
    return rs, m, Q, S, keep


def eq(got, want, what=""):
    assert got[0].dtype == np.float32 and got[1].dtype == np.int64, what
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[0], want[0]), what


@pytest.mark.parametrize("seed", range(3))
def test_tagged_model_equals_tagged_ref(oracle, seed):
    rs, m, Q, S, keep = small(oracle, 40 + seed)
    B = len(Q)
    m.set_tags(rs.randint(0, 8, size=m.N) | (rs.randint(0, 4, size=m.N) << 8) | (int(seed == 0) << 31))
    mm, mv = im.draw_filters(rs, B)
    assert len({(int(a), int(b)) for a, b in zip(mm, mv)}) >= len(im.FILTERS)
    for kp in (None, keep):
        elig = tagged_ref.eligibility(m.tags, mm, mv, ~m.removed if kp is None else ~m.removed & kp)
        assert elig.any(1).sum() < B and elig.all(1).sum() == 0     # a filter that matches nothing; the removals bind
        for k in (1, 10, 64):
            got = m.tagged_search(S, k, mm, mv, kp)
            eq(got, tagged_ref.expected(oracle, Q, m.rows, elig, k, range(B), m.idx_offset), (k, kp is None))
            assert (got[1][~elig.any(1)] == -1).all() and np.isneginf(got[0][~elig.any(1)]).all()
        eq(m.tagged_search(S, 10, 0, 0, kp), m.search(S, 10, kp), "mask 0 / value 0 is no filter")
        eq(m.tagged_search(S, 5, 0x7, 3, kp), m.tagged_search(S, 5, np.full(B, 0x7), np.full(B, 3), kp), "ints are every query's words")


@pytest.mark.parametrize("seed", range(3))
def test_biased_model_equals_biased_ref(oracle, seed):
    rs, m, Q, S, keep = small(oracle, 50 + seed)
    B = len(Q)
    ex = lists(rs, m, B, 6)
    for name, bias in biased_ref.bias_patterns(m.N, seed).items():
        if name not in im.BIAS_CYCLE + ("zero",):
            continue
        m.set_bias(bias)
        for kp in (None, keep):
            live = m.live(kp)
            for k in (1, 10, 64):
                eq(m.biased_search(S, k, kp), biased_ref.expected(oracle, Q, m.rows, bias, k, range(B), live, m.idx_offset), (name, k))
            eq(m.biased_search(S, 10, kp, ex), im.idiom(m.biased_scores(S), ex, 10, m.idx_offset, live), (name, "exclude"))
            if name == "zero":
                eq(m.biased_search(S, 10, kp), m.search(S, 10, kp), "a bias of zeros")
    m.set_bias(None)
    with pytest.raises(AssertionError):
        m.biased_search(S, 10)


@pytest.mark.parametrize("seed", range(3))
def test_cursor_model_equals_cursor_ref(oracle, seed):
    rs, m, Q, S, keep = small(oracle, 60 + seed)
    B = len(Q)
    ex = lists(rs, m, B, 6)
    first = m.search(S, 40)
    for kp in (None, keep):
        live = m.live(kp)
        col = rs.randint(0, 40, size=B)
        cursors = [(first[0][np.arange(B), col], first[1][np.arange(B), col]),                  # a place of a previous result
                   (np.full(B, np.nan, np.float32), np.full(B, m.idx_offset + 3)),               # NaN: nothing is eligible
                   (S[:, 0].copy(), np.full(B, m.idx_offset + m.N + 50)),                        # an id beyond the corpus
                   (S[:, np.flatnonzero(m.removed)[0]].copy(), np.full(B, m.idx_offset + np.flatnonzero(m.removed)[0])),
                   (np.float32(np.inf), -1), (np.float32(-np.inf), -1), (np.float32(1.0), -1)]
        for n, (av, ai) in enumerate(cursors):
            for k in (1, 10, 64):
                got = m.search_after(S, k, (av, ai), kp)
                eq(got, cursor_ref.expected(oracle, Q, m.rows, av, ai, k, range(B), m.idx_offset, live), (n, k))
                if n == 1:
                    assert (got[1] == -1).all()
            wide = m.search_after(S, 10 + ex.shape[1], (av, ai), kp)
            eq(m.search_after(S, 10, (av, ai), kp, ex), im.filter_ref(wide[0], wide[1], ex, 10), (n, "exclude"))
        eq(m.search_after(S, 10, None, kp), m.search(S, 10, kp), "the open cursor")
        # the lower twin as cursor: the next page begins with the upper twin, at the same score
        nxt = m.search_after(S, 3, (first[0][:, 0], first[1][:, 0]))
        tied = first[0][:, 0] == first[0][:, 1]
        assert tied.any() and np.array_equal(nxt[1][tied, 0], first[1][tied, 1]) and np.array_equal(nxt[0][tied, 0], first[0][tied, 0])
        pages = m.pages(S, 10, 7, kp)
        cat = (np.concatenate([p[0] for p in pages], 1), np.concatenate([p[1] for p in pages], 1))
        eq(cat, m.search(S, 70, kp), "7 pages of 10")
        eq(m.deep_search(S, 70, kp), cat, "deep_search(70)")
        eq(m.deep_search(S, m.N + 9, kp), m.search(S, m.N + 9, kp), "deeper than the corpus: the tail")


@pytest.mark.parametrize("seed", range(3))
def test_mining_model_equals_cursor_ref_over_the_live_rows(oracle, seed):
    rs, m, Q, S, keep = small(oracle, 70 + seed)
    B, off = len(Q), m.idx_offset
    pos = np.stack([np.concatenate([rs.randint(0, m.N, size=2) + off, [np.flatnonzero(m.removed)[b], -1, off + m.N + 2][b % 3:b % 3 + 1]])
                    for b in range(B)]).astype(np.int64)
    pos[:, 2] += np.where(np.arange(B) % 3 == 0, off, 0)
    for kp in (None, keep):
        live = np.flatnonzero(m.live(kp))
        sub = np.full(m.N, len(live) + 5)                            # a positive that is not live: no document of the sub-corpus
        sub[live] = np.arange(len(live))
        loc, ok = m.local(pos)
        pos_sub = np.where(ok, sub[loc], np.where(pos < 0, pos, len(live) + 7)).astype(np.int64)
        for kw in ({}, {"margin": 1.5}, {"ratio": 0.5}):
            (wv, wi), c = cursor_ref.mine(np.ascontiguousarray(S[:, live]), pos_sub, 10, idx_offset=0, **kw)
            want = (wv, np.where(wi >= 0, live[np.maximum(wi, 0)] + off, -1))
            eq(m.mine(S, pos, 10, keep=kp, **kw), want, sorted(kw))
    gone = np.tile(np.flatnonzero(m.removed)[:3] + off, (B, 1))      # every positive removed: the plain top-k
    eq(m.mine(S, gone, 10, margin=2.0, keep=keep), m.search(S, 10, keep), "no valid positive")
    eq(m.mine(S, gone[:, :0], 10), m.search(S, 10), "no positives at all")


def collapse_by_sorting(m, s, k, mpg, keep=None, exclude=()):
    """One row, the long way: every eligible document sorted as tuples, then the walk with a dict."""
    pairs = sorted((-float(s[n]), n + m.idx_offset) for n in range(m.N)
                   if not m.removed[n] and (keep is None or keep[n]) and n + m.idx_offset not in set(int(x) for x in exclude))
    seen, out = {}, []
    for negs, gid in pairs:
        g = int(m.groups[gid - m.idx_offset])
        if g >= 0:
            if seen.get(g, 0) >= mpg:
                continue
            seen[g] = seen.get(g, 0) + 1
        out.append((-negs, gid, g))
    out = out[:k] + [(-np.inf, -1, -1)] * (k - len(out[:k]))
    return tuple(np.array([o[j] for o in out], dtype=t) for j, t in enumerate((np.float32, np.int64, np.int64)))


@pytest.mark.parametrize("seed", range(3))
def test_collapse_model_equals_a_full_sort(oracle, seed, monkeypatch):
    rs, m, Q, S, keep = small(oracle, 80 + seed)
    B = len(Q)
    ex = lists(rs, m, B, 6)
    g = rs.randint(0, 40, size=m.N).astype(np.int64)
    g[rs.rand(m.N) < 0.1] = -3
    m.set_groups(g)
    for prefix in (1024, 8):                                        # 8: the walk has to come back for longer prefixes
        monkeypatch.setattr(im.IndexModel, "WALK_PREFIX", prefix)
        for kp in (None, keep):
            for k, mpg, e in ((10, 1, None), (40, 1, None), (60, 2, ex), (5, 3, ex), (m.N, 1, None)):
                got = m.collapsed_search(S, k, mpg, kp, e)
                assert got[2].dtype == np.int64
                for b in range(B):
                    want = collapse_by_sorting(m, S[b], k, mpg, kp, () if e is None else e[b])
                    assert all(np.array_equal(got[j][b], want[j]) for j in range(3)), (prefix, k, mpg, b)
                if e is None:
                    want = collapse_ref.search(S, g, k, mpg, m.live(kp), m.idx_offset)
                    assert all(np.array_equal(got[j], want[j]) for j in range(3))
    m.set_groups(np.zeros(m.N, dtype=np.int64))                     # every row in one group, m = 1: one result
    v, i, gg = m.collapsed_search(S, 10, 1, keep)
    eq((v[:, :1], i[:, :1]), m.search(S, 1, keep))
    assert (i[:, 1:] == -1).all() and (gg[:, 0] == 0).all() and (gg[:, 1:] == -1).all()
    m.set_groups(-1 - rs.randint(0, 3, size=m.N).astype(np.int64))  # all groups negative: the plain search
    v, i, gg = m.collapsed_search(S, 10, 1, keep, ex)
    eq((v, i), m.search(S, 10, keep, ex))
    assert np.array_equal(gg, m.groups[i - m.idx_offset])
    m.set_groups(None)
    with pytest.raises(AssertionError):
        m.collapsed_search(S, 10, 1)


def test_diverse_model_is_its_own_search_then_mmr_ref(oracle):
    rs, m, Q, S, keep = small(oracle, 90)
    ex = lists(rs, m, len(Q), 6)
    for kp, e in ((None, None), (keep, ex)):
        eq(m.diverse_search(S, 10, 1.0, None, kp, e, oracle), m.search(S, 10, kp, e), "lambda 1: relevance alone")
        fv, fi = m.search(S, 24, kp, e)
        got = m.diverse_search(S, 6, 0.4, 24, kp, e, oracle)
        eq(got, mmr_ref.select(oracle, fv, fi, m.rows, 6, 0.4, m.idx_offset)[:2])
        assert all(set(got[1][b]) <= set(fi[b]) and len(set(got[1][b])) == 6 for b in range(len(Q)))
        assert not np.isin(got[1] - m.idx_offset, np.flatnonzero(m.removed)).any()


FLAVOUR_SEEDS = [100 * seed + n for seed in (1, 2) for n in range(5)]   # test_random_flavour_calls_on_one_index[name-seed]


@pytest.mark.parametrize("seed", FLAVOUR_SEEDS)
def test_flavour_sequences_hold_their_floor(seed):
    ops = im.flavour_sequence(seed)
    assert ops == im.flavour_sequence(seed) and len(ops) == 24
    kinds = [o[0] for o in ops]
    assert all(kinds.count(f) >= 2 for f in im.FLAVOURS) and kinds.count("remove") >= 2
    assert all(kinds.count(s) >= 1 for s in im.SETTERS)
    first = kinds.index("remove")
    assert kinds.index("identities") > first and kinds.index("masked_rounds") > first
    assert set(kinds) <= set(im.FLAVOURS) | set(im.SETTERS) | {"remove", "identities", "masked_rounds"}


@pytest.mark.parametrize("seed", (1, 2))
def test_pipelined_sequences_with_flavour_calls(seed):
    shapes = ((1, 10), (33, 10), (33, 50), (130, 10), (33, 100))
    ops = im.sequence(seed, 30, shapes, 50)
    mixed = im.with_flavours(ops, seed, (1, 33, 130))
    assert mixed == im.with_flavours(ops, seed, (1, 33, 130))
    assert [o for o in mixed if o[0] not in im.PIPE_FLAVOURS] == ops             # the pipelined calls, in their order
    assert all(sum(o[0] == f for o in mixed) >= 2 for f in im.PIPE_FLAVOURS)
    assert all(o[1] in (1, 33, 130) and 0 <= o[2] < im.POOL for o in mixed if o[0] in im.PIPE_FLAVOURS)


def test_tag_and_group_fixtures(oracle, monkeypatch):
    import synth
    assert im.n_heads(3000) == 1 and im.n_heads(3067) == 1 and im.n_heads(65536) == 7
    monkeypatch.setattr(im, "HEAD", 40)
    rs = np.random.RandomState(3)
    N = 300
    D = synth.unit_rows(3, N, 16)
    pick = rs.choice(N, 2 * im.N_TIES, replace=False)
    D[pick[im.N_TIES:]] = D[pick[:im.N_TIES]]                         # twins
    Q = synth.unit_rows(4, 30, 16)
    Q[:im.N_TIES] = D[pick[:im.N_TIES]]
    S = oracle.score_all(np.ascontiguousarray(Q), np.ascontiguousarray(D))
    pairs = im.twin_pairs(S)
    assert all(set(pairs[j]) == {pick[j], pick[im.N_TIES + j]} for j in range(im.N_TIES))
    for seed in (1, 2):
        tags = im.tag_fixture(N, pairs, seed)
        tenant, field = tags & 0x7, (tags >> 8) & 0x3
        assert tags.dtype == np.uint32 and not (tags & ~np.uint32(0x307)).any() and set(field) == {0, 1, 2, 3}
        assert set(np.flatnonzero(tenant == im.SMALL_TENANT)) == set(pairs[:3].ravel()) and set(tenant) == set(range(8))
        assert (tenant[pairs[3:, 0]] != tenant[pairs[3:, 1]]).all()
        g = im.group_fixture(S, pairs, seed)
        head = np.lexsort((np.arange(N), -S[0]))[:40]
        assert (g[head] == im.BIG_GROUP).all() and (g == im.BIG_GROUP).sum() == 40
        rest = g[g != im.BIG_GROUP]
        ids, sizes = np.unique(rest[rest >= 0], return_counts=True)
        assert sizes.max() <= 40 and sizes.min() == 1 and 0.04 < (rest < 0).mean() < 0.2 and len(set(rest[rest < 0])) > 1
        free = [j for j in range(im.N_TIES) if not np.isin(pairs[j], head).any()]
        assert any(g[pairs[j, 0]] == g[pairs[j, 1]] for j in free) and any(g[pairs[j, 0]] != g[pairs[j, 1]] for j in free)
    assert not np.array_equal(im.group_fixture(S, pairs, 1), im.group_fixture(S, pairs, 2))
    mm, mv = im.draw_filters(rs, 33)
    elig = tagged_ref.eligibility(im.tag_fixture(N, pairs, 1), mm, mv)
    assert elig.all(1).any() and (~elig.any(1)).any() and len({(int(a), int(b)) for a, b in zip(mm, mv)}) > 6
