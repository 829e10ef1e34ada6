"""The six search flavours that came after tests/test_index_sequences_gpu.py -- tagged, biased, cursor (search_after / pages /
deep_search), diverse, collapsed search and hard-negative mining -- driven through HISTORIES of calls on one index and
compared with tests/index_model.py by equality of values and indices.

Their own modules call each flavour on a fresh index.  Here the state moves between the calls: documents are removed, tags,
bias and groups are replaced or cleared, a call keep is ANDed on top, submitted steps of a ShardedIndex are in flight while
a flavour call takes a slot of its own, and a StreamedIndex hands its state to resident().  Every answer is also held
against the index's OTHER calls under the same mask (score_ids of what came back, the plain search a flavour degenerates
to).  Corpora, query pool, score matrices and thresholds are those of tests/test_index_sequences_gpu.py."""
import collections
import copy

import numpy as np
import pytest
import torch

import biased_ref
import index_model as im
from test_index_sequences_gpu import NAMES, OFF, SHARD_K, One, Pipe, dev, same, top_lists
from test_index_sequences_gpu import corpora, product_thresholds, tt  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

KMAX = 64                                             # TAGGED_KMAX = BIASED_KMAX = AFTER_KMAX
K_PLAIN = (1, 10, 63, 64, 65, 100)                    # k on both sides of the bound
K_E = ((10, 0), (64, 0), (65, 0), (100, 0), (10, 5), (10, 54), (10, 55), (60, 4), (60, 5))   # ... and k + E = 64 and 65
CURSORS = ("position", "twin", "none", "nan", "removed", "beyond")


def test_the_bounds_are_the_products(tt):
    from twotowermlretrieval_amd import index
    assert index.TAGGED_KMAX == index.BIASED_KMAX == index.AFTER_KMAX == KMAX


# ---- fixtures planted on the twin rows, made once per corpus ------------------------------------------------------------------

_FIXTURES = {}


class Fixtures:
    def __init__(self, c):
        self.pairs = im.twin_pairs(c.S)
        self.tags = [im.tag_fixture(c.N, self.pairs, seed) for seed in (1, 2)]
        self.groups = [im.group_fixture(c.S, self.pairs, seed) for seed in (1, 2)]
        self.bias = {name: b for name, b in biased_ref.bias_patterns(c.N, 7).items() if name in im.BIAS_CYCLE + ("zero",)}
        assert all((g == im.BIG_GROUP).sum() >= im.HEAD for g in self.groups)


def fixtures(c):
    if id(c.S) not in _FIXTURES:                      # (the score matrix lives as long as the process: its id is a key)
        _FIXTURES[id(c.S)] = Fixtures(c)
    return _FIXTURES[id(c.S)]


def words(a):
    """uint32 words as the int32 device tensor the product takes."""
    return dev(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32))


def sevens(B, k):
    return (torch.full((B, k), 7.0, device="cuda"), torch.full((B, k), 7, dtype=torch.int64, device="cuda"))


def untouched(out):
    return bool((out[0] == 7.0).all()) and bool((out[1] == 7).all())


def rows_of(got):
    """A single query's result as a batch of one."""
    return tuple(g[None] for g in got)


class State:
    """What One and Pipe share here: tags, bias and groups set on the index and on the model alike."""

    def plant(self):
        self.fx = fixtures(self.c)
        self.turn = {"tags": 0, "groups": 0, "bias": 0}
        self.put_tags(), self.put_bias(im.BIAS_CYCLE[0]), self.put_groups()

    def put_tags(self):
        t = self.fx.tags[self.turn["tags"] % 2]
        self.ix.set_tags(words(t))
        self.model.set_tags(t)

    def put_bias(self, bias):
        """A pattern's name, the values themselves, or None."""
        self.bias_name = bias if bias is None or isinstance(bias, str) else "restored"
        b = self.fx.bias[bias] if isinstance(bias, str) else bias
        self.ix.set_bias(None if b is None else dev(b))
        self.model.set_bias(b)

    def put_groups(self, g="fixture"):
        g = self.fx.groups[self.turn["groups"] % 2] if isinstance(g, str) else g
        self.ix.set_groups(None if g is None else dev(g))
        self.model.set_groups(g)

    def removed_ids(self):
        return OFF + np.flatnonzero(self.model.removed)

    def consistent(self, got, q, keep, what, biased=False):
        """What came back, against the index's other calls under the same mask: score_ids of the returned ids are the
        returned values (+ bias[id], one float32 add, for a biased search), and no removed document is among them."""
        vals, idx = got[0].contiguous(), got[1].contiguous()
        sc = self.ix.score_ids(q, idx, keep=keep)
        if biased:
            sc = sc + dev(self.model.bias)[(idx - OFF).clamp(min=0)]      # (the tail: -inf + a finite bias = -inf)
        assert torch.equal(sc, vals), f"{what}: score_ids of the returned ids"
        assert not np.isin(idx.cpu().numpy(), self.removed_ids()).any(), f"{what}: a removed document came back"


# ---- a. one index, many calls -------------------------------------------------------------------------------------------------

class Flavours(One, State):
    """One BruteForceIndex / StreamedIndex and its IndexModel, given the same flavour calls.  Every op takes its own
    RandomState and counts itself in `ran` when it has run to its end."""

    def __init__(self, tt, c, oracle, ix=None, model=None):
        self.tt, self.c, self.oracle = tt, c, oracle
        self.ix = c.single(tt) if ix is None else ix
        self.gone = np.zeros(0, dtype=np.int64)                         # (One's: kept by remove() here as there)
        self.ran = collections.Counter()
        self.masked_rounds_seen = 0
        self.exclude_biased = isinstance(self.ix, tt.BruteForceIndex)   # (StreamedIndex.biased_search takes no exclude=)
        if model is None:
            self.model = c.model()
            self.plant()
        else:                                                           # an index that already carries the model's state
            self.model, self.fx, self.turn, self.bias_name = model, fixtures(c), {"tags": 0, "groups": 0, "bias": 0}, None

    def batch(self, rs, start=None):
        B = (0, 1, 33)[rs.randint(3)]                                   # 0: a single query vector
        start = rs.randint(im.POOL) if start is None else start
        q, S = self.take(start, max(B, 1))
        return B, q, S

    def plain_after(self, q, S, what):
        """A tagged or biased call must not leak into the next plain calls."""
        same(self.ix.search(q, 10), self.model.search(S, 10), f"search after {what}")
        assert np.array_equal(self.ix.count(q, 0.1).cpu().numpy(), self.model.count(S, 0.1)), f"count after {what}"
        rc, rv, ri = self.ix.range_search(q, 0.1, 10)
        wc, wv, wi = self.model.range_search(S, 0.1, 10)
        assert np.array_equal(rc.cpu().numpy(), wc), f"range_search counts after {what}"
        same((rv, ri), (wv, wi), f"range_search after {what}")

    # -- the flavours --

    def tagged(self, rs):
        B, q, S = self.batch(rs)
        k = K_PLAIN[rs.randint(len(K_PLAIN))]
        mask, keep = self.keep(rs, 0.4)
        mm, mv = im.draw_filters(rs, S.shape[0])
        out = sevens(B, k) if (rs.rand() < 0.5 or k > KMAX) and B else None      # over the bound: always, to see nothing written
        what = f"tagged_search B={B} k={k} keep={mask is not None} out={out is not None}"
        if B == 0:
            call = lambda: rows_of(self.ix.tagged_search(q[0], k, int(mm[0]), int(mv[0]), keep=keep))   # ints: every query's words
        else:
            call = lambda: self.ix.tagged_search(q, k, words(mm), words(mv), keep=keep, out=out)
        if k > KMAX:
            with pytest.raises(ValueError, match="tagged search answers"):
                call()
            assert out is None or untouched(out), what
        else:
            got = call()
            assert out is None or (got[0] is out[0] and got[1] is out[1])
            same(got, self.model.tagged_search(S, k, mm, mv, mask), what)
            self.consistent(got, q, keep, what)
            ids = got[1].cpu().numpy()
            t = self.model.tags[np.clip(ids - OFF, 0, self.c.N - 1)]
            assert ((ids < 0) | ((t & mm[:, None]) == mv[:, None])).all(), f"{what}: the results satisfy the filter"
        self.plain_after(q, S, what)
        self.ran["tagged"] += 1

    def biased(self, rs):
        B, q, S = self.batch(rs)
        k, E = K_E[rs.randint(len(K_E))]
        E = E if self.exclude_biased else 0
        mask, keep = self.keep(rs, 0.4)
        ex = None
        if E:                                                           # each query's own best by the biased score, two random
            ex = np.concatenate([self.model.biased_search(S, E - 2, mask)[1], rs.randint(0, self.c.N, size=(S.shape[0], 2)) + OFF], 1)
        out = sevens(B, k) if (rs.rand() < 0.5 or k + E > KMAX) and B else None  # over the bound: always, to see nothing written
        what = f"biased_search[{self.bias_name}] B={B} k={k} E={E} keep={mask is not None} out={out is not None}"
        kw = {} if ex is None else {"exclude": dev(ex[0]) if B == 0 else dev(ex)}
        if B == 0:
            call = lambda: rows_of(self.ix.biased_search(q[0], k, keep=keep, **kw))
        else:
            call = lambda: self.ix.biased_search(q, k, keep=keep, out=out, **kw)
        if k + E > KMAX:
            with pytest.raises(ValueError, match="biased search"):
                call()
            assert out is None or untouched(out), what
        else:
            got = call()
            assert out is None or (got[0] is out[0] and got[1] is out[1])
            same(got, self.model.biased_search(S, k, mask, ex), what)
            self.consistent(got, q, keep, what, biased=True)
        self.plain_after(q, S, what)
        self.ran["biased"] += 1

    def cursor(self, rs, kind, S, mask):
        """(after for the model, after for the index) of one of CURSORS over the queries of S."""
        B = S.shape[0]
        prev = self.model.search(S, 64, mask)                           # "a previous result": the first page of 64
        col = rs.randint(0, 64, size=B)
        gone = np.flatnonzero(self.model.removed)
        if kind == "removed" and len(gone) == 0:
            kind = "position"
        if kind == "none":
            return None, None
        if kind == "nan":
            return (np.float32(np.nan), OFF + 5), (float("nan"), OFF + 5)
        if kind == "twin":                                              # the lower twin: the next page begins with the upper one
            av, ai = prev[0][:, 0].copy(), prev[1][:, 0].copy()
        elif kind == "position":
            av, ai = prev[0][np.arange(B), col], prev[1][np.arange(B), col]
        elif kind == "removed":                                         # the place of a document removed since
            n = gone[rs.randint(len(gone), size=B)]
            av, ai = S[np.arange(B), n].copy(), OFF + n
        else:                                                           # an id beyond the corpus
            av, ai = prev[0][np.arange(B), col], OFF + self.c.N + 1000 + np.arange(B)
        av, ai = np.ascontiguousarray(av, dtype=np.float32), np.ascontiguousarray(ai, dtype=np.int64)
        return (av, ai), (dev(av), dev(ai))

    def after(self, rs):
        kind = CURSORS[rs.randint(len(CURSORS))]
        B = (0, 1, 33)[rs.randint(3)]
        k, E = K_E[rs.randint(len(K_E))]
        mask = rs.rand(self.c.N) < 0.5 if rs.rand() < 0.4 else None
        start = rs.randint(im.POOL)
        if kind == "twin":                                              # a tie query whose twins are both there
            whole = [j for j in range(im.N_TIES) if not self.model.removed[self.fx.pairs[j]].any()]
            start = 0 if B == 33 else whole[rs.randint(len(whole))]
            E = 0
            if mask is not None:
                mask[self.fx.pairs.ravel()] = True
        q, S = self.take(start, max(B, 1))
        keep = None if mask is None else self.c.pack(self.tt, mask)
        on_model, on_gpu = self.cursor(rs, kind, S, mask)
        ex = None
        if E:                                                           # the places right behind the cursor, and two random ids
            ex = np.concatenate([self.model.search_after(S, E - 2, on_model, mask)[1], rs.randint(0, self.c.N, size=(S.shape[0], 2)) + OFF], 1)
        out = sevens(B, k) if (rs.rand() < 0.5 or k + E > KMAX) and B else None  # over the bound: always, to see nothing written
        what = f"search_after[{kind}] B={B} k={k} E={E} keep={mask is not None} out={out is not None}"
        kw = {} if ex is None else {"exclude": dev(ex[0]) if B == 0 else dev(ex)}
        if B == 0:
            call = lambda: rows_of(self.ix.search_after(q[0], k, on_gpu, keep=keep, **kw))
        else:
            call = lambda: self.ix.search_after(q, k, on_gpu, keep=keep, out=out, **kw)
        if k + E > KMAX:
            with pytest.raises(ValueError, match="cursor search"):
                call()
            assert out is None or untouched(out), what
        else:
            got = call()
            assert out is None or (got[0] is out[0] and got[1] is out[1])
            want = self.model.search_after(S, k, on_model, mask, ex)
            same(got, want, what)
            self.consistent(got, q, keep, what)
            if kind == "twin":
                tied = np.flatnonzero((start + np.arange(S.shape[0])) % im.POOL < im.N_TIES)
                tied = tied[~self.model.removed[self.fx.pairs[(start + tied) % im.POOL]].any(1)]
                assert len(tied) and (want[0][tied, 0] == on_model[0][tied]).all() and (want[1][tied, 0] > on_model[1][tied]).all()
            if kind == "nan":
                assert (want[1] == -1).all()
        self.ran["after"] += 1

    def pages(self, rs):
        B, q, S = self.batch(rs)
        mask, keep = self.keep(rs, 0.4)
        q_ = q[0] if B == 0 else q
        if rs.rand() < 0.5:
            k = (10, 64)[rs.randint(2)]
            got = list(self.ix.pages(q_, k, n_pages=3, keep=keep))
            for n, (g, w) in enumerate(zip(got, self.model.pages(S, k, 3, mask))):
                same(rows_of(g) if B == 0 else g, w, f"page {n} of k={k} B={B} keep={mask is not None}")
            assert len(got) == 3
            self.consistent(tuple(torch.cat([rows_of(g)[j] if B == 0 else g[j] for g in got], 1) for j in range(2)), q, keep, "pages")
        else:
            k_total = (70, 130)[rs.randint(2)]
            got = self.ix.deep_search(q_, k_total, keep=keep)
            got = rows_of(got) if B == 0 else got
            same(got, self.model.deep_search(S, k_total, mask), f"deep_search({k_total}) B={B} keep={mask is not None}")
            self.consistent(got, q, keep, "deep_search")
        self.ran["pages"] += 1

    def diverse(self, rs):
        B, q, S = self.batch(rs)
        k = (5, 10, 32)[rs.randint(3)]
        lam = (1.0, 0.5, 0.3, 0.0)[rs.randint(4)]
        fk = (None, 64, 128)[rs.randint(3)]
        mask, keep = self.keep(rs, 0.4)
        ex = top_lists(self.model, S, 5, rs, mask) if rs.rand() < 0.3 else None
        kw = {} if ex is None else {"exclude": dev(ex[0]) if B == 0 else dev(ex)}
        got = self.ix.diverse_search(q[0] if B == 0 else q, k, lam, fetch_k=fk, keep=keep, **kw)
        got = rows_of(got) if B == 0 else got
        what = f"diverse_search B={B} k={k} lambda={lam} fetch_k={fk} keep={mask is not None} exclude={ex is not None}"
        same(got, self.model.diverse_search(S, k, lam, fk, mask, ex, self.oracle), what)
        self.consistent(got, q, keep, what)
        self.ran["diverse"] += 1

    def collapsed(self, rs, start=None, B=None, k=None, m=None, keep_p=0.4, exclude_p=0.3):
        if B is None:
            B, q, S = self.batch(rs, start)
        else:
            q, S = self.take(start, B)
        k = (5, 10, 40)[rs.randint(3)] if k is None else k
        m = (1, 2, 3)[rs.randint(3)] if m is None else m
        mask, keep = self.keep(rs, keep_p)
        ex = top_lists(self.model, S, 5, rs, mask) if rs.rand() < exclude_p else None
        kw = {} if ex is None else {"exclude": dev(ex[0]) if B == 0 else dev(ex)}
        got = self.ix.collapsed_search(q[0] if B == 0 else q, k, m, keep=keep, **kw)
        got = rows_of(got) if B == 0 else got
        what = f"collapsed_search B={B} k={k} m={m} keep={mask is not None} exclude={ex is not None} rounds={self.ix.collapse_rounds}"
        wv, wi, wg = self.model.collapsed_search(S, k, m, mask, ex)
        same(got[:2], (wv, wi), what)
        assert got[2].dtype == torch.int64 and np.array_equal(got[2].cpu().numpy(), wg), f"{what}: group ids"
        assert got[3].dtype == torch.int32 and bool((got[3] == 1).all()), f"{what}: exact=True ends complete"
        self.consistent(got[:2], q, keep, what)
        self.ran["collapsed"] += 1
        return mask

    def mine(self, rs):
        B, q, S = self.batch(rs)
        R = S.shape[0]
        k = (10, 61, 62)[rs.randint(3)]                                 # with P = 3: k + P = 64 and 65
        rule = ({}, {"margin": 0.05}, {"ratio": 0.95})[rs.randint(3)]
        mask, keep = self.keep(rs, 0.4)
        gone = np.flatnonzero(self.model.removed)
        odd = [np.full(R, -1), np.full(R, OFF + self.c.N + 7)] + ([OFF + gone[rs.randint(len(gone), size=R)]] if len(gone) else [])
        # the query's best document whether or not it is still there, a random one, and padding / another index's / a removed one
        pos = np.stack([OFF + np.argmax(S, 1), OFF + rs.randint(0, self.c.N, size=R), odd[rs.randint(len(odd))]], 1).astype(np.int64)
        plain = len(gone) >= 3 and rs.rand() < 0.25
        if plain:                                                       # every positive removed: the plain top-k
            pos = np.tile(OFF + gone[:3], (R, 1)).astype(np.int64)
        what = f"mine_hard_negatives B={B} k={k} {rule} keep={mask is not None} all positives removed={plain}"
        call = lambda: self.tt.mine_hard_negatives(self.ix, q[0] if B == 0 else q, dev(pos[0]) if B == 0 else dev(pos), k, keep=keep, **rule)
        if k + 3 > KMAX:
            with pytest.raises(ValueError, match="cursor search"):
                call()
        else:
            got = rows_of(call()) if B == 0 else call()
            want = self.model.mine(S, pos, k, keep=mask, **rule)
            same(got, want, what)
            self.consistent(got, q, keep, what)
            assert not (got[1].cpu().numpy()[:, :, None] == pos[:, None, :]).any(), f"{what}: a positive came back"
            if plain:
                same(got, self.model.search(S, k, mask), f"{what}: the plain top-k")
        self.ran["mine"] += 1

    # -- the state --

    def remove(self, rs):
        """The two best live documents of three pool queries -- the first time those of tie queries 0, 1, 2: their twins,
        all of the small tenant -- and three ids that are nobody's."""
        starts = (0, 1, 2) if not self.ran["remove"] else rs.randint(0, im.POOL, size=3)
        ids = np.concatenate([self.model.search(self.c.S[s:s + 1], 2)[1].ravel() for s in starts])
        ids = np.concatenate([ids[ids >= 0], [OFF + self.c.N, OFF - 1, -1]]).astype(np.int64)
        self.ix.remove_ids(dev(ids) if rs.rand() < 0.5 else ids.tolist())
        self.model.remove(ids)
        self.gone = np.union1d(self.gone, ids[:-3])
        q, S = self.take(int(starts[0]), 33)
        got = self.ix.search(q, 10)
        same(got, self.model.search(S, 10), "search after remove_ids")
        assert not np.isin(got[1].cpu().numpy(), self.removed_ids()).any()
        assert not self.model.live()[(self.model.tags & 0x7) == im.SMALL_TENANT].any(), "the small tenant is empty now"
        v, i = self.ix.tagged_search(q, 10, 0x7, im.SMALL_TENANT)
        assert bool((i == -1).all()) and bool(torch.isneginf(v).all()), "a tenant that removals emptied"
        self.ran["remove"] += 1

    def set_tags(self, rs):
        self.turn["tags"] += 1
        self.put_tags()
        self.ran["set_tags"] += 1

    def set_bias(self, rs):
        """set_bias(None): a biased_search must raise; then the next pattern of the cycle."""
        q, S = self.take(rs.randint(im.POOL), 33)
        self.put_bias(None)
        assert self.ix.bias is None
        with pytest.raises(ValueError, match="has no bias"):
            self.ix.biased_search(q, 10)
        self.turn["bias"] += 1
        self.put_bias(im.BIAS_CYCLE[self.turn["bias"] % len(im.BIAS_CYCLE)])
        same(self.ix.biased_search(q, 10), self.model.biased_search(S, 10), f"biased_search under the new bias {self.bias_name}")
        self.ran["set_bias"] += 1

    def set_groups(self, rs):
        q, S = self.take(rs.randint(im.POOL), 33)
        if rs.rand() < 0.5:
            self.put_groups(None)
            with pytest.raises(ValueError, match="has no groups"):
                self.ix.collapsed_search(q, 10)
        self.turn["groups"] += 1
        self.put_groups()
        same(self.ix.collapsed_search(q, 10, 1)[:2], self.model.collapsed_search(S, 10, 1)[:2], "collapsed_search under the new groups")
        self.ran["set_groups"] += 1

    # -- what the flavours degenerate to, and the rounds no other call reaches --

    def identities(self, rs):
        assert self.model.removed.any(), "the identities are to hold with removals in force"
        q, S = self.take(rs.randint(im.POOL), 33)
        plain = self.ix.search(q, 10)
        same(plain, self.model.search(S, 10), "the plain search of the identities")

        def is_plain(got, what):
            assert torch.equal(got[1], plain[1]) and torch.equal(got[0], plain[0]), f"{what} equals search()"

        bias = self.model.bias
        self.put_bias("zero")
        is_plain(self.ix.biased_search(q, 10), "biased_search under a bias of zeros")
        self.put_bias(bias)
        is_plain(self.ix.tagged_search(q, 10, 0, 0), "tagged_search(mask 0, value 0)")
        is_plain(self.ix.search_after(q, 10, None), "search_after(None)")
        is_plain(self.ix.diverse_search(q, 10, 1.0), "diverse_search(lambda_=1)")
        groups = self.model.groups
        self.put_groups(np.full(self.c.N, -1, dtype=np.int64))
        v, i, g, complete = self.ix.collapsed_search(q, 10, 1)
        is_plain((v, i), "collapsed_search with every row ungrouped")
        assert bool((g == -1).all()) and bool((complete == 1).all()) and self.ix.collapse_rounds == (1, 0)
        self.put_groups(groups)
        paged = list(self.ix.pages(q, 10, n_pages=7))
        paged = (torch.cat([p[0] for p in paged], 1), torch.cat([p[1] for p in paged], 1))
        deep, wide = self.ix.deep_search(q, 70), self.ix.search(q, 70)
        assert torch.equal(paged[1], deep[1]) and torch.equal(paged[0], deep[0]), "7 pages of 10 equal deep_search(70)"
        assert torch.equal(deep[1], wide[1]) and torch.equal(deep[0], wide[0]), "deep_search(70) equals search(70)"
        same(wide, self.model.search(S, 70), "search(70)")
        self.ran["identities"] += 1

    def masked_rounds(self, rs):
        """Tie query 0 (and its neighbour) under removals AND a call keep: BIG_GROUP owns more of query 0's eligible head than
        the batched rounds fetch, so exact=True must go on to the masked rounds, whose keep mask is built from the groups,
        ANDed with the call's keep and then with the removals."""
        assert self.model.removed.any()
        mask = self.collapsed(rs, start=0, B=2, k=10, m=1, keep_p=1.0, exclude_p=0.0)
        assert mask is not None and self.ix.collapse_rounds[1] > 0, f"no masked round ran: {self.ix.collapse_rounds}"
        self.masked_rounds_seen += 1
        self.ran["collapsed"] -= 1
        self.ran["masked_rounds"] += 1


@pytest.mark.parametrize("seed", (1, 2))
@pytest.mark.parametrize("name", NAMES)
def test_random_flavour_calls_on_one_index(tt, corpora, oracle, name, seed):
    o = Flavours(tt, corpora(name), oracle)
    ops = im.flavour_sequence(100 * seed + NAMES.index(name))
    for kind, draw in ops:
        print(kind, draw)
        getattr(o, kind)(np.random.RandomState(draw))
    print(dict(o.ran))
    assert sum(o.ran.values()) == len(ops), "an op was skipped"
    assert all(o.ran[f] >= 2 for f in im.FLAVOURS) and o.ran["remove"] >= 2 and all(o.ran[s] >= 1 for s in im.SETTERS)
    assert o.ran["identities"] >= 1 and o.masked_rounds_seen >= 1 and o.ix.keep_mask is not None


# ---- b. resident() carries the state ------------------------------------------------------------------------------------------

def test_resident_carries_removals_tags_bias_and_groups(tt, corpora, oracle):
    """StreamedIndex.resident() hands the new index COPIES of the keep-bitmask, tags, bias and groups: every flavour and the
    plain calls answer as the streamed index and the model do, and from then on the indexes are independent."""
    c = corpora("streamed")
    st = Flavours(tt, c, oracle)
    st.remove(np.random.RandomState(1))
    st.remove(np.random.RandomState(2))
    made = {"float32": st.ix.resident(), "bfloat16": st.ix.resident(torch.bfloat16)}
    taken = copy.deepcopy(st.model)                                      # the state resident() was taken in
    assert made["float32"].docs.dtype == torch.float32 and made["bfloat16"].docs.dtype == torch.bfloat16
    for ix in made.values():                                             # copies, not views: before any call replaces a tensor
        for mine, theirs in ((ix.keep_mask, st.ix.keep_mask), (ix.tags, st.ix.tags), (ix.bias, st.ix.bias), (ix.groups, st.ix.groups)):
            assert mine is not None and mine.data_ptr() != theirs.data_ptr() and torch.equal(mine, theirs)
    for what, ix in [("streamed", st.ix)] + list(made.items()):
        print(what)
        o = Flavours(tt, c, oracle, ix=ix, model=copy.deepcopy(st.model))
        for n, kind in enumerate(im.FLAVOURS + im.FLAVOURS + ("identities", "masked_rounds")):   # the same draws on all three
            getattr(o, kind)(np.random.RandomState(900 + n))
        q, S = o.take(3, 33)
        o.plain_after(q, S, f"on the {what} index")
    # independent from here on
    q, S = st.take(0, 33)
    before = st.model.search(S, 10)
    r32, r16 = made["float32"], made["bfloat16"]
    r32.remove_ids(dev(before[1][:, 0].copy()))                          # every query's best: gone from the fp32 copy alone
    same(st.ix.search(q, 10), before, "the streamed index after a removal on its resident copy")
    same(r16.search(q, 10), before, "the bf16 copy after a removal on the fp32 copy")
    m32 = copy.deepcopy(st.model)
    m32.remove(before[1][:, 0])
    same(r32.search(q, 10), m32.search(S, 10), "the fp32 copy after its own removal")
    st.ix.remove_ids(dev(before[1][:, 1].copy()))                        # ... and the other way round
    st.model.remove(before[1][:, 1])
    same(st.ix.search(q, 10), st.model.search(S, 10), "the streamed index after its own removal")
    same(r32.search(q, 10), m32.search(S, 10), "the fp32 copy after a removal on the streamed index")
    same(r16.search(q, 10), before, "the bf16 copy after both")
    st.ix.set_bias(None)                                                 # ... and so are the setters' tensors
    st.ix.set_groups(None)
    same(r16.biased_search(q, 10), taken.biased_search(S, 10), "the bf16 copy keeps its bias")
    same(r16.collapsed_search(q, 10, 1)[:2], taken.collapsed_search(S, 10, 1)[:2], "the bf16 copy keeps its groups")


# ---- c. the sharded pipeline ----------------------------------------------------------------------------------------------------

class FlavourPipe(Pipe, State):
    """Pipe with tags, bias and groups planted, and flavour calls of the submitted steps' own B with k = 10: per-shard
    lists of k' = 50, the submitted (B, 10) steps' own shape.  The flavour calls are no submits: the PipelineModel's history
    does not record them, they expire nothing."""

    def __init__(self, tt, c):
        Pipe.__init__(self, tt, c)
        self.plant()
        self.n_flavours = collections.Counter()

    def draw(self, B, start, draw):
        q, S = self.take(start, B)
        rs = np.random.RandomState(draw)
        mask = rs.rand(self.c.N) < 0.5 if rs.rand() < 0.4 else None
        return q, S, rs, mask, None if mask is None else self.c.pack(self.tt, mask)

    def done(self, kind, got, want, q, keep, biased=False):
        same(got, want, f"sharded {kind}")
        self.consistent(got, q, keep, f"sharded {kind}", biased)
        self.n_flavours[kind] += 1
        return got, want

    def tagged(self, B, start, draw):
        q, S, rs, mask, keep = self.draw(B, start, draw)
        mm, mv = im.draw_filters(rs, B)
        got = self.ix.tagged_search(q, 10, words(mm), words(mv), keep=keep)
        return self.done("tagged", got, self.model.tagged_search(S, 10, mm, mv, mask), q, keep)

    def biased(self, B, start, draw):
        q, S, rs, mask, keep = self.draw(B, start, draw)
        return self.done("biased", self.ix.biased_search(q, 10, keep=keep), self.model.biased_search(S, 10, mask), q, keep, True)

    def after(self, B, start, draw):
        q, S, rs, mask, keep = self.draw(B, start, draw)
        prev = self.model.search(S, 64, mask)
        col = rs.randint(0, 64, size=B)
        av, ai = np.ascontiguousarray(prev[0][np.arange(B), col]), np.ascontiguousarray(prev[1][np.arange(B), col])
        got = self.ix.search_after(q, 10, (dev(av), dev(ai)), keep=keep)
        return self.done("after", got, self.model.search_after(S, 10, (av, ai), mask), q, keep)


def batches(c):
    return sorted({B for B, _ in c.shapes})


@pytest.mark.parametrize("name", NAMES)
def test_flavour_calls_between_a_submit_and_its_result(tt, corpora, name):
    c = corpora(name)
    for B in batches(c):
        p = FlavourPipe(tt, c)
        h = p.submit(B, 10, start=5)
        p.tagged(B, 60, 1)
        p.biased(B, 70, 2)
        p.after(B, 80, 3)
        p.result(h)                                                 # its own rows, whatever the flavour calls wrote
        assert p.pm.history.shapes == [im.step_shape(B, 10, 0, SHARD_K)]


@pytest.mark.parametrize("name", NAMES)
def test_two_pending_steps_stay_collectable_through_flavour_calls(tt, corpora, name):
    c = corpora(name)
    p = FlavourPipe(tt, c)
    h0 = p.submit(33, 10, start=0)
    h1 = p.submit(33, 10, start=40)
    for t in range(2):                                              # the steps' own (B, k', k), six times
        p.tagged(33, 10 + t, 4 + t)
        p.biased(33, 20 + t, 6 + t)
        p.after(33, 30 + t, 8 + t)
    assert len(p.pm.history.shapes) == 2 and p.pm.valid(h0) and p.pm.valid(h1)
    p.result(h1)
    p.result(h0)
    h2 = p.submit(33, 10, start=80)                                 # ONE further submit of the shape: h1 still holds
    p.tagged(33, 50, 10)
    p.result(h1)
    p.result(h2)


@pytest.mark.parametrize("name", NAMES)
def test_tagged_search_and_search_after_share_a_slot_set_not_their_results(tt, corpora, name):
    """Both take slot set 2 of one (B, k', k): what the first call returned must be its own tensors, not views of the slot
    the second call writes."""
    c = corpora(name)
    p = FlavourPipe(tt, c)
    h = p.submit(33, 10, start=9)
    first, want_first = p.tagged(33, 20, 11)
    second, want_second = p.after(33, 90, 12)
    assert not np.array_equal(want_first[1], want_second[1])
    same(first, want_first, "tagged_search's tensors after a search_after of its shape")
    third, want_third = p.tagged(33, 55, 13)
    same(second, want_second, "search_after's tensors after a tagged_search of its shape")
    p.search(33, 10, start=70)                                      # search() takes the same set
    same(third, want_third, "tagged_search's tensors after a search() of its shape")
    fourth, want_fourth = p.biased(33, 56, 14)
    p.biased(33, 57, 15)
    same(fourth, want_fourth, "biased_search's tensors after another of its shape")
    p.result(h)


@pytest.mark.parametrize("name", NAMES)
def test_remove_ids_between_a_submit_and_a_flavour_call(tt, corpora, name):
    """The pending step keeps its pre-removal answer; the flavour calls that follow the removal see it."""
    c = corpora(name)
    p = FlavourPipe(tt, c)
    for round_ in range(2):                                         # the removal that allocates the mask, then one more
        h = p.submit(33, 10, start=0)
        gone = np.concatenate([p.remove(start, 3) for start in (0, 5, 32)])
        for kind in im.PIPE_FLAVOURS:
            got, _ = getattr(p, kind)(33, 0, 20 + round_)
            assert not np.isin(got[1].cpu().numpy(), gone).any(), kind
        q, S = p.take(0, 33)
        same(p.ix.tagged_search(q, 10, 0, 0), p.model.search(S, 10), "tagged_search(0, 0) after the removal")
        before = p.result(h)
        assert np.isin(gone, before[1].cpu().numpy()).all()


@pytest.mark.parametrize("name", NAMES)
def test_diverse_collapsed_and_mined_on_the_sharded_index_after_removals(tt, corpora, oracle, name):
    c = corpora(name)
    p = FlavourPipe(tt, c)
    h = p.submit(33, 10, start=0)
    for start in (0, 1, 2, 40):
        p.remove(start, 2)
    rs = np.random.RandomState(31)
    mask = rs.rand(c.N) < 0.5
    keep = c.pack(tt, mask)
    q, S = p.take(0, 33)
    for kp, kd in ((None, None), (mask, keep)):
        same(p.ix.diverse_search(q, 10, 0.5, keep=kd), p.model.diverse_search(S, 10, 0.5, None, kp, None, oracle), "sharded diverse_search")
        ex = top_lists(p.model, S, 5, rs, kp)
        got = p.ix.collapsed_search(q, 10, 2, keep=kd, exclude=dev(ex))
        want = p.model.collapsed_search(S, 10, 2, kp, ex)
        same(got[:2], want[:2], "sharded collapsed_search")
        assert np.array_equal(got[2].cpu().numpy(), want[2]) and bool((got[3] == 1).all())
        pos = np.stack([OFF + np.argmax(S, 1), OFF + rs.randint(0, c.N, size=33), np.full(33, -1)], 1).astype(np.int64)
        got = tt.mine_hard_negatives(p.ix, q, dev(pos), 10, margin=0.05, keep=kd)
        same(got, p.model.mine(S, pos, 10, margin=0.05, keep=kp), "sharded mine_hard_negatives")
        p.consistent(got, q, kd, "sharded mine_hard_negatives")
    got = p.ix.collapsed_search(q[:2], 10, 1, keep=keep)             # tie query 0: the masked rounds, sharded
    want = p.model.collapsed_search(S[:2], 10, 1, mask)
    same(got[:2], want[:2], "sharded collapsed_search through masked rounds")
    assert np.array_equal(got[2].cpu().numpy(), want[2]) and p.ix.collapse_rounds[1] > 0
    p.result(h)                                                     # submitted before all of it: still its own rows


@pytest.mark.parametrize("seed", (1, 2))
@pytest.mark.parametrize("name", NAMES)
def test_random_pipelined_sequences_with_flavour_calls(tt, corpora, name, seed):
    c = corpora(name)
    p = FlavourPipe(tt, c)
    for op in im.with_flavours(im.sequence(seed, 30, c.shapes, SHARD_K), seed, batches(c)):
        print(op)
        getattr(p, op[0])(*op[1:])
    print(f"{p.n_results} results over {len(p.shapes_used)} shapes, flavour calls {dict(p.n_flavours)}")
    assert p.n_results >= im.MIN_RESULTS and all(p.n_flavours[kind] >= 2 for kind in im.PIPE_FLAVOURS)
