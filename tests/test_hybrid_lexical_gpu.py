"""HybridSearcher(lexical="gpu") and SimpleHybridRetriever(lexical="gpu") against the default (sklearn) path, on a corpus of a
few hundred synthetic passages generated here.

The GPU lexical score is the fp32 chain over the f32-rounded TF-IDF rows, sklearn's the float64 cosine: for a query of m terms
they differ by at most E = (m + 3) * 2^-24 (tests/test_lexical_cpu.py).  Criterion, for every case: every returned document's
score is within E of the default path's score of THAT document, and no document outside the returned list has a default-path
score above the last returned score by more than 2 E.  For the blends E is scaled by (1 - alpha), plus 3 * 2^-24 for the f32
blend."""
import numpy as np
import pytest
import torch

import synth

pytestmark = pytest.mark.gpu
pytest.importorskip("sklearn")

N_DOCS, DIM, VOCAB = 400, 64, 160
U = 2.0 ** -24


class StubInferencer:
    def __init__(self, vec):
        self.vec = vec

    def get_query_embedding(self, query):
        return self.vec


def _passages(seed, n, words, lo=5, hi=30):
    rng = np.random.default_rng(seed)
    p = 1.0 / np.arange(1, len(words) + 1)
    p /= p.sum()
    docs, seen = [], set()
    while len(docs) < n:
        d = " ".join(words[t] for t in rng.choice(len(words), size=int(rng.integers(lo, hi)), p=p))
        if d not in seen:
            seen.add(d)
            docs.append(d)
    return docs


def _queries(docs, words):
    return [" ".join(docs[7].split()[:6]), docs[123], f"{words[3]} {words[40]} {words[90]}", words[0],
            f"{words[150]} {words[151]} {words[5]} {words[5]}", "zzzunknown qqqunknown"]


@pytest.fixture(scope="module")
def corpus():
    from sklearn.feature_extraction.text import TfidfVectorizer
    words = [f"w{i}x" for i in range(VOCAB)]
    docs = _passages(3, N_DOCS, words)
    tfidf = TfidfVectorizer(stop_words="english", max_features=20000)
    mat = tfidf.fit_transform(docs)
    return words, docs, tfidf, mat, synth.unit_rows(41, N_DOCS, DIM).copy(), synth.unit_rows(42, 1, DIM)[0].copy()


def _searcher(corpus, **kw):
    from twotowermlretrieval_amd.hybrid import HybridSearcher
    words, docs, tfidf, mat, E, u = corpus
    return HybridSearcher(StubInferencer(u), docs, torch.from_numpy(E).cuda(), tfidf_vectorizer=tfidf, doc_tfidf_matrix=mat,
                          n_candidates=20, **kw)


def _check(returned, default_score, E, what):
    """returned: [(index, score)] best first; default_score: {index: the default path's score of that document}."""
    assert returned, what
    for i, s in returned:
        assert i in default_score, (what, i)
        assert abs(s - default_score[i]) <= E, (what, i, s, default_score[i], E)
    last = min(s for _, s in returned)
    inside = {i for i, _ in returned}
    for i, s in default_score.items():
        if i not in inside:
            assert s <= last + 2 * E, (what, i, s, last, E)


def test_keyword_search_alpha_0(corpus):
    from sklearn.metrics.pairwise import cosine_similarity
    from twotowermlretrieval_amd.lexical import LexicalIndex
    words, docs, tfidf, mat, _, _ = corpus
    hs, hs0 = _searcher(corpus, lexical="gpu"), _searcher(corpus)
    assert hs0.lexical == "sklearn" and hs0.lexical_index is None and isinstance(hs.lexical_index, LexicalIndex)
    assert hs.lexical_index.ntotal == N_DOCS and hs.lexical_index.n_features == mat.shape[1]
    for query in _queries(docs, words):
        q = tfidf.transform([query])
        got = hs.search(query, alpha=0.0, n_results=10)
        want = hs0.search(query, alpha=0.0, n_results=10)
        if q.nnz == 0:
            assert got == [] and want == []
            continue
        E = (q.nnz + 3) * U
        sims = cosine_similarity(q, mat).flatten()                              # the default path's score of every document
        # (documents at or below the reference's 1e-5 cut are no matches: nothing in this corpus scores within E of it)
        assert not ((sims > 1e-5 - 2 * E) & (sims <= 1e-5 + 2 * E)).any()
        _check([(r["index"], r["score"]) for r in got], {i: float(s) for i, s in enumerate(sims) if s > 1e-5}, E, query)
        assert len(got) == len(want)
        for r in got:
            assert r["doc"] == docs[r["index"]] and r["dense_score"] == 0.0 and r["tfidf_score"] == r["score"]
        scores = [r["score"] for r in got]
        assert scores == sorted(scores, reverse=True)


def test_removed_documents_do_not_come_back_through_the_lexical_side(corpus):
    words, docs, tfidf, mat, _, _ = corpus
    hs = _searcher(corpus, lexical="gpu")
    query = docs[123]
    first = hs.search(query, alpha=0.0, n_results=5)
    assert first[0]["index"] == 123
    hs.index.remove_ids([123, first[1]["index"]])
    again = [r["index"] for r in hs.search(query, alpha=0.0, n_results=5)]
    assert 123 not in again and first[1]["index"] not in again and again[0] == first[2]["index"]
    assert 123 not in [r["index"] for r in hs.search(query, alpha=0.5, n_results=10)]


def test_lexical_candidates_blend(corpus):
    words, docs, tfidf, mat, _, _ = corpus
    alpha = 0.5
    hs, hs0 = _searcher(corpus, lexical="gpu", lexical_candidates=5), _searcher(corpus, lexical_candidates=5)
    for query in _queries(docs, words):
        m = tfidf.transform([query]).nnz
        E = (1 - alpha) * (m + 3) * U + 3 * U
        got = hs.search(query, alpha=alpha, n_results=10)
        everything = hs0.search(query, alpha=alpha, n_results=N_DOCS)           # the default path's score of every candidate
        assert len(got) == 10 and 20 <= len(everything) <= 25
        _check([(r["index"], r["score"]) for r in got], {r["index"]: r["score"] for r in everything}, E, query)


@pytest.mark.parametrize("alpha", [0.3, 1.0])
def test_simple_hybrid_retriever(tmp_path, golden, alpha):
    from test_inferencer_gpu import _artifacts
    from twotowermlretrieval_amd.hybrid import SimpleHybridRetriever
    g = golden("g11_hybrid.npz")
    art = str(_artifacts(tmp_path, g))
    # the few words the synthetic tower knows (the rest embed as <unk>), most frequent first, then filler words
    words = ["w5", "w6", "w7", "machine", "learning", "mail"] + [f"w{i}x" for i in range(VOCAB - 6)]
    docs = _passages(5, 300, words)
    r, r0 = SimpleHybridRetriever(art, alpha=alpha, lexical="gpu"), SimpleHybridRetriever(art, alpha=alpha)
    r.fit(docs)
    r0.fit(docs)
    assert r0.lexical_index is None and r.lexical_index.ntotal == len(docs)
    row = {d: i for i, d in enumerate(docs)}
    queries = [" ".join(docs[7].split()[:6]), docs[50], f"{words[3]} {words[40]} {words[90]}", "zzzunknown " + words[1]]
    for query in queries:
        m = r.tfidf.transform([query]).nnz
        E = (1 - alpha) * (m + 3) * U + 3 * U
        got = r.search(query, top_k=10)
        default = {row[d]: float(s) for d, s in r0.search(query, top_k=len(docs))}   # every document's default-path score
        assert len(got) == 10 and len(default) == len(docs) and all(isinstance(d, str) for d, _ in got)
        _check([(row[d], s) for d, s in got], default, E, (alpha, query))
        assert [s for _, s in got] == sorted((s for _, s in got), reverse=True)
