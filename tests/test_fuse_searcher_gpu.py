"""HybridSearcher(fusion="rrf") against a Python restatement of reciprocal rank fusion over the two lists it fuses, and
fusion="blend" (the default) against the searcher as it always was."""
import numpy as np
import pytest
import torch

import synth

pytestmark = pytest.mark.gpu
pytest.importorskip("sklearn")

from test_hybrid_lexical_gpu import DIM, N_DOCS, VOCAB, StubInferencer, _passages, _queries  # noqa: E402

N_CAND = 20


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
                          n_candidates=N_CAND, **kw)


def _rrf(dense, lexical, alpha, n):
    """Reciprocal rank fusion as a reader would write it: [(index, cosine)] and [(index, tfidf)], best first -> [(index,
    score, cosine or None, tfidf or None)].  Every term is w / (60 + rank) in float64 rounded to float32 once, the two terms
    added in float32, dense first."""
    term = {}
    for l, (lst, w) in enumerate(((dense, alpha), (lexical, 1.0 - alpha))):
        for rank, (i, s) in enumerate(lst, start=1):
            term.setdefault(i, [None, None, None, None])
            term[i][l] = np.float32(w / (60.0 + rank))
            term[i][2 + l] = s
    rows = []
    for i, (td, tl, sd, sl) in term.items():
        acc = np.float32(np.float32(0) + (td if td is not None else np.float32(0)))
        acc = np.float32(acc + (tl if tl is not None else np.float32(0)))
        rows.append((i, acc, sd, sl))
    rows.sort(key=lambda r: (-float(r[1]), r[0]))
    return rows[:n]


@pytest.mark.parametrize("alpha", [0.5, 0.8, 0.0])
def test_rrf_against_a_python_restatement(corpus, alpha):
    from twotowermlretrieval_amd.hybrid import LEXICAL_MIN_SCORE
    words, docs, tfidf, mat, E, u = corpus
    hs = _searcher(corpus, lexical="gpu", fusion="rrf")
    dv, di = hs.index.search(torch.from_numpy(u).cuda(), N_CAND)
    dense = list(zip(di.cpu().tolist(), dv.cpu().tolist()))
    for query in _queries(docs, words):
        lv, li = hs.lexical_index.search(tfidf.transform([query]), N_CAND, min_score=LEXICAL_MIN_SCORE)
        lexical = [(i, s) for i, s in zip(li[0].cpu().tolist(), lv[0].cpu().tolist()) if i >= 0]
        want = _rrf(dense, lexical, alpha, 10)
        got = hs.search(query, alpha=alpha, n_results=10)
        assert len(got) == len(want) == 10
        for r, (i, s, sd, sl) in zip(got, want):
            assert r["index"] == i and r["doc"] == docs[i], query
            assert np.float32(r["score"]) == s and r["score"] == float(s), query
            assert r["dense_score"] == (0.0 if sd is None else sd) and r["tfidf_score"] == (0.0 if sl is None else sl), query
        if lexical and alpha <= 0.5:                                        # (the best lexical match is among the ten)
            assert any(r["tfidf_score"] > 0 for r in got)
    # more results than the two lists hold: the union, then nothing
    everything = hs.search(_queries(docs, words)[1], alpha=0.5, n_results=100)
    assert N_CAND <= len(everything) <= 2 * N_CAND and len({r["index"] for r in everything}) == len(everything)


def test_rrf_reports_the_chroma_dense_score_and_skips_removed_documents(corpus):
    words, docs, tfidf, mat, E, u = corpus
    a, b = _searcher(corpus, lexical="gpu", fusion="rrf"), _searcher(corpus, lexical="gpu", fusion="rrf", dense_score="chroma_l2")
    query = docs[123]
    ra, rb = a.search(query), b.search(query)
    assert [r["index"] for r in ra] == [r["index"] for r in rb] and [r["score"] for r in ra] == [r["score"] for r in rb]
    for x, y in zip(ra, rb):
        assert y["dense_score"] == (2.0 * x["dense_score"] - 1.0 if x["dense_score"] != 0.0 else 0.0)
    assert 123 in [r["index"] for r in ra]
    a.index.remove_ids([123])
    assert 123 not in [r["index"] for r in a.search(query, n_results=40)]


def test_blend_is_the_default_and_unchanged(corpus, monkeypatch):
    """fusion="blend" is the searcher as it was: the same results as a searcher built without the argument, on both lexical
    paths, and the fuse kernel is never called."""
    from twotowermlretrieval_amd import fusion
    words, docs, tfidf, mat, E, u = corpus

    def refuse(*a, **kw):
        raise AssertionError("the blend must not fuse")
    monkeypatch.setattr(fusion, "fuse_topk", refuse)
    for kw in (dict(), dict(lexical="gpu", lexical_candidates=5)):
        old, new = _searcher(corpus, **kw), _searcher(corpus, fusion="blend", **kw)
        assert old.fusion == "blend"
        for query in _queries(docs, words):
            for alpha in (0.0, 0.5, 1.0):
                assert old.search(query, alpha=alpha) == new.search(query, alpha=alpha), (query, alpha)
