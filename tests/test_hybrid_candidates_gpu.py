"""HybridSearcher(lexical_candidates=n): the best lexical matches of the whole corpus join the dense top-`n_candidates`, with
their exact dense scores from index.score_ids.  A stub inferencer returns a fixed unit vector; one document of a 300-document
synthetic corpus is the best lexical match of the query but lies outside the dense top-`n_candidates`: the default
(lexical_candidates=0, today's code) can never return it, lexical_candidates=20 does."""
import numpy as np
import pytest
import torch

import synth

pytestmark = pytest.mark.gpu

N_DOCS, DIM, PLANTED, N_CAND = 300, 64, 123, 10
QUERY = "zebra quokka xylophone"
PARTIAL = (5, 17, 40, 250)    # documents that share one word with the query


class StubInferencer:
    def __init__(self, vec):
        self.vec = vec

    def get_query_embedding(self, query):
        return self.vec


def _corpus():
    docs = [f"alpha{i % 7} beta{i % 11} gamma{i % 13} common filler text" for i in range(N_DOCS)]
    for i in PARTIAL:
        docs[i] += " zebra"
    docs[PLANTED] = QUERY
    E = synth.unit_rows(31, N_DOCS, DIM).copy()
    u = synth.unit_rows(32, 1, DIM)[0].copy()
    r = E[PLANTED] - np.dot(E[PLANTED], u) * u          # orthogonal to the query: far below the dense top-10 (cos ~ 0.3)
    E[PLANTED] = (r / np.linalg.norm(r)).astype(np.float32)
    return docs, E, u


def _searcher(docs, E, u, **kw):
    from sklearn.feature_extraction.text import TfidfVectorizer
    from twotowermlretrieval_amd.hybrid import HybridSearcher
    tfidf = TfidfVectorizer(stop_words="english", max_features=20000)
    mat = tfidf.fit_transform(docs)
    return HybridSearcher(StubInferencer(u), docs, torch.from_numpy(E).cuda(), tfidf_vectorizer=tfidf, doc_tfidf_matrix=mat,
                          n_candidates=N_CAND, **kw)


def _blend(hs, cand, cos, alpha, n_results):
    """hybrid.py's own expressions over a candidate list and its cosines."""
    from sklearn.metrics.pairwise import cosine_similarity
    dense = cos if hs.dense_score == "cosine" else 2.0 * cos - 1.0
    tf = np.nan_to_num(cosine_similarity(hs.tfidf.transform([QUERY]), hs.tfidf.transform([hs.documents[i] for i in cand]))[0])
    final = alpha * dense + (1.0 - alpha) * tf
    order = np.argsort(-final, kind="stable")[:n_results]
    return [{"doc": hs.documents[cand[i]], "index": cand[i], "score": float(final[i]), "dense_score": float(dense[i]),
             "tfidf_score": float(tf[i])} for i in order]


@pytest.mark.parametrize("dense_score", ["cosine", "chroma_l2"])
def test_lexical_candidates_reach_the_blend(oracle, dense_score):
    from sklearn.metrics.pairwise import cosine_similarity
    docs, E, u = _corpus()
    S = oracle.score_all(u[None, :], E)[0]              # the chain's score of every document
    top = np.lexsort((np.arange(N_DOCS), -S))[:N_CAND]
    assert PLANTED not in top and not set(PARTIAL) <= set(top.tolist())
    alpha = 0.5

    hs0 = _searcher(docs, E, u, dense_score=dense_score)                     # lexical_candidates = 0: today's search
    assert hs0.lexical_candidates == 0
    want0 = _blend(hs0, [int(i) for i in top], S[top], alpha, 10)
    got0 = hs0.search(QUERY, alpha=alpha, n_results=10)
    assert got0 == want0
    assert PLANTED not in [r["index"] for r in got0]                         # the hole: the best lexical match is lost

    hs = _searcher(docs, E, u, dense_score=dense_score, lexical_candidates=20)
    sims = cosine_similarity(hs.tfidf.transform([QUERY]), hs.doc_tfidf).flatten()
    assert int(np.argmax(sims)) == PLANTED
    lex = [int(i) for i in np.argsort(-sims, kind="stable")[:20] if sims[i] > 1e-5]
    assert set(lex) == {PLANTED, *PARTIAL}                                   # fewer than 20 documents match at all
    extra = [i for i in lex if i not in set(top.tolist())]
    cand = [int(i) for i in top] + extra
    want = _blend(hs, cand, np.concatenate([S[top], S[extra]]), alpha, 10)
    got = hs.search(QUERY, alpha=alpha, n_results=10)
    assert got == want
    hit = [r for r in got if r["index"] == PLANTED]
    assert len(hit) == 1 and got[0]["index"] == PLANTED                      # returned, and on top of the blend
    cos = S[PLANTED]
    assert hit[0]["dense_score"] == float(cos if dense_score == "cosine" else np.float32(2.0) * cos - np.float32(1.0))
    # (`got == want` above is the blend, expression for expression; in float64 it agrees to the fp32 rounding of alpha * dense)
    assert hit[0]["score"] == pytest.approx(alpha * hit[0]["dense_score"] + (1.0 - alpha) * hit[0]["tfidf_score"], abs=2e-7)
    assert hit[0]["tfidf_score"] == pytest.approx(1.0, abs=1e-9)             # the document IS the query
    # alpha = 0 is the pure keyword search either way
    assert hs.search(QUERY, alpha=0.0, n_results=5) == hs0.search(QUERY, alpha=0.0, n_results=5)
    # a removed document scores -inf and is no candidate
    hs.index.remove_ids([PLANTED])
    assert PLANTED not in [r["index"] for r in hs.search(QUERY, alpha=alpha, n_results=10)]
