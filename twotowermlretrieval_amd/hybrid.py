"""Hybrid rerank stage of the reference's /search handler (frontend/main.py:102-210) with the ChromaDB
HNSW lookup replaced by the exact GPU top-50.

    1. query string -> unit vector (QueryInferencer / the HIP query tower)
    2. exact top-`n_candidates` (50) passages by cosine over the resident embedding matrix
    3. TF-IDF cosine of the query against those candidates (sklearn, CPU: sparse string work, out of the
       GPU path's scope -- the fitted vectorizer is the reference's `tfidf_artifacts.pkl`)
    4. final = alpha * dense + (1 - alpha) * tfidf, sort, top `n_results` (10)

Dense score definition.  The reference stores embeddings in a Chroma collection created WITHOUT
`hnsw:space` (save_to_chromaDB.ipynb), i.e. squared-L2 distances, and uses `1 - dist` as the semantic
score (frontend/main.py:162); for unit vectors that is 2*cos - 1, not the cosine.  `dense_score="cosine"`
(default) uses the cosine itself; `dense_score="chroma_l2"` reproduces the reference's 2*cos - 1 so the
blend weights match its behaviour exactly.  alpha == 0 is the reference's pure keyword search over the
whole corpus (frontend/main.py:119-147) and, by default, never touches the GPU.

Lexical half on the GPU (opt-in, lexical="gpu").  The whole-corpus TF-IDF steps -- the alpha == 0 keyword search, the
lexical_candidates, SimpleHybridRetriever's blend over every document -- are one LexicalIndex.search (lexical.py) instead
of sklearn's cosine_similarity + argsort on the host.  The GPU lexical score is the fp32 dot product of the f32-ROUNDED
TF-IDF rows; sklearn renormalises in float64, so the two agree within (m + 3) * 2^-24 for a query of m terms and are not
bit-identical: near-ties may swap, which is why the default, lexical="sklearn", stays the code it always was.

Rank fusion (opt-in, fusion="rrf", needs lexical="gpu").  Step 4's blend adds a cosine to a TF-IDF score and sees the dense
candidates only.  fusion="rrf" replaces steps 3 and 4 by reciprocal rank fusion (fusion.py) of the dense top-`n_candidates` and
the lexical top-`n_candidates` of the WHOLE corpus: score = alpha / (60 + dense rank) + (1 - alpha) / (60 + lexical rank), ranks
from 1, a list that lacks the document adding 0 -- one launch on the device.  The default, fusion="blend", is the reference's
step 4, untouched.
"""
from __future__ import annotations

from typing import Dict, List, Sequence

import numpy as np
import torch

from .index import BruteForceIndex, score_all
from .lexical import LexicalIndex

# the smallest float32 above 1e-5: `score >= LEXICAL_MIN_SCORE` in fp32 mirrors the reference's `score > 1e-5`
LEXICAL_MIN_SCORE = float(np.nextafter(np.float32(1e-5), np.float32(1.0)))


def _lexical_mode(lexical: str) -> str:
    if lexical not in ("sklearn", "gpu"):
        raise ValueError("lexical must be 'sklearn' or 'gpu'")
    return lexical


class HybridSearcher:
    def __init__(self, inferencer, documents: Sequence[str], doc_embeddings: torch.Tensor = None, tfidf_vectorizer=None,
                 doc_tfidf_matrix=None, n_candidates: int = 50, dense_score: str = "cosine", index: BruteForceIndex = None,
                 lexical_candidates: int = 0, lexical: str = "sklearn", fusion: str = "blend"):
        """documents: documents.pkl's list (row i of the embeddings <-> documents[i]); any object with __len__ and __getitem__
        is used as it is (a corpus too large for a Python list: an mmap-backed or generated sequence), other iterables are
        listed.  index: an existing BruteForceIndex over the embedding matrix instead of doc_embeddings (one is built otherwise).
        lexical_candidates: 0 (the default) blends over the dense top-`n_candidates` only, as the reference does -- the best
        lexical match is lost when it ranks below them by cosine.  n > 0 adds the query's n best TF-IDF matches over the
        whole corpus (similarity > 1e-5) to the candidates; their dense scores come from index.score_ids.
        lexical: "sklearn" (the default) computes the whole-corpus TF-IDF steps on the host as the reference does; "gpu"
        uploads doc_tfidf_matrix once as a LexicalIndex and answers them with one search each (module docstring).
        fusion: "blend" (the default) is the reference's alpha * dense + (1 - alpha) * tfidf over the candidates; "rrf" (needs
        lexical="gpu") ranks the union of the dense and the lexical top-`n_candidates` by reciprocal rank fusion with the
        weights (alpha, 1 - alpha) (module docstring)."""
        if fusion not in ("blend", "rrf"):
            raise ValueError("fusion must be 'blend' or 'rrf'")
        if fusion == "rrf" and lexical != "gpu":
            raise ValueError("fusion='rrf' fuses the two lists on the device: it needs lexical='gpu'")
        self.fusion = fusion
        if dense_score not in ("cosine", "chroma_l2"):
            raise ValueError("dense_score must be 'cosine' or 'chroma_l2'")
        self.lexical = _lexical_mode(lexical)
        if (index is None) == (doc_embeddings is None):
            raise ValueError("HybridSearcher wants doc_embeddings or index (exactly one)")
        self.inferencer = inferencer
        indexable = hasattr(documents, "__getitem__") and hasattr(documents, "__len__") and not isinstance(documents, (str, bytes))
        self.documents = documents if indexable else list(documents)
        # single-query searches stream the fp16 shadow corpus
        self.index = index if index is not None else BruteForceIndex(doc_embeddings, screen=True)
        if len(self.documents) != self.index.ntotal:
            raise ValueError(f"{len(self.documents)} documents for {self.index.ntotal} embedding rows")
        self.n_candidates = int(n_candidates)
        self.dense_score = dense_score
        self.lexical_candidates = int(lexical_candidates)
        if self.lexical_candidates < 0:
            raise ValueError(f"lexical_candidates = {lexical_candidates} < 0")
        if tfidf_vectorizer is None:  # same construction as backend/main.py:142-143
            from sklearn.feature_extraction.text import TfidfVectorizer
            tfidf_vectorizer = TfidfVectorizer(stop_words="english", max_features=20000)
            doc_tfidf_matrix = tfidf_vectorizer.fit_transform(self.documents)
        self.tfidf = tfidf_vectorizer
        self.doc_tfidf = doc_tfidf_matrix
        self.lexical_index = (LexicalIndex(doc_tfidf_matrix, self.index.device, self.index.idx_offset)
                              if self.lexical == "gpu" else None)

    def _lexical_top(self, q_tfidf, n: int):
        """lexical="gpu": the n best TF-IDF matches of the whole corpus with score > 1e-5, not removed from the dense index:
        (row numbers, scores), best first."""
        n = min(n, self.index.ntotal)
        if n <= 0:
            return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.float32)
        vals, idx = self.lexical_index.search(q_tfidf, n, min_score=LEXICAL_MIN_SCORE, keep=self.index.keep_mask)
        vals, idx = vals[0].cpu().numpy(), idx[0].cpu().numpy()
        live = idx >= 0
        return idx[live] - self.index.idx_offset, vals[live]

    def _search_rrf(self, query: str, alpha: float, n_results: int) -> List[Dict]:
        """fusion="rrf": the dense and the lexical top-n_candidates, one fuse launch, the reference's dict per result with the
        fused score as `score`; a component a list lacks reads 0.0."""
        from .fusion import fuse_topk
        n = min(self.n_candidates, self.index.ntotal)
        if n <= 0 or n_results <= 0:
            return []
        q = torch.from_numpy(self.inferencer.get_query_embedding(query)).to(self.index.docs.device)
        dv, di = self.index.search(q, n)
        lv, li = self.lexical_index.search(self.tfidf.transform([query]), n, min_score=LEXICAL_MIN_SCORE, keep=self.index.keep_mask)
        fv, fi, pos = fuse_topk(((dv, di), (lv[0], li[0])), min(int(n_results), 2 * n), method="rrf",
                                weights=(float(alpha), 1.0 - float(alpha)), return_positions=True)
        fv, fi, pos, dv, lv = fv.cpu().numpy(), fi.cpu().numpy(), pos.cpu().numpy(), dv.cpu().numpy(), lv[0].cpu().numpy()
        out = []
        for s, i, (pd, pl) in zip(fv, fi, pos):
            if i < 0:
                break
            cos = float(dv[pd]) if pd >= 0 else 0.0
            row = int(i) - self.index.idx_offset
            out.append({"doc": self.documents[row], "index": row, "score": float(s),
                        "dense_score": cos if self.dense_score == "cosine" or pd < 0 else 2.0 * cos - 1.0,
                        "tfidf_score": float(lv[pl]) if pl >= 0 else 0.0})
        return out

    def search(self, query: str, alpha: float = 0.5, n_results: int = 10) -> List[Dict]:
        from sklearn.metrics.pairwise import cosine_similarity
        if self.fusion == "rrf":
            return self._search_rrf(query, alpha, n_results)
        if alpha == 0.0 and self.lexical == "gpu":
            rows, sims = self._lexical_top(self.tfidf.transform([query]), n_results)
            return [{"doc": self.documents[int(i)], "index": int(i), "score": float(s), "dense_score": 0.0,
                     "tfidf_score": float(s)} for i, s in zip(rows, sims)]
        if alpha == 0.0:
            sims = cosine_similarity(self.tfidf.transform([query]), self.doc_tfidf).flatten()
            order = np.argsort(-sims, kind="stable")[:n_results]
            return [{"doc": self.documents[i], "index": int(i), "score": float(sims[i]), "dense_score": 0.0,
                     "tfidf_score": float(sims[i])} for i in order if sims[i] > 1e-5]
        q = torch.from_numpy(self.inferencer.get_query_embedding(query)).to(self.index.docs.device)
        k = min(self.n_candidates, self.index.ntotal)
        vals, idx = self.index.search(q, k)
        cos = vals.cpu().numpy()
        cand = [int(i) for i in idx.cpu().tolist() if i >= 0]
        q_tfidf = self.tfidf.transform([query])
        if self.lexical_candidates > 0 and q_tfidf.nnz > 0:
            # the best lexical matches of the whole corpus join the dense top-k, with their exact dense scores
            have = set(cand)
            if self.lexical == "gpu":
                extra = [int(i) for i in self._lexical_top(q_tfidf, self.lexical_candidates)[0] if int(i) not in have]
            else:
                sims = cosine_similarity(q_tfidf, self.doc_tfidf).flatten()
                extra = [int(i) for i in np.argsort(-sims, kind="stable")[:self.lexical_candidates] if sims[i] > 1e-5 and int(i) not in have]
            if extra:
                s = self.index.score_ids(q, torch.tensor(extra, dtype=torch.int64, device=q.device)).cpu().numpy()
                live = np.isfinite(s)  # (a removed document scores -inf: it is no candidate)
                cos = np.concatenate([cos[:len(cand)], s[live]])
                cand += [i for i, ok in zip(extra, live) if ok]
        dense = cos[:len(cand)] if self.dense_score == "cosine" else 2.0 * cos[:len(cand)] - 1.0
        if q_tfidf.nnz > 0:
            tf = np.nan_to_num(cosine_similarity(q_tfidf, self.tfidf.transform([self.documents[i] for i in cand]))[0])
        else:
            tf = np.zeros(len(cand))
        final = alpha * dense + (1.0 - alpha) * tf
        order = np.argsort(-final, kind="stable")[:n_results]
        return [{"doc": self.documents[cand[i]], "index": cand[i], "score": float(final[i]),
                 "dense_score": float(dense[i]), "tfidf_score": float(tf[i])} for i in order]


class SimpleHybridRetriever:
    """Drop-in for backend/simple_hybrid.py:13-67 (same constructor, `fit`, `search` and return types): TF-IDF + dense
    scores of EVERY document, combined = alpha * dense + (1 - alpha) * tfidf, descending argsort, top_k (doc, score)
    pairs.  As in the reference the corpus is embedded with the SAME (query) encoder (:37-41) and the vectorizer is
    TfidfVectorizer(stop_words='english', max_features=10000) (:24).  The dense scores come from the HIP path
    (query tower + tt_score_all_f32); the TF-IDF half is sklearn on the CPU, as in the reference.
    RESTRICTION: the dense term is the dot product of the tower outputs, which equals the reference's
    sklearn `cosine_similarity` only for unit rows, i.e. with NORMALIZE_OUTPUT = true (the reference's default and the
    only configuration G11 pins); with NORMALIZE_OUTPUT = false the blend differs from the reference's."""

    def __init__(self, artifacts_path: str, alpha: float = 0.5, device=None, lexical: str = "sklearn"):
        """lexical: "sklearn" (the default) is the reference's host blend over every document; "gpu" keeps the TF-IDF matrix
        on the device as a LexicalIndex and makes the blend and the top_k selection one search over it, with the dense scores
        as its base: no N-sized array goes to the host (hybrid.py's docstring has the numerics)."""
        from sklearn.feature_extraction.text import TfidfVectorizer
        self.lexical = _lexical_mode(lexical)
        self.lexical_index = None
        from .query_inferencer import QueryInferencer
        self.dense_retriever = QueryInferencer(artifacts_path, device=device)
        self.alpha = alpha
        self.tfidf = TfidfVectorizer(stop_words="english", max_features=10000)
        self.documents: List[str] = []
        self.doc_embeddings = None

    def fit(self, documents: Sequence[str]) -> None:
        self.documents = list(documents)
        self.tfidf_matrix = self.tfidf.fit_transform(self.documents)
        # one batched call of the query tower instead of the reference's per-document loop: same rows
        self.doc_embeddings = self.dense_retriever.get_query_embeddings(self.documents)
        if self.lexical == "gpu":
            self.lexical_index = LexicalIndex(self.tfidf_matrix, self.doc_embeddings.device)

    def search(self, query: str, top_k: int = 10):
        if self.lexical == "gpu":
            q = torch.from_numpy(self.dense_retriever.get_query_embedding(query)).to(self.doc_embeddings.device)
            dense = score_all(q.unsqueeze(0), self.doc_embeddings)
            vals, idx = self.lexical_index.search(self.tfidf.transform([query]), min(top_k, max(len(self.documents), 1)),
                                                  base=dense, w_base=self.alpha, w_lex=1 - self.alpha)
            return [(self.documents[i], float(v)) for v, i in zip(vals[0].tolist(), idx[0].tolist()) if i >= 0]
        from sklearn.metrics.pairwise import cosine_similarity
        tfidf_scores = cosine_similarity(self.tfidf.transform([query]), self.tfidf_matrix)[0]
        q = torch.from_numpy(self.dense_retriever.get_query_embedding(query)).to(self.doc_embeddings.device)
        dense_scores = score_all(q, self.doc_embeddings).cpu().numpy().astype(np.float64)
        combined = self.alpha * dense_scores + (1 - self.alpha) * tfidf_scores
        top = np.argsort(combined)[::-1][:top_k]
        return [(self.documents[i], combined[i]) for i in top]
