"""Lexical search on the device: sparse TF-IDF rows times a sparse query with an exact top-k (csrc/lexical.hip).

Replaces the whole-corpus lexical step of the reference's hybrid search

    cosine_similarity(query_tfidf, doc_tfidf_matrix) ; argsort ; score > 1e-5     (frontend/main.py:119-147)
    alpha * dense + (1 - alpha) * tfidf over every document ; argsort             (backend/simple_hybrid.py:44-60)

with one pass over a CSR matrix resident in HBM; no [B,N] array is formed and nothing N-sized goes to the host.

Score.  s(b,n) = the fp32 dot product of row n with the query over the row's stored entries in ascending column order, every
product rounded to fp32 and added in fp32 (include/tt.h, "Lexical search").  For TfidfVectorizer's unit-norm rows that is the
cosine of the f32-ROUNDED rows: sklearn's cosine_similarity renormalises in float64, so the two agree within
(m + 3) * 2^-24 for a query of m terms (tests/test_lexical_cpu.py) and are not bit-identical -- which is why the hybrid
classes use this path only on request (lexical="gpu").

Everything runs through libtt.so; there is no CPU fallback: corpus and query tensors must be on the GPU (a scipy matrix is
validated and converted on the host once, then uploaded).
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib
from .index import _and_keep, _check_keep, _clear_ids, _min_score, _need_cuda, _out_pair, _stream

__all__ = ["LexicalIndex", "lexical_score_topk", "lexical_score_all", "csr_arrays", "validate_csr"]

TT_LEXICAL_FMAX = 20480  # include/tt.h


def csr_arrays(matrix) -> Tuple[np.ndarray, np.ndarray, np.ndarray, int]:
    """A scipy sparse matrix (CSR, CSC, ...) as the arrays the kernels read: (indptr int64 [N+1], cols int32 [nnz], vals f32
    [nnz], n_features), made from a COPY with sorted column indices and duplicates summed.  The has_sorted_indices flag is not
    trusted (TfidfVectorizer.fit_transform hands out unsorted rows), and indptr is widened: scipy uses int32 below 2^31
    entries."""
    import scipy.sparse as sp
    if not sp.issparse(matrix):
        raise TypeError(f"expected a scipy sparse matrix, got {type(matrix).__name__}")
    m = sp.csr_matrix(matrix, copy=True)
    m.has_sorted_indices = False  # (sort_indices() would return at once on a stale flag)
    m.sum_duplicates()            # sorts the indices, then merges equal columns
    m.sort_indices()
    return (np.ascontiguousarray(m.indptr, dtype=np.int64), np.ascontiguousarray(m.indices, dtype=np.int32),
            np.ascontiguousarray(m.data, dtype=np.float32), int(m.shape[1]))


def validate_csr(indptr: np.ndarray, cols: np.ndarray, n_features: int, what: str, sorted_rows: bool) -> None:
    """Host-side check, once per matrix: indptr starts at 0, never decreases and ends at nnz; 0 <= col < n_features;
    with sorted_rows, columns strictly ascending inside a row."""
    if indptr.ndim != 1 or indptr.size < 1 or cols.ndim != 1:
        raise ValueError(f"{what}: indptr must be [N+1] and cols [nnz]")
    if int(indptr[0]) != 0:
        raise ValueError(f"{what}: indptr[0] = {int(indptr[0])}, expected 0")
    if indptr.size > 1 and bool((np.diff(indptr) < 0).any()):
        raise ValueError(f"{what}: indptr decreases")
    if int(indptr[-1]) != cols.size:
        raise ValueError(f"{what}: indptr[-1] = {int(indptr[-1])} but {cols.size} entries are stored")
    if cols.size and (int(cols.min()) < 0 or int(cols.max()) >= n_features):
        raise ValueError(f"{what}: column outside [0, {n_features})")
    if sorted_rows and cols.size > 1:
        starts = np.zeros(cols.size, dtype=bool)
        starts[indptr[:-1][indptr[:-1] < cols.size]] = True
        if bool(((np.diff(cols) <= 0) & ~starts[1:]).any()):
            raise ValueError(f"{what}: columns must be strictly ascending within a row")


def _csr_tensors(t, what: str):
    """(indptr int64, cols int32, vals f32) device tensors as the C calls read them, contiguous."""
    if len(t) != 3 or not all(isinstance(x, torch.Tensor) for x in t):
        raise TypeError(f"{what} must be (indptr, cols, vals) tensors")
    indptr, cols, vals = t
    _need_cuda(indptr, cols, vals)
    if indptr.dtype != torch.int64 or cols.dtype != torch.int32 or vals.dtype != torch.float32:
        raise TypeError(f"{what}: want indptr int64, cols int32, vals float32, got {indptr.dtype}, {cols.dtype}, {vals.dtype}")
    if indptr.dim() != 1 or indptr.numel() < 1 or cols.dim() != 1 or vals.shape != cols.shape:
        raise ValueError(f"{what}: want indptr [rows+1], cols [nnz], vals [nnz]")
    if not (indptr.device == cols.device == vals.device):
        raise ValueError(f"{what}: tensors on different devices")
    return indptr.contiguous(), cols.contiguous(), vals.contiguous()


def check_query_columns(q, n_features: int) -> None:
    """ValueError if a (q_indptr, q_cols, q_vals) device triple holds a column outside [0, n_features).  It reads the
    columns' extremes on the host: a SYNCHRONISATION with the stream that produced them, which is why no search makes this
    check by itself (the kernels drop such a column).  For callers who build their own device queries and want to know."""
    _, qc, _ = _csr_tensors(q, "q")
    if qc.numel():
        lo, hi = int(qc.min()), int(qc.max())
        if lo < 0 or hi >= n_features:
            raise ValueError(f"q: column outside [0, {n_features})")


def _query_tensors(q, n_features: int, device):
    """The queries of a search as device CSR: a scipy sparse [B, n_features] matrix (converted like the corpus: duplicates
    summed, a wrong width refused), or a (q_indptr, q_cols, q_vals) device triple, taken as it is: its dtypes, shapes and
    device are checked, its contents are not read -- a search stays asynchronous to the host, and the kernel drops a column
    outside [0, n_features) (check_query_columns looks, at the price of a synchronisation)."""
    if isinstance(q, (tuple, list)):
        qi, qc, qv = _csr_tensors(q, "q")
        if qi.device != device:
            raise ValueError(f"queries on {qi.device} but the index lives on {device}")
        return qi, qc, qv
    indptr, cols, vals, f = csr_arrays(q)
    if f != n_features:
        raise ValueError(f"q has {f} columns, the index {n_features}")
    return tuple(torch.from_numpy(a).to(device) for a in (indptr, cols, vals))


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None or t.numel() == 0 else t.data_ptr()


def lexical_score_topk(corpus, n_features: int, q, k: int, idx_offset: int = 0, keep: Optional[torch.Tensor] = None,
                       min_score=None, base: Optional[torch.Tensor] = None, w_base: float = 0.0, w_lex: float = 1.0,
                       out=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """The exact top-k of sparse rows times sparse queries, fused (tt_lexical_score_topk_f32).
    corpus = (indptr int64 [N+1], cols int32, vals f32) device tensors, columns ascending within a row; cols and vals are the
    BASES of the matrix: a slice of the rows is (indptr[r0:r1 + 1], cols, vals) with idx_offset = r0, nothing copied.
    q = (q_indptr int64 [B+1], q_cols int32, q_vals f32) device tensors, columns distinct within a query.
    keep: packed keep-bitmask over the N rows (pack_keep_mask).  min_score: a float or a float32 [B] device tensor; only
    documents whose value is >= it are returned.  base: float32 [B, >= N] device tensor (a row stride is fine): the ranked
    value becomes fl32(fl32(w_base * base[b][n]) + fl32(w_lex * s)).  Returns (vals f32 [B,k], idx int64 [B,k]), (value desc,
    index asc), tail (-inf, -1)."""
    indptr, cols, vals = _csr_tensors(corpus, "corpus")
    qi, qc, qv = _csr_tensors(q, "q")
    dev = indptr.device
    if qi.device != dev:
        raise ValueError(f"queries on {qi.device} but the corpus lives on {dev}")
    N, B = indptr.numel() - 1, qi.numel() - 1
    if keep is not None:
        keep = _check_keep(keep, N, dev)
    thr = None if min_score is None else _min_score(min_score, B, dev)
    stride = 0
    if base is not None:
        _need_cuda(base)
        if base.dtype != torch.float32 or base.dim() != 2 or base.shape[0] != B or base.shape[1] < N or base.device != dev:
            raise ValueError(f"base must be float32 [{B}, >= {N}] on {dev}, got {base.dtype} {tuple(base.shape)} on {base.device}")
        if base.stride(1) != 1 and base.shape[1] > 1:
            base = base.contiguous()
        stride = base.stride(0) if B > 1 else max(base.shape[1], N)
    ov, oi = _out_pair(B, k, dev, out)
    with torch.cuda.device(dev):
        L = _lib.lib()
        need = L.tt_lexical_workspace_bytes(B, N, k)
        ws = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
        _lib.check(L.tt_lexical_score_topk_f32(indptr.data_ptr(), _ptr(cols), _ptr(vals), N, int(n_features), qi.data_ptr(),
                                               _ptr(qc), _ptr(qv), B, _ptr(keep), _ptr(thr), _ptr(base), stride, float(w_base),
                                               float(w_lex), int(k), int(idx_offset), ov.data_ptr(), oi.data_ptr(),
                                               ws.data_ptr(), ws.numel(), _stream(indptr)))
    return ov, oi


def lexical_score_all(corpus, n_features: int, q) -> torch.Tensor:
    """Every lexical score as a [B,N] float32 matrix (tt_lexical_score_all_f32): the same chain lexical_score_topk ranks by.
    Materialises B*N floats: for tests and small corpora."""
    indptr, cols, vals = _csr_tensors(corpus, "corpus")
    qi, qc, qv = _csr_tensors(q, "q")
    if qi.device != indptr.device:
        raise ValueError(f"queries on {qi.device} but the corpus lives on {indptr.device}")
    N, B = indptr.numel() - 1, qi.numel() - 1
    out = torch.empty((B, N), dtype=torch.float32, device=indptr.device)
    with torch.cuda.device(indptr.device):
        _lib.check(_lib.lib().tt_lexical_score_all_f32(indptr.data_ptr(), _ptr(cols), _ptr(vals), N, int(n_features),
                                                       qi.data_ptr(), _ptr(qc), _ptr(qv), B, _ptr(out), _stream(indptr)))
    return out


class LexicalIndex:
    """A sparse document-term matrix (TF-IDF, BM25 weights: any CSR) resident in HBM with exact top-k search.

    matrix: a scipy sparse matrix [N, F] -- doc_tfidf_matrix of tfidf_artifacts.pkl as it is; CSR, CSC or any other format
    -- or (indptr, cols, vals, n_features) with device tensors.  A scipy matrix is copied, its indices sorted and duplicates
    summed (csr_arrays); either form is validated on the host once: indptr monotone from 0, 0 <= col < F, columns ascending
    within a row.  Stored as float32 values, int32 columns, int64 indptr (8 bytes per entry + 8 per row).  F <= 20480.
    Row i is document idx_offset + i in what search() returns.  remove_ids / keep_mask / search(keep=) work as on
    BruteForceIndex, with the same packed words (pack_keep_mask).

    Callers, streams and threads: searches of one index may be in flight on any number of streams and host threads at once
    (workspace and outputs are per call; nothing is ordered against another call).  With a device CSR query a search is
    asynchronous to the host: the triple's contents are not read (check_query_columns does, and synchronises); a scipy
    query is converted on the host and copied.  remove_ids is the one mutating caller's."""

    def __init__(self, matrix, device=None, idx_offset: int = 0):
        from_tensors = isinstance(matrix, (tuple, list))
        if from_tensors:
            if len(matrix) != 4:
                raise TypeError("LexicalIndex wants a scipy sparse matrix or (indptr, cols, vals, n_features)")
            indptr, cols, vals = _csr_tensors(matrix[:3], "matrix")
            n_features = int(matrix[3])
            if device is not None and torch.device(device).type != indptr.device.type:
                raise ValueError(f"matrix on {indptr.device} but device = {device}")
            h_indptr, h_cols = indptr.cpu().numpy(), cols.cpu().numpy()
        else:
            h_indptr, h_cols, h_vals, n_features = csr_arrays(matrix)
        if not 1 <= n_features <= TT_LEXICAL_FMAX:
            raise ValueError(f"n_features = {n_features}: the kernels hold the query's dense image in LDS, 1 <= F <= {TT_LEXICAL_FMAX}")
        validate_csr(h_indptr, h_cols, n_features, "LexicalIndex", from_tensors)  # (csr_arrays has just sorted its rows)
        if h_indptr.size - 1 >= 2 ** 31 - 64:
            raise ValueError("LexicalIndex holds fewer than 2^31 - 64 rows (shard larger corpora; idx_offset makes ids global)")
        if not from_tensors:
            dev = torch.device("cuda" if device is None else device)
            if dev.type != "cuda":
                _need_cuda(torch.empty(0, device=dev))
            indptr, cols, vals = (torch.from_numpy(a).to(dev) for a in (h_indptr, h_cols, h_vals))
        self.indptr, self.cols, self.vals = indptr, cols, vals
        self._n_features = n_features
        self.idx_offset = int(idx_offset)
        self._keep: Optional[torch.Tensor] = None

    @property
    def ntotal(self) -> int:
        return self.indptr.numel() - 1

    @property
    def n_features(self) -> int:
        return self._n_features

    @property
    def device(self) -> torch.device:
        return self.indptr.device

    @property
    def keep_mask(self) -> Optional[torch.Tensor]:
        """The persistent keep-bitmask (int32 [ceil(N/32)], bit n = document n not removed), or None: nothing removed yet."""
        return self._keep

    def remove_ids(self, ids) -> None:
        """Withdraw documents: GLOBAL ids (with idx_offset); ids that are not this index's are ignored."""
        self._keep = _clear_ids(self._keep, self.ntotal, self.device, ids, self.idx_offset)

    def search(self, q, k: int = 10, min_score=None, keep: Optional[torch.Tensor] = None, base: Optional[torch.Tensor] = None,
               w_base: float = 0.0, w_lex: float = 1.0, out=None) -> Tuple[torch.Tensor, torch.Tensor]:
        """(vals f32 [B,k], idx int64 [B,k]) like every other search: the k best documents by lexical score, or, with
        `base` (float32 [B, >= N], e.g. score_all's dense scores), by fl32(fl32(w_base * base) + fl32(w_lex * score)).
        q: a scipy sparse [B,F] matrix, or a (q_indptr, q_cols, q_vals) device CSR triple.  min_score: a float or a float32
        [B] device tensor: only documents whose ranked value is >= it are returned.  keep: a packed keep-bitmask for this call,
        ANDed with remove_ids' persistent one.  One pass over the matrix per query (B passes for a batch)."""
        qt = _query_tensors(q, self._n_features, self.device)
        keep = _and_keep(self._keep, keep, self.ntotal, self.device)
        return lexical_score_topk((self.indptr, self.cols, self.vals), self._n_features, qt, k, self.idx_offset, keep,
                                  min_score, base, w_base, w_lex, out)

    def score_all(self, q) -> torch.Tensor:
        """float32 [B,N]: the lexical score of every document (removed ones included), the values search() ranks by."""
        return lexical_score_all((self.indptr, self.cols, self.vals), self._n_features,
                                 _query_tensors(q, self._n_features, self.device))
