"""Rank fusion on the device: the best k ids of the union of several ranked lists (csrc/fuse.hip).

Replaces the last step of the reference's hybrid search

    final = alpha * dense + (1 - alpha) * tfidf ; sort ; top n                    (frontend/main.py:102-210, hybrid.py step 4)

where the two scales are not comparable, where a document is in one list only, or where there are more than two lists:
reciprocal rank fusion (RRF), Borda counts, any rank weighting, and weighted score sums.  The lists are the sorted (vals, idx)
rows every search here returns; they stay on the device, and the fusion is one launch.

The rule (include/tt.h, "Fused lists").  In every list the first occurrence of an id counts.  The fused score of an id is
acc = +0.0f, then for the lists in order acc = fl32(acc + t_l), with t_l = table[l][column] (method="rrf": the table is
w_l / (c + column + 1), formed in float64 and rounded once) or fl32(weight[l] * value) (method="score") where the id is
present, and missing[l] where it is not.  The result is sorted by (fused desc, id asc), tail (-inf, -1).  The kernel divides
nothing, so the result is bit-defined by the table.

Everything runs through libtt.so; there is no CPU fallback.
"""
from __future__ import annotations

import math
from functools import lru_cache
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from .index import _need_cuda, _stream

__all__ = ["rrf_weights", "fuse_topk", "fused_search", "HybridIndex", "FUSE_LMAX", "FUSE_EMAX"]

FUSE_LMAX = 8      # lists per row
FUSE_EMAX = 1024   # entries per row, L * M: TT_TOPK_LARGE_KMAX


def _host_weights(weights, L: int, what: str = "weights") -> Tuple[float, ...]:
    """L finite floats: `weights` as given, or ones."""
    if weights is None:
        return (1.0,) * L
    w = tuple(float(x) for x in weights)
    if len(w) != L:
        raise ValueError(f"{what}: {len(w)} values for {L} lists")
    if not all(math.isfinite(x) for x in w):
        raise ValueError(f"{what} must be finite, got {w}")
    return w


def rrf_weights(L: int, M: int, c: float = 60.0, weights=None) -> torch.Tensor:
    """The reciprocal-rank table of tt_topk_fuse_rank_f32: float32 [L,M] on the host, entry (l, m) = weights[l] / (c + m + 1)
    computed in float64 and rounded once (weights default to 1; c >= 0, Cormack et al.'s 60 by default)."""
    L, M, c = int(L), int(M), float(c)
    if L < 1 or M < 1:
        raise ValueError(f"rrf_weights: L = {L}, M = {M} (need L >= 1, M >= 1)")
    if not math.isfinite(c) or c < 0.0:
        raise ValueError(f"rrf_weights: c = {c} (need a finite c >= 0)")
    w = np.asarray(_host_weights(weights, L), dtype=np.float64)
    table = w[:, None] / (c + np.arange(1, M + 1, dtype=np.float64))[None, :]
    return torch.from_numpy(table.astype(np.float32))


@lru_cache(maxsize=64)
def _rrf_table(L: int, M: int, c: float, weights: Tuple[float, ...], device: torch.device) -> torch.Tensor:
    return rrf_weights(L, M, c, weights).to(device)


@lru_cache(maxsize=64)
def _vector(values: Tuple[float, ...], device: torch.device) -> torch.Tensor:
    return torch.tensor(values, dtype=torch.float32, device=device)


def _device_f32(t: torch.Tensor, shape: Tuple[int, ...], device, what: str) -> torch.Tensor:
    """A caller's device tensor for weights / missing: taken as it is (a captured graph sees rewritten values), so only its
    dtype, shape and device are checked -- its contents are the caller's to keep finite."""
    if t.dtype != torch.float32 or tuple(t.shape) != shape or t.device != device:
        raise ValueError(f"{what} as a tensor must be float32 {list(shape)} on {device}, got {t.dtype} {list(t.shape)} on {t.device}")
    return t if t.is_contiguous() else t.contiguous()


def _check_shape(B: int, L: int, M: int, k: int) -> None:
    if L < 1 or M < 1:
        raise ValueError(f"fuse_topk: L = {L} lists of M = {M} entries (need L >= 1, M >= 1)")
    if L > FUSE_LMAX:
        raise ValueError(f"fuse_topk fuses at most {FUSE_LMAX} lists, got L = {L}")
    if L * M > FUSE_EMAX:
        raise ValueError(f"fuse_topk holds L * M <= {FUSE_EMAX} entries per query, got {L} * {M} = {L * M}")
    if not 1 <= k <= L * M:
        raise ValueError(f"fuse_topk: k = {k} (need 1 <= k <= L * M = {L * M})")


def _minmax(vals: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    """normalize="minmax": every list's valid values (idx >= 0) mapped to [0,1] per query, a constant list to 1; padding stays
    -inf.  torch element-wise ops in front of the launch -- outside the kernel and its bit-level contract."""
    valid = idx >= 0
    lo = torch.where(valid, vals, torch.full_like(vals, math.inf)).amin(-1, keepdim=True)
    hi = torch.where(valid, vals, torch.full_like(vals, -math.inf)).amax(-1, keepdim=True)
    span = hi - lo
    unit = torch.where(span > 0, (vals - lo) / span, torch.ones_like(vals))
    return torch.where(valid, unit, torch.full_like(vals, -math.inf))


def _fuse_packed(vals: Optional[torch.Tensor], idx: torch.Tensor, k: int, method: str, c: float, weights, missing,
                 normalize: Optional[str], return_positions: bool, out):
    """fuse_topk over lists that already lie as one [B,L,M] pair (vals may be None for method="rrf")."""
    if method not in ("rrf", "score"):
        raise ValueError(f"method must be 'rrf' or 'score', got {method!r}")
    if normalize not in (None, "minmax"):
        raise ValueError(f"normalize must be None or 'minmax', got {normalize!r}")
    if normalize is not None and method != "score":
        raise ValueError("normalize= maps scores: it needs method='score' (ranks have no scale to normalise)")
    if not isinstance(idx, torch.Tensor) or idx.dtype != torch.int64 or idx.dim() != 3:
        raise ValueError("fuse_topk wants idx int64 [B,L,M]")
    B, L, M = idx.shape
    k = int(k)
    _check_shape(B, L, M, k)
    dev = idx.device
    score = method == "score"
    if score:
        if not isinstance(vals, torch.Tensor) or vals.dtype != torch.float32 or vals.shape != idx.shape or vals.device != dev:
            raise ValueError("method='score' wants vals f32 with idx's shape on idx's device")
        table = (_device_f32(weights, (L,), dev, "weights") if isinstance(weights, torch.Tensor)
                 else _host_weights(weights, L))
    elif isinstance(weights, torch.Tensor):
        table = _device_f32(weights, (L, M), dev, "weights (method='rrf': the [L,M] table itself)")
    else:
        if not math.isfinite(float(c)) or float(c) < 0.0:
            raise ValueError(f"fuse_topk: c = {c} (need a finite c >= 0)")
        table = _host_weights(weights, L)
    miss = (_device_f32(missing, (L,), dev, "missing") if isinstance(missing, torch.Tensor)
            else _host_weights((0.0,) * L if missing is None else missing, L, "missing"))
    _need_cuda(idx)
    if isinstance(table, tuple):
        table = _vector(table, dev) if score else _rrf_table(L, M, float(c), table, dev)
    if isinstance(miss, tuple):
        miss = _vector(miss, dev)
    idx = idx.contiguous()
    if score:
        vals = vals.contiguous()
        if normalize == "minmax":
            vals = _minmax(vals, idx)
    n_out = 3 if return_positions else 2
    if out is None:
        out = (torch.empty((B, k), dtype=torch.float32, device=dev), torch.empty((B, k), dtype=torch.int64, device=dev),
               torch.empty((B, k, L), dtype=torch.int32, device=dev))[:n_out]
    if len(out) != n_out:
        raise ValueError(f"out must be (vals, idx{', pos' if return_positions else ''})")
    want = ((torch.float32, (B, k)), (torch.int64, (B, k)), (torch.int32, (B, k, L)))
    for t, (dt, shape) in zip(out, want):
        if t.dtype != dt or tuple(t.shape) != shape or t.device != dev or not t.is_contiguous():
            raise ValueError(f"out: want contiguous {dt} {list(shape)} on {dev}, got {t.dtype} {list(t.shape)} on {t.device}")
    pos_ptr = out[2].data_ptr() if return_positions else None
    lib = _lib.lib()
    with torch.cuda.device(dev):
        if score:
            _lib.check(lib.tt_topk_fuse_score_f32(vals.data_ptr(), idx.data_ptr(), B, L, M, table.data_ptr(), miss.data_ptr(), k,
                                                  out[0].data_ptr(), out[1].data_ptr(), pos_ptr, _stream(idx)))
        else:
            _lib.check(lib.tt_topk_fuse_rank_f32(idx.data_ptr(), B, L, M, table.data_ptr(), miss.data_ptr(), k, out[0].data_ptr(),
                                                 out[1].data_ptr(), pos_ptr, _stream(idx)))
    return tuple(out)


def _pack(lists, need_vals: bool):
    """The lists as one ([B,L,M] f32 or None, [B,L,M] int64) pair, shorter lists padded with (-inf, -1); single: the lists
    were one query's 1-D rows."""
    lists = list(lists)
    if not lists:
        raise ValueError("fuse_topk: no lists")
    pairs = []
    for n, pair in enumerate(lists):
        if not isinstance(pair, (tuple, list)) or len(pair) != 2:
            raise ValueError(f"fuse_topk: list {n} must be a (vals, idx) pair")
        v, i = pair
        if not isinstance(i, torch.Tensor) or i.dtype != torch.int64 or i.dim() not in (1, 2):
            raise ValueError(f"fuse_topk: list {n}: idx must be int64 [B,M] ([M] for a single query)")
        if v is None and need_vals:
            raise ValueError(f"fuse_topk: list {n} has no values, which method='score' needs")
        if v is not None and (not isinstance(v, torch.Tensor) or v.dtype != torch.float32 or v.shape != i.shape or v.device != i.device):
            raise ValueError(f"fuse_topk: list {n}: vals must be float32 with idx's shape on idx's device")
        pairs.append((v, i))
    single = pairs[0][1].dim() == 1
    if any((i.dim() == 1) != single for _, i in pairs):
        raise ValueError("fuse_topk: the lists mix single-query [M] and batched [B,M] rows")
    if single:
        pairs = [(None if v is None else v.unsqueeze(0), i.unsqueeze(0)) for v, i in pairs]
    B, dev = pairs[0][1].shape[0], pairs[0][1].device
    if any(i.shape[0] != B or i.device != dev for _, i in pairs):
        raise ValueError("fuse_topk: the lists must hold the same B queries on one device")
    L, M = len(pairs), max(i.shape[1] for _, i in pairs)
    if L > FUSE_LMAX:
        raise ValueError(f"fuse_topk fuses at most {FUSE_LMAX} lists, got L = {L}")
    if M < 1 or L * M > FUSE_EMAX:
        raise ValueError(f"fuse_topk holds 1 <= L * M <= {FUSE_EMAX} entries per query, got {L} * {M} = {L * M}")
    idx = torch.full((B, L, M), -1, dtype=torch.int64, device=dev)
    vals = torch.full((B, L, M), -math.inf, dtype=torch.float32, device=dev) if need_vals else None
    for l, (v, i) in enumerate(pairs):
        idx[:, l, :i.shape[1]] = i
        if need_vals:
            vals[:, l, :i.shape[1]] = v
    return vals, idx, single


def fuse_topk(lists: Sequence, k: int, method: str = "rrf", c: float = 60.0, weights=None, missing=None,
              normalize: Optional[str] = None, return_positions: bool = False, out=None):
    """The best k ids of the union of L ranked lists per query (tt_topk_fuse_rank_f32 / _score_f32, one launch).
    lists: a sequence of (vals f32 [B,M_l], idx int64 [B,M_l]) pairs as the searches and merges return them -- equal B, any
    widths, padding (-inf, idx < 0) at the tail -- packed into one [B,L,M] pair, M = the largest width, with (-inf, -1)
    padding.  L <= 8, L * M <= 1024, 1 <= k <= L * M.  With method="rrf" only the ids are read (vals may be None).
    method="rrf": the term of list l at column m is weights[l] / (c + m + 1) (float64, rounded once: rrf_weights); any other
    rank weighting -- Borda counts, a cut-off -- is a float32 [L,M] DEVICE tensor passed as weights, used as the table.
    method="score": the term is fl32(weights[l] * value).  Either way an id that a list lacks takes missing[l] (0 by default)
    from it, the terms are added in list order in fp32, and the first occurrence of an id in a list counts.
    weights / missing: sequences of L finite floats (device copies are cached per (L, M, c, weights)), or float32 device
    tensors ([L]; the rrf table [L,M]) read at launch time, so that a captured graph sees rewritten values.
    normalize="minmax" (method="score" only): every list's valid values are mapped to [0,1] per query first, a constant list
    to 1 -- torch element-wise ops in front of the launch, outside the kernel's bit-level contract.
    Returns (vals f32 [B,k], idx int64 [B,k]) sorted by (fused desc, id asc), tail (-inf, -1); with return_positions also
    pos int32 [B,k,L]: the column of result r in list l, -1 where it is absent (gather component scores with it).
    1-D lists ([M_l]) are one query's: squeezed results.  out: optional (vals, idx[, pos]) to write into.  Runs on the current
    stream, asynchronous to the host."""
    if method not in ("rrf", "score"):
        raise ValueError(f"method must be 'rrf' or 'score', got {method!r}")
    vals, idx, single = _pack(lists, method == "score")
    if single and out is not None:
        raise ValueError("out= needs batched lists")
    res = _fuse_packed(vals, idx, k, method, c, weights, missing, normalize, return_positions, out)
    return tuple(t[0] for t in res) if single else res


def _fetch_k(k: int, fetch_k: Optional[int]) -> int:
    """How many rows every list of a fused search holds: fetch_k, by default min(max(4 k, 64), 512)."""
    k = int(k)
    if k < 1:
        raise ValueError(f"fused search: k = {k} < 1")
    fk = min(max(4 * k, 64), 512) if fetch_k is None else int(fetch_k)
    if fk < 1:
        raise ValueError(f"fused search: fetch_k = {fk} < 1")
    return fk


def fused_search(index, q_variants: torch.Tensor, k: int = 10, fetch_k: Optional[int] = None, **fuse_kw):
    """Query expansion: q_variants [B,V,d] holds V phrasings (or towers' outputs) of each of B queries.  One index.search of
    the B * V rows at fetch_k (default min(max(4 k, 64), 512), at most the index's size), then one fuse launch with L = V over
    the rows as they lie -- nothing is copied.  fuse_kw: fuse_topk's method, c, weights, missing, normalize,
    return_positions.  [V,d] is one query's variants: squeezed results."""
    if q_variants.dim() == 2:
        return tuple(t[0] for t in fused_search(index, q_variants.unsqueeze(0), k, fetch_k, **fuse_kw))
    if q_variants.dim() != 3:
        raise ValueError(f"fused_search wants q_variants [B,V,d], got {tuple(q_variants.shape)}")
    B, V, d = q_variants.shape
    fk = _fetch_k(k, fetch_k)
    fk = min(fk, getattr(index, "ntotal", fk))
    k = int(k)
    _check_shape(B, V, fk, k)
    vals, idx = index.search(q_variants.reshape(B * V, d), fk)
    kw = dict(method="rrf", c=60.0, weights=None, missing=None, normalize=None, return_positions=False, out=None)
    unknown = set(fuse_kw) - set(kw)
    if unknown:
        raise TypeError(f"fused_search: unexpected arguments {sorted(unknown)}")
    kw.update(fuse_kw)
    return _fuse_packed(vals.reshape(B, V, fk), idx.reshape(B, V, fk), k, **kw)


def _gather(vals: torch.Tensor, pos: torch.Tensor) -> torch.Tensor:
    """vals [B,M] at columns pos [B,k]; NaN where pos < 0."""
    got = vals.gather(1, pos.clamp(min=0).to(torch.int64))
    return torch.where(pos >= 0, got, torch.full_like(got, math.nan))


class HybridIndex:
    """A dense index and a lexical index over the same ids, searched together: both searches stay on the device and one fuse
    launch ranks the union of their lists (reciprocal rank fusion by default).

    dense_index: a BruteForceIndex, a StreamedIndex or a ShardedIndex (the search is then a collective, as that class's are;
    every rank holds the lexical index of the whole corpus and gets the same rows).  lexical_index: a LexicalIndex whose
    ids (idx_offset + row) name the same documents.

    Callers, streams and threads: search() issues the two searches and the fuse launch on the current stream, in that order;
    it holds no state of its own, so what the two indexes say about concurrent callers holds for it."""

    def __init__(self, dense_index, lexical_index):
        from .lexical import LexicalIndex
        if not isinstance(lexical_index, LexicalIndex):
            raise TypeError(f"HybridIndex wants a LexicalIndex, got {type(lexical_index).__name__}")
        if not hasattr(dense_index, "search") or not hasattr(dense_index, "device"):
            raise TypeError(f"HybridIndex wants a dense index with search() and device, got {type(dense_index).__name__}")
        if dense_index.device != lexical_index.device:
            raise ValueError(f"dense index on {dense_index.device}, lexical index on {lexical_index.device}")
        self.dense = dense_index
        self.lexical = lexical_index

    def search(self, q: torch.Tensor, q_lex, k: int = 10, fetch_k: Optional[int] = None, method: str = "rrf", c: float = 60.0,
               weights=None, keep=None, exclude: Optional[torch.Tensor] = None, return_components: bool = False,
               lex_min_score=None):
        """q [B,d]: the dense queries; q_lex: the same B queries for the lexical index (a scipy sparse [B,F] matrix or a device
        CSR triple).  The two searches run at fetch_k (default min(max(4 k, 64), 512), at most each index's size), then
        fuse_topk(method, c, weights) over (dense, lexical) in that order -> (vals f32 [B,k], idx int64 [B,k]), k <= 2 fetch_k.
        keep: a packed keep-bitmask for this call, given to both searches; a (dense_keep, lexical_keep) pair where the two
        indexes hold different rows (a ShardedIndex takes its rank's).  exclude: per-query lists of global ids [B,E]: the
        dense search takes them as its exclude=, the lexical search runs for fetch_k + E and is filtered the same way, so no
        listed id is returned.  lex_min_score: the lexical search's min_score (documents that share no term with the query
        score 0 and otherwise fill the lexical list in index order).  return_components: also (dense [B,k], lexical [B,k]),
        each result's score in the two lists, NaN where a list lacks it.  [d] with a one-row q_lex is one query."""
        from .index import _check_exclude, _exclude_row, topk_exclude
        if q.dim() == 1:
            res = self.search(q.unsqueeze(0), q_lex, k, fetch_k, method, c, weights, keep, _exclude_row(exclude),
                              return_components, lex_min_score)
            return tuple(t[0] for t in res)
        k = int(k)
        fk = _fetch_k(k, fetch_k)
        # (a ShardedIndex does not know the corpus size: its lists are padded where the corpus is smaller)
        fk_d, fk_l = min(fk, getattr(self.dense, "ntotal", fk)), min(fk, self.lexical.ntotal)
        _check_shape(q.shape[0], 2, max(fk_d, fk_l), k)
        keep_d, keep_l = keep if isinstance(keep, (tuple, list)) else (keep, keep)
        dv, di = self.dense.search(q, fk_d, keep=keep_d, exclude=exclude)
        if exclude is not None:
            exclude, fk_e = _check_exclude(exclude, q.shape[0], fk_l, self.lexical.device)
            lv, li = topk_exclude(*self.lexical.search(q_lex, min(fk_e, self.lexical.ntotal), min_score=lex_min_score, keep=keep_l),
                                  exclude, fk_l)
        else:
            lv, li = self.lexical.search(q_lex, fk_l, min_score=lex_min_score, keep=keep_l)
        res = fuse_topk(((dv, di), (lv, li)), k, method=method, c=c, weights=weights, return_positions=return_components)
        if not return_components:
            return res
        fv, fi, pos = res
        return fv, fi, _gather(dv, pos[:, :, 0]), _gather(lv, pos[:, :, 1])
