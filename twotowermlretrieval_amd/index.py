"""Exact brute-force cosine/dot top-k over a resident document-embedding matrix.

Drop-in for the reference's scoring idiom

    sim = torch.matmul(query_emb, doc_embeddings.t()); torch.topk(sim, k)
    (backend/evaluators.py:185-186, :269-272; backend/trainer.py:62-65)

with the same return convention as torch.topk: (values [B,k] f32 descending,
indices [B,k] int64).  The [B,N] score matrix is never materialised.  Ties are
DEFINED (score desc, index asc); torch.topk leaves them unspecified.

Everything here runs through libtt.so (hand-written HIP, gfx950).  There is no
PyTorch/CPU fallback: inputs must be CUDA(ROCm) tensors.
"""
from __future__ import annotations

import contextlib
import threading
from functools import lru_cache
from typing import Callable, NamedTuple, Optional, Tuple

import torch

from . import _lib

__all__ = ["GraphedSearch", "score_topk", "pack_keep_mask", "topk_merge", "topk_exclude", "score_rank", "score_all", "score_ids", "mmr_select", "topk_collapse", "BruteForceIndex", "ShardedIndex", "PendingSearch", "StreamedIndex",
           "shard_bounds", "seed_union", "score_count", "topk_cut_below", "score_topk_tagged", "score_topk_biased", "l2_bias", "l2_distances", "score_topk_after"]


def _stream(t: torch.Tensor) -> int:
    return torch.cuda.current_stream(t.device).cuda_stream


def _need_cuda(*ts: torch.Tensor) -> None:
    for t in ts:
        if not t.is_cuda:
            raise RuntimeError("twotowermlretrieval_amd: this path runs only on an AMD GPU via libtt.so; "
                               f"got a {t.device} tensor (no CPU fallback exists)")


def _f32c(t: torch.Tensor) -> torch.Tensor:
    if t.dtype != torch.float32:
        raise TypeError(f"expected float32, got {t.dtype}")
    return t if t.is_contiguous() else t.contiguous()


def _docs_c(t: torch.Tensor) -> torch.Tensor:
    """A document matrix as the exact kernels read it: float32, or bfloat16 kept as it is (tt_score_topk_bf16)."""
    if t.dtype == torch.bfloat16:
        return t if t.is_contiguous() else t.contiguous()
    return _f32c(t)


# Above this k the exact search and the merges take the large-k entry points (tt_score_topk_large_*, tt_topk_merge_large,
# tt_topk_merge_shards_large: k <= 1024); at or below it, the k <= 64 calls as they always were.
SMALL_KMAX = 64


class _ExactRoute(NamedTuple):
    """Where an exact search goes: the C entry point, its workspace query, and how the two take their arguments."""
    fn: str
    ws_fn: str
    ws_takes_dtype: bool  # the workspace query ends in a bf16 flag (the large and masked ones; the k <= 64 ones come per dtype)
    masked: bool          # the entry point takes the keep-bitmask, in front of k

    def workspace_bytes(self, B: int, N: int, d: int, k: int, dtype: torch.dtype) -> int:
        tail = (int(dtype == torch.bfloat16),) if self.ws_takes_dtype else ()
        return getattr(_lib.lib(), self.ws_fn)(B, N, d, k, *tail)

    def args(self, q_ptr: int, B: int, d: int, docs_ptr: int, N: int, keep_ptr: Optional[int], k: int, tail: tuple) -> tuple:
        """The entry point's arguments; tail = (idx_offset, values, indices, workspace, workspace bytes, stream)."""
        return (q_ptr, B, d, docs_ptr, N, *((keep_ptr,) if self.masked else ()), k, *tail)


@lru_cache(maxsize=None)  # (eight routes)
def _exact_route(dtype: torch.dtype, k: int, masked: bool) -> _ExactRoute:
    """The one place that names the exact entry points.  A mask takes the masked call at any k; without one k <= 64 stays
    on the calls it always used (the large entry point costs a launch and a larger workspace more)."""
    t = "bf16" if dtype == torch.bfloat16 else "f32"
    if masked:
        return _ExactRoute(f"tt_score_topk_masked_{t}", "tt_score_topk_masked_workspace_bytes", True, True)
    if k > SMALL_KMAX:
        return _ExactRoute(f"tt_score_topk_large_{t}", "tt_score_topk_large_workspace_bytes", True, False)
    return _ExactRoute(f"tt_score_topk_{t}", "tt_score_topk_bf16_workspace_bytes" if t == "bf16" else "tt_score_topk_workspace_bytes",
                       False, False)


def _merge_fn(k: int, kp: int = 0, shards: bool = False) -> str:
    """The C merge a k-merge (of per-shard lists of kp when `shards`) calls."""
    large = k > SMALL_KMAX or kp > SMALL_KMAX
    if shards:
        return "tt_topk_merge_shards_large" if large else "tt_topk_merge_shards"
    return "tt_topk_merge_large" if large else "tt_topk_merge"


@lru_cache(maxsize=None)  # (twelve names; composed once each, not per search)
def _screened_fn(phase: str, bf16: bool, masked: bool = False) -> str:
    """The C entry point of one phase of a screened search: "whole", or "seed_list" then "seeded" (ShardedIndex's union seed).
    masked: the form that takes a keep-bitmask behind N (screen_masked=True indexes under a mask)."""
    infix = {"whole": "", "seed_list": "seed_list_", "seeded": "seeded_"}[phase]
    return f"tt_score_topk_screened_{infix}{'masked_' if masked else ''}{'bf16' if bf16 else 'f32'}"


def _out_pair(B: int, k: int, device, out=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """The (values f32 [B,k], indices int64 [B,k]) a search writes: the caller's `out`, or fresh tensors."""
    if out is not None:
        return out
    return (torch.empty((B, k), dtype=torch.float32, device=device), torch.empty((B, k), dtype=torch.int64, device=device))


def _pad_pair(vals: torch.Tensor, idx: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(vals, idx) filled with the padding of a search that found nothing: (-inf, -1)."""
    vals.fill_(float("-inf"))
    idx.fill_(-1)
    return vals, idx


def _copied(out, vals: torch.Tensor, idx: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """A finished (vals, idx) as the caller gets it: copied into `out` when that is given."""
    if out is None:
        return vals, idx
    out[0].copy_(vals)
    out[1].copy_(idx)
    return out


def _cloned(vals: torch.Tensor, idx: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    return vals.clone(), idx.clone()


def _squeezed(search: Callable, q: torch.Tensor, *args) -> Tuple[torch.Tensor, torch.Tensor]:
    """A single query vector [d]: the same search as the [1,d] batch, squeezed result."""
    vals, idx = search(q.unsqueeze(0), *args)
    return vals[0], idx[0]


def _keep_words(n: int) -> int:
    """Words of a keep-bitmask over n documents (one bit each, 32 per word)."""
    return (n + 31) // 32


_KEEP_DTYPES = tuple(t for t in (torch.int32, getattr(torch, "uint32", None)) if t is not None)


def _check_keep(keep: Optional[torch.Tensor], n: int, device) -> Optional[torch.Tensor]:
    """A packed keep-bitmask over n documents on `device`, as the masked kernels read it (int32 view); None stays None."""
    if keep is None:
        return None
    if keep.dtype not in _KEEP_DTYPES:
        raise TypeError(f"keep must be a packed int32 / uint32 bitmask (pack_keep_mask), got {keep.dtype}")
    if keep.device != device:
        raise ValueError(f"keep on {keep.device} but the documents live on {device}")
    if keep.dim() != 1 or keep.numel() != _keep_words(n):
        raise ValueError(f"keep must hold exactly ceil(N/32) = {_keep_words(n)} words for N = {n}, got {tuple(keep.shape)}")
    keep = keep if keep.is_contiguous() else keep.contiguous()
    return keep if keep.dtype == torch.int32 else keep.view(torch.int32)


def pack_keep_mask(keep_bool: torch.Tensor) -> torch.Tensor:
    """keep_bool [N] on the device (bool, or any dtype: non-zero = keep) -> the packed keep-bitmask int32 [ceil(N/32)] that
    score_topk(..., keep=) and the indexes' search(..., keep=) take: bit n & 31 of word n >> 5 = document n may be returned
    (tt_keep_mask_pack, one launch; the bits beyond N are zero)."""
    _need_cuda(keep_bool)
    if keep_bool.dim() != 1:
        raise ValueError(f"pack_keep_mask wants a [N] vector, got {tuple(keep_bool.shape)}")
    b = keep_bool if keep_bool.dtype in (torch.bool, torch.uint8) else keep_bool != 0
    b = b.contiguous().view(torch.uint8)
    n = b.numel()
    keep = torch.empty(_keep_words(n), dtype=torch.int32, device=b.device)
    with torch.cuda.device(b.device):
        _lib.check(_lib.lib().tt_keep_mask_pack(b.data_ptr(), n, keep.data_ptr(), _stream(b)))
    return keep


def _clear_ids(keep: Optional[torch.Tensor], n: int, device, ids, idx_offset: int) -> torch.Tensor:
    """remove_ids of the indexes: `keep` (an all-ones mask over n documents when None) with the bits of the global ids that
    fall in [idx_offset, idx_offset + n) cleared in place, one launch (tt_keep_mask_clear_ids); other ids are ignored."""
    if keep is None:
        keep = torch.full((_keep_words(n),), -1, dtype=torch.int32, device=device)
        if n % 32:  # (the kernels ignore the bits beyond n; zero like pack_keep_mask's, so that the two compare equal)
            keep[-1] = (1 << (n % 32)) - 1
    ids = torch.as_tensor(ids, dtype=torch.int64, device=device).reshape(-1).contiguous()
    with torch.cuda.device(device):
        _lib.check(_lib.lib().tt_keep_mask_clear_ids(keep.data_ptr(), n, ids.data_ptr(), ids.numel(), idx_offset, _stream(keep)))
    return keep


def _and_keep(persistent: Optional[torch.Tensor], keep: Optional[torch.Tensor], n: int, device) -> Optional[torch.Tensor]:
    """The mask a search runs under: the index's persistent mask, the caller's per-call one, or their AND (one torch op on
    n/32 words); None = unmasked."""
    keep = _check_keep(keep, n, device)
    if keep is None:
        return persistent
    return keep if persistent is None else keep & persistent


def _keep_slice(keep: Optional[torch.Tensor], lo: int, n: int) -> Optional[torch.Tensor]:
    """The words of a checked keep-bitmask that cover rows [lo, lo + n), lo a multiple of 32 (a StreamedIndex block's)."""
    return None if keep is None else keep[lo // 32:lo // 32 + _keep_words(n)]


def _front(q: torch.Tensor, docs: torch.Tensor, docs_c: Callable = _docs_c) -> Tuple[torch.Tensor, torch.Tensor]:
    """What every module-level scoring function checks first of q [B,d] and docs [N,d]: both on the GPU, q float32 and docs
    as the kernels read them (docs_c: _docs_c, or _f32c where no bf16 kernel exists), contiguous, of one width."""
    _need_cuda(q, docs)
    q, docs = _f32c(q), docs_c(docs)
    if docs.dim() != 2 or docs.shape[1] != q.shape[1]:
        raise ValueError(f"shape mismatch: q {tuple(q.shape)} vs docs {tuple(docs.shape)}")
    return q, docs


def score_topk(q: torch.Tensor, docs: torch.Tensor, k: int, idx_offset: int = 0,
               workspace: Optional[torch.Tensor] = None, keep: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """topk(q @ docs.T, k) fused.  q [B,d] or [d] float32; docs [N,d] (row i <-> document i), float32 or bfloat16.  A bf16
    matrix is read as it is (d in {64, 128, 192, 256}); the result is that of its exact fp32 widening, bit for bit.
    keep: a packed keep-bitmask (pack_keep_mask: int32 / uint32, exactly ceil(N/32) words, on the documents' device) -> the
    exact top-k of the documents whose bit is set (tt_score_topk_masked_f32 / _bf16, any k up to 1024), tail (-inf, -1) when
    fewer than k are kept.  A masked document is still read and scored: a selective mask pays the full scan."""
    if q.dim() == 1:
        return _squeezed(score_topk, q, docs, k, idx_offset, workspace, keep)
    q, docs = _front(q, docs)
    B, d = q.shape
    N = docs.shape[0]
    keep = _check_keep(keep, N, docs.device)
    vals, idx = _out_pair(B, k, q.device)
    with torch.cuda.device(q.device):  # workspace sizing depends on the device's CU count
        route = _exact_route(docs.dtype, k, keep is not None)
        need = route.workspace_bytes(B, N, d, k, docs.dtype)
        if workspace is None or workspace.numel() < need:
            workspace = torch.empty(max(need, 16), dtype=torch.uint8, device=q.device)
        tail = (idx_offset, vals.data_ptr(), idx.data_ptr(), workspace.data_ptr(), workspace.numel(), _stream(q))
        _lib.check(getattr(_lib.lib(), route.fn)(*route.args(q.data_ptr(), B, d, docs.data_ptr(), N,
                                                             None if keep is None else keep.data_ptr(), k, tail)))
    return vals, idx


def _tag_words(n: int) -> int:
    """Words of a tags buffer over n documents as the tagged kernels read it: one per document, whole 32-document tiles."""
    return 32 * _keep_words(n)


def _check_tags(tags: torch.Tensor, n: int, device) -> torch.Tensor:
    """The tags of n documents on `device` as tt_score_topk_tagged_* reads them: int32 [32*ceil(n/32)], contiguous (the bit
    pattern is read as unsigned).  A [n] tensor is padded with zeros, which the kernels ignore."""
    if not isinstance(tags, torch.Tensor) or tags.dtype not in _KEEP_DTYPES:
        raise TypeError(f"tags must be an int32 / uint32 tensor, one word per document, got {getattr(tags, 'dtype', type(tags))}")
    if tags.device != device:
        raise ValueError(f"tags on {tags.device} but the documents live on {device}")
    if tags.dim() != 1 or tags.numel() not in (n, _tag_words(n)):
        raise ValueError(f"tags must hold N = {n} words (or N padded to whole tiles, {_tag_words(n)}), got {tuple(tags.shape)}")
    tags = tags if tags.dtype == torch.int32 else tags.view(torch.int32)
    if tags.numel() != _tag_words(n):
        padded = torch.zeros(_tag_words(n), dtype=torch.int32, device=device)
        padded[:n] = tags
        return padded
    return tags if tags.is_contiguous() else tags.contiguous()


def _match_words(x, B: int, device, what: str) -> torch.Tensor:
    """match_mask / match_value of B queries on `device` as the tagged kernels read them (int32 [B], contiguous): an int32
    [B] device tensor, or a Python int in [-2^31, 2^32) (its low 32 bits) for every query."""
    if isinstance(x, torch.Tensor):
        if x.dtype not in _KEEP_DTYPES:
            raise TypeError(f"{what} must be an int or an int32 / uint32 tensor, got {x.dtype}")
        if x.device != device:
            raise ValueError(f"{what} on {x.device} but the search runs on {device}")
        if tuple(x.shape) != (B,):
            raise ValueError(f"{what} must be one word per query, [B] = [{B}], got {tuple(x.shape)}")
        x = x if x.dtype == torch.int32 else x.view(torch.int32)
        return x if x.is_contiguous() else x.contiguous()
    if isinstance(x, bool) or not isinstance(x, int):
        raise TypeError(f"{what} must be an int or an int32 / uint32 tensor, got {type(x).__name__}")
    if not -(1 << 31) <= x < (1 << 32):
        raise ValueError(f"{what} = {x} is not a 32-bit word")
    x &= 0xffffffff
    return torch.full((B,), x - (1 << 32) if x >= (1 << 31) else x, dtype=torch.int32, device=device)


TAGGED_KMAX = SMALL_KMAX  # tagged search keeps the k <= 64 lists only (tt_score_topk_tagged_*)
BIASED_KMAX = SMALL_KMAX  # biased search keeps the k <= 64 lists only (tt_score_topk_biased_*)
AFTER_KMAX = SMALL_KMAX   # one cursor call answers k <= 64 (tt_score_topk_after_*): a larger page is two consecutive calls


class _Mode(NamedTuple):
    """One k <= 64 mode of the exact kernel: its entry points, its bound on k and the words of its refusals.  The entry
    points take (q, B, d, docs, N, *the mode's own tensors, keep, k, idx_offset, vals, idx, workspace, its bytes, stream)."""
    ws_fn: str
    fn_f32: str
    fn_bf16: str
    kmax: int
    subject: str    # "... answers 1 <= k <= kmax"
    per: str = ""   # behind the bound of one call
    hint: str = ""  # behind the refusal of one call, where a deeper search exists

    def check_k(self, k: int, hint: bool = True) -> None:
        if not 1 <= k <= self.kmax:
            raise ValueError(f"{self.subject} answers 1 <= k <= {self.kmax}{self.per}, got k = {k}{self.hint if hint else ''}")

    def shard_k(self, k: int, shard_k: int) -> int:
        """max(k, shard_k), the length of a shard's list (ShardedIndex), which the mode must answer."""
        kp = max(k, shard_k)
        if not 1 <= k or kp > self.kmax:
            raise ValueError(f"{self.subject} answers 1 <= max(k, shard_k) <= {self.kmax}, got k = {k}, shard_k = {shard_k}")
        return kp


def _mode(stem: str, kmax: int, subject: str, per: str = "", hint: str = "") -> _Mode:
    return _Mode(f"tt_score_topk_{stem}_workspace_bytes", f"tt_score_topk_{stem}_f32", f"tt_score_topk_{stem}_bf16", kmax,
                 subject, per, hint)


# The one place that names the modes' entry points; their own tensors are (tags, match_mask, match_value), (bias,), (av, ai).
_TAGGED = _mode("tagged", TAGGED_KMAX, "tagged search")
_BIASED = _mode("biased", BIASED_KMAX, "biased search")
_AFTER = _mode("after", AFTER_KMAX, "a cursor search", " per call", " (pages() / deep_search() go deeper)")


def _mode_into(mode: _Mode, q: torch.Tensor, docs: torch.Tensor, own: tuple, keep: Optional[torch.Tensor], k: int,
               idx_offset: int, out=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """A mode's entry point over checked arguments: q [B,d] f32, docs [N,d] f32 or bf16, `own` the mode's tensors as its
    kernel reads them (padded tags and int32 [B] match words; a padded bias whose storage is 16-byte aligned; a checked
    cursor, _cursor), keep a checked keep-bitmask or None -> (vals, idx), `out` when given."""
    mode.check_k(k)
    B, d = q.shape
    N = docs.shape[0]
    bf16 = docs.dtype == torch.bfloat16
    pair = _out_pair(B, k, q.device, out)
    if N == 0 or B == 0:  # (an empty torch tensor has no address to hand to the call)
        _pad_pair(*pair)
        return pair
    vals, idx = pair
    with torch.cuda.device(q.device):  # workspace sizing depends on the device's CU count
        L = _lib.lib()
        ws = torch.empty(max(getattr(L, mode.ws_fn)(B, N, d, k, int(bf16)), 16), dtype=torch.uint8, device=q.device)
        fn = getattr(L, mode.fn_bf16 if bf16 else mode.fn_f32)
        _lib.check(fn(q.data_ptr(), B, d, docs.data_ptr(), N, *[t.data_ptr() for t in own],
                      None if keep is None else keep.data_ptr(), k, idx_offset, vals.data_ptr(), idx.data_ptr(), ws.data_ptr(),
                      ws.numel(), _stream(q)))
    return pair


def score_topk_tagged(q: torch.Tensor, docs: torch.Tensor, tags: torch.Tensor, match_mask, match_value, k: int,
                      idx_offset: int = 0, keep: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """score_topk with a filter per query, in one pass over docs: query b sees document n iff
    (tags[n] & match_mask[b]) == match_value[b] (and its bit in `keep`, a pack_keep_mask bitmask, when given).  tags: int32
    [N] or [32*ceil(N/32)] on the documents' device, one word per document, read as unsigned (a [N] tensor is padded here).
    match_mask / match_value: int32 [B] device tensors, or Python ints for every query.  Mask 0xffffffff is equality on the
    whole tag, mask 0 with value 0 no filter, a value with a bit outside the mask matches nothing.  Returns the exact top-k
    of each query's eligible documents, (score desc, index asc), tail (-inf, -1) -- what score_topk(q[b], docs, k, keep=
    that eligibility) returns, bit for bit (tt_score_topk_tagged_f32 / _bf16; k <= 64).  An ineligible document is still read
    and scored: the batch pays one full scan, whatever its filters."""
    if q.dim() == 1:
        return _squeezed(score_topk_tagged, q, docs, tags, match_mask, match_value, k, idx_offset, keep)
    q, docs = _front(q, docs)
    B, N = q.shape[0], docs.shape[0]
    tags = _check_tags(tags, N, docs.device)
    mm = _match_words(match_mask, B, docs.device, "match_mask")
    mv = _match_words(match_value, B, docs.device, "match_value")
    return _mode_into(_TAGGED, q, docs, (tags, mm, mv), _check_keep(keep, N, docs.device), k, int(idx_offset))


def _check_bias(bias: torch.Tensor, n: int, device) -> torch.Tensor:
    """The biases of n documents on `device` as tt_score_topk_biased_* reads them: float32 [32*ceil(n/32)], contiguous.  A
    [n] tensor is padded with zeros (the kernels ignore the words beyond n whatever they hold)."""
    if not isinstance(bias, torch.Tensor) or bias.dtype != torch.float32:
        raise TypeError(f"bias must be a float32 tensor, one value per document, got {getattr(bias, 'dtype', type(bias))}")
    if bias.device != device:
        raise ValueError(f"bias on {bias.device} but the documents live on {device}")
    if bias.dim() != 1 or bias.numel() not in (n, _tag_words(n)):
        raise ValueError(f"bias must hold N = {n} values (or N padded to whole tiles, {_tag_words(n)}), got {tuple(bias.shape)}")
    if bias.numel() != _tag_words(n):
        padded = torch.zeros(_tag_words(n), dtype=torch.float32, device=device)
        padded[:n] = bias
        return padded
    return bias if bias.is_contiguous() else bias.contiguous()


def _set_bias(bias: Optional[torch.Tensor], n: int, device) -> Optional[torch.Tensor]:
    """set_bias of the indexes: the checked, padded biases of n rows on `device` (None clears them), with the one finiteness
    check of the first n values (a host synchronisation on a device tensor)."""
    if bias is None:
        return None
    bias = _check_bias(bias, n, device)
    if not bool(torch.isfinite(bias[:n]).all()):
        raise ValueError("set_bias: every bias must be finite (NaN or +-inf found)")
    return bias


def score_topk_biased(q: torch.Tensor, docs: torch.Tensor, bias: torch.Tensor, k: int, idx_offset: int = 0,
                      keep: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """topk(q @ docs.T + bias[None, :], k) fused, in one pass over docs and without the [B,N] matrix: document n scores
    fl32(s + bias[n]), s being score_topk's score -- one fp32 add behind the finished multiply chain.  bias: float32 [N] or
    [32*ceil(N/32)] on the documents' device (a [N] tensor is padded here): a popularity or recency prior, a boost or a
    demotion; l2_bias(docs) makes the ranking that of the Euclidean distance.  keep: a pack_keep_mask bitmask, as in
    score_topk.  Returns the exact top-k of the biased score over the kept documents, (score desc, index asc), tail
    (-inf, -1); the values are the biased scores (tt_score_topk_biased_f32 / _bf16; k <= 64).  The biases must be finite: this
    function does NOT check it, a check would need a host synchronisation (the indexes' set_bias checks once)."""
    if q.dim() == 1:
        return _squeezed(score_topk_biased, q, docs, bias, k, idx_offset, keep)
    q, docs = _front(q, docs)
    N = docs.shape[0]
    bias = _check_bias(bias, N, docs.device)
    return _mode_into(_BIASED, q, docs, (bias,), _check_keep(keep, N, docs.device), k, int(idx_offset))


def l2_bias(docs: torch.Tensor) -> torch.Tensor:
    """float32 [N]: -|d_n|^2 / 2 of every row of docs [N,d] (float32 or bfloat16, any device), each row's sum of squares taken
    in float64 (bf16 rows: over their widened values) and rounded once.  With this bias a biased search ranks by
    q.d - |d|^2/2 = (|q|^2 - |q - d|^2) / 2, the order of the Euclidean distance; l2_distances maps the values back."""
    if docs.dim() != 2:
        raise ValueError(f"l2_bias wants docs [N,d], got {tuple(docs.shape)}")
    out = torch.empty(docs.shape[0], dtype=torch.float32, device=docs.device)
    step = 1 << 16  # (rows per chunk: the float64 copy stays small next to the corpus)
    for lo in range(0, docs.shape[0], step):
        rows = docs[lo:lo + step].to(torch.float64)
        out[lo:lo + step] = (rows * rows).sum(dim=1).mul_(-0.5).to(torch.float32)
    return out


def l2_distances(q: torch.Tensor, vals: torch.Tensor) -> torch.Tensor:
    """Squared Euclidean distances of a biased search under l2_bias: q [B,d] (or [d]) and the values [B,k] (or [k]) it
    returned -> |q|^2 - 2 vals, clamped at 0, with the (-inf) tail mapped to +inf.  float32, ascending along k."""
    qn = (q.to(torch.float32) ** 2).sum(dim=-1, keepdim=True)
    return (qn - 2.0 * vals).clamp_(min=0.0)


def _cursor(after, B: int, device) -> Tuple[torch.Tensor, torch.Tensor]:
    """The cursors of B queries on `device` as tt_score_topk_after_* reads them: (float32 [B], int64 [B]), contiguous.
    after = (vals, ids): each a tensor of B elements on the device (a 0-d tensor or [1] for a single query) or a Python
    number for every query; None = the open cursor (+inf, -1), in front of every document."""
    av, ai = (float("inf"), -1) if after is None else after
    parts = []
    for x, dtype, what in ((av, torch.float32, "score"), (ai, torch.int64, "id")):
        if isinstance(x, torch.Tensor):
            if x.dtype != dtype:
                raise TypeError(f"the cursor's {what}s must be {dtype}, got {x.dtype}")
            if x.device != device:
                raise ValueError(f"the cursor's {what}s on {x.device} but the search runs on {device}")
            if x.numel() != B or x.dim() > 1:
                raise ValueError(f"the cursor holds one {what} per query ([{B}]), got {tuple(x.shape)}")
            parts.append(x.reshape(B).contiguous())
        elif isinstance(x, bool) or not isinstance(x, (int, float)) or (dtype == torch.int64 and not isinstance(x, int)):
            raise TypeError(f"the cursor's {what} must be a {dtype} tensor or a Python {'int' if dtype == torch.int64 else 'float'}, got {type(x)}")
        else:
            if dtype == torch.int64 and not -(1 << 63) <= x < (1 << 63):
                raise ValueError(f"the cursor's id {x} is no int64")
            parts.append(torch.full((B,), x, dtype=dtype, device=device))
    return parts[0], parts[1]


def score_topk_after(q: torch.Tensor, docs: torch.Tensor, after_val, after_idx, k: int, idx_offset: int = 0,
                     keep: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """The next k results after a cursor, in one pass over docs: document n (global id g = n + idx_offset) with score s --
    score_topk's score, the same bits -- is eligible for query b iff it lies strictly after (after_val[b], after_idx[b]) in the
    order (score desc, index asc): s < a or (s == a and g > i).  after_val: float32 [B] on the device or a Python float,
    after_idx: int64 [B] GLOBAL ids or a Python int (any int64: ids of other shards are ordinary).  (+inf, -1) is the open
    cursor (score_topk's result), (ceiling, -1) asks for the k best documents that score at most `ceiling`, the last column of
    a page asks for the next page, and (-inf, -1) -- the tail of an exhausted page -- returns nothing.  keep: a pack_keep_mask
    bitmask, as in score_topk.  Returns the exact top-k of the eligible kept documents, tail (-inf, -1)
    (tt_score_topk_after_f32 / _bf16; k <= 64 per call)."""
    if q.dim() == 1:
        return _squeezed(score_topk_after, q, docs, after_val, after_idx, k, idx_offset, keep)
    q, docs = _front(q, docs)
    cursor = _cursor((after_val, after_idx), q.shape[0], docs.device)
    return _mode_into(_AFTER, q, docs, cursor, _check_keep(keep, docs.shape[0], docs.device), k, int(idx_offset))


class _CursorSearch:
    """What the three indexes share of the cursor search: search_after's front (a single query, exclude=), pages() and
    deep_search().  An index supplies _search_after(q [B,d], k, av, ai, keep, out) and _cursor_device()."""

    def search_after(self, q: torch.Tensor, k: int, after=None, keep: Optional[torch.Tensor] = None,
                     exclude: Optional[torch.Tensor] = None, out=None) -> Tuple[torch.Tensor, torch.Tensor]:
        """The next k results after a cursor (score_topk_after): after = (vals [B], ids [B]) with GLOBAL ids -- tensors on
        the index's device or Python numbers -- or None, the open cursor; q [B,d] or a single [d].  The last column of a page
        is the cursor of the next one; (ceiling, -1) asks for the k best rows that score at most `ceiling`.  Exact at any
        depth, one pass over the rows per call.  keep= and remove_ids compose as in tagged_search.  exclude= (int64 [B,E];
        [E] with a 1-D q) takes biased_search's route: a cursor search for k + E, then the filter (tt_topk_exclude_ids); the
        bound is k + E <= 64.  Always the exact kernel in its cursor mode, also on a screen=True index, whose fallback_flags
        then read all ones as after tagged_search.  ValueError: k (+ E) > 64 -- pages() and deep_search() go deeper."""
        if q.dim() == 1:
            return _squeezed(self.search_after, q, k, after, keep, _exclude_row(exclude))
        _need_cuda(q)
        dev = self._cursor_device()
        B = q.shape[0]
        if exclude is not None:
            exclude, kk = _check_exclude(exclude, B, k, dev)
            if kk > AFTER_KMAX:
                raise ValueError(f"a cursor search with an exclusion list runs for k + E = {kk} > {AFTER_KMAX}")
            v, i = self.search_after(q, kk, after, keep)
            return topk_exclude(v, i, exclude, k, out)
        av, ai = _cursor(after, B, dev)
        return self._search_after(q, k, av, ai, keep, out)

    def pages(self, q: torch.Tensor, k: int, n_pages: Optional[int] = None, keep: Optional[torch.Tensor] = None):
        """A generator of consecutive result pages (vals [B,k], idx [B,k]) of q, k <= 64 per page: the first is search_after's
        under the open cursor, and each further page's cursor is the previous page's last column, taken on the device with
        no host synchronisation.  One pass over the rows per page, however deep.  It stops after n_pages; with n_pages=None it
        never stops by itself -- a query whose rows are used up yields (-inf, -1) tails from then on (the tail is a valid
        cursor that returns nothing), and telling that takes a look at the values, which is the caller's to spend."""
        after = None
        n = 0
        while n_pages is None or n < n_pages:
            v, i = self.search_after(q, k, after, keep=keep)
            yield v, i
            after = (v[..., -1].clone(), i[..., -1].clone())
            n += 1

    def deep_search(self, q: torch.Tensor, k_total: int, keep: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """The exact top-k_total at ANY depth (search() stops at k = 1024): ceil(k_total / 64) pages of 64 concatenated and cut
        to k_total.  The cost is one pass over the rows per 64 results -- 16 passes where search(k = 1024) takes one to three,
        so below 1024 search() is the call to make."""
        if k_total < 1:
            raise ValueError(f"k_total = {k_total} < 1")
        got = list(self.pages(q, AFTER_KMAX, n_pages=(k_total + AFTER_KMAX - 1) // AFTER_KMAX, keep=keep))
        return (torch.cat([v for v, _ in got], dim=-1)[..., :k_total].contiguous(),
                torch.cat([i for _, i in got], dim=-1)[..., :k_total].contiguous())


def topk_merge(vals: torch.Tensor, idx: torch.Tensor, k: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """Top-k of [B,M] unordered candidates (idx < 0 = padding); (score desc, index asc)."""
    _need_cuda(vals, idx)
    vals = _f32c(vals)
    idx = idx.contiguous()
    if idx.dtype != torch.int64 or vals.shape != idx.shape or vals.dim() != 2:
        raise ValueError("topk_merge wants vals f32 [B,M] and idx int64 [B,M]")
    B, M = vals.shape
    ov, oi = _out_pair(B, k, vals.device)
    with torch.cuda.device(vals.device):
        _lib.check(getattr(_lib.lib(), _merge_fn(k))(vals.data_ptr(), idx.data_ptr(), B, M, k, ov.data_ptr(),
                                                     oi.data_ptr(), _stream(vals)))
    return ov, oi


EXCLUDE_KMAX = 1024  # k + E of a search with an exclusion list: TT_TOPK_LARGE_KMAX, what every path answers exactly


def _check_exclude(exclude: torch.Tensor, B: int, k: int, device) -> Tuple[torch.Tensor, int]:
    """A per-query exclusion list for B queries on `device` as tt_topk_exclude_ids reads it (int64 [B,E], contiguous), and the
    k + E the search in front of the filter runs for."""
    if not isinstance(exclude, torch.Tensor) or exclude.dtype != torch.int64:
        raise ValueError(f"exclude must be an int64 tensor of document ids, got {getattr(exclude, 'dtype', type(exclude))}")
    if exclude.device != device:
        raise ValueError(f"exclude on {exclude.device} but the search runs on {device}")
    if exclude.dim() != 2 or exclude.shape[0] != B:
        raise ValueError(f"exclude must be [B,E] = [{B},E] (one list per query; [E] for a single query), got {tuple(exclude.shape)}")
    E = exclude.shape[1]
    if k < 1:
        raise ValueError(f"k = {k} < 1")
    if k + E > EXCLUDE_KMAX:
        raise ValueError(f"k + E = {k} + {E} = {k + E} > {EXCLUDE_KMAX}: a search with an exclusion list runs for k + E")
    return (exclude if exclude.is_contiguous() else exclude.contiguous()), k + E


def _exclude_row(exclude: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    """The [1,E] list of a single query's [E] list."""
    if exclude is None:
        return None
    if not isinstance(exclude, torch.Tensor) or exclude.dim() != 1:
        raise ValueError(f"a single query takes exclude [E], got {tuple(getattr(exclude, 'shape', ()))}")
    return exclude.unsqueeze(0)


def topk_exclude(vals: torch.Tensor, idx: torch.Tensor, exclude: torch.Tensor, k: int, out=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Per-query exclusion over sorted lists the caller holds: vals f32 / idx int64 [B,M] as the searches and merges return
    them ((score desc, index asc), padding at the tail), exclude int64 [B,E] (ids as in idx; negative = padding) -> the first k
    entries of each row whose index is not in that row's list, then (-inf, -1) (tt_topk_exclude_ids, one launch).  Rows that
    are the exact top-(k + E) give the exact top-k of the documents not listed.  out: optional (vals [B,k], idx [B,k])."""
    _need_cuda(vals, idx, exclude)
    vals = _f32c(vals)
    if idx.dtype != torch.int64 or vals.shape != idx.shape or vals.dim() != 2:
        raise ValueError("topk_exclude wants vals f32 [B,M] and idx int64 [B,M]")
    idx = idx.contiguous()
    B, M = vals.shape
    if exclude.dtype != torch.int64 or exclude.device != vals.device or exclude.dim() != 2 or exclude.shape[0] != B:
        raise ValueError(f"topk_exclude wants exclude int64 [{B},E] on {vals.device}, got {exclude.dtype} {tuple(exclude.shape)} on {exclude.device}")
    exclude = exclude.contiguous()
    ov, oi = _out_pair(B, k, vals.device, out)
    with torch.cuda.device(vals.device):
        _lib.check(_lib.lib().tt_topk_exclude_ids(vals.data_ptr(), idx.data_ptr(), B, M, exclude.data_ptr(), exclude.shape[1], k,
                                                  ov.data_ptr(), oi.data_ptr(), _stream(vals)))
    return ov, oi


def _min_score(min_score, B: int, device) -> torch.Tensor:
    """The thresholds of a threshold search of B queries on `device` as the C calls read them (float32 [B], contiguous): a
    Python number for every query, or a float32 [B] tensor on the device (a 0-d tensor or [1] for a single query vector)."""
    if isinstance(min_score, torch.Tensor):
        if min_score.dtype != torch.float32:
            raise TypeError(f"min_score must be a float or a float32 tensor, got {min_score.dtype}")
        if min_score.device != device:
            raise ValueError(f"min_score on {min_score.device} but the search runs on {device}")
        if min_score.dim() == 0 and B == 1:
            min_score = min_score.reshape(1)
        if tuple(min_score.shape) != (B,):
            raise ValueError(f"min_score must be one threshold per query, [B] = [{B}], got {tuple(min_score.shape)}")
        return min_score if min_score.is_contiguous() else min_score.contiguous()
    if isinstance(min_score, bool) or not isinstance(min_score, (int, float)):
        raise TypeError(f"min_score must be a float or a float32 tensor, got {type(min_score).__name__}")
    return torch.full((B,), float(min_score), dtype=torch.float32, device=device)


def _count_into(q: torch.Tensor, docs: torch.Tensor, thr: torch.Tensor, keep: Optional[torch.Tensor], count: torch.Tensor,
                accumulate: bool) -> None:
    """tt_score_count_f32 / _bf16 of checked arguments: q [B,d] f32, docs [N,d] f32 or bf16, thr [B] f32, keep a checked
    keep-bitmask or None, count int64 [B] (added to when `accumulate`)."""
    B, d = q.shape
    N = docs.shape[0]
    bf16 = docs.dtype == torch.bfloat16
    with torch.cuda.device(q.device):  # workspace sizing depends on the device's CU count
        L = _lib.lib()
        ws = torch.empty(max(L.tt_score_count_workspace_bytes(B, N, d, int(bf16)), 16), dtype=torch.uint8, device=q.device)
        fn = L.tt_score_count_bf16 if bf16 else L.tt_score_count_f32
        _lib.check(fn(q.data_ptr(), B, d, docs.data_ptr(), N, None if keep is None else keep.data_ptr(), thr.data_ptr(),
                      count.data_ptr(), int(accumulate), ws.data_ptr(), ws.numel(), _stream(q)))


def score_count(q: torch.Tensor, docs: torch.Tensor, min_score, keep: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(q @ docs.T >= min_score).sum(1) fused: int64 [B] (0-d for a single query [d]), the number of documents whose score --
    score_topk's fp32 chain, bit for bit -- is at least the query's threshold.  min_score: a Python float, or a float32 [B]
    device tensor (one threshold per query); NaN counts nothing, -inf counts every (kept) document.  docs float32 or
    bfloat16 like score_topk's; keep: a packed keep-bitmask (pack_keep_mask) -> only the kept documents are counted.  One
    pass of the exact kernel over docs in its counting mode (tt_score_count_f32 / _bf16): the cost of an exact search."""
    if q.dim() == 1:
        return score_count(q.unsqueeze(0), docs, min_score, keep)[0]
    q, docs = _front(q, docs)
    thr = _min_score(min_score, q.shape[0], q.device)
    keep = _check_keep(keep, docs.shape[0], docs.device)
    count = torch.empty(q.shape[0], dtype=torch.int64, device=q.device)
    _count_into(q, docs, thr, keep, count, False)
    return count


def topk_cut_below(vals: torch.Tensor, idx: torch.Tensor, min_score) -> Tuple[torch.Tensor, torch.Tensor]:
    """Cut sorted top-k rows at a per-query threshold, IN PLACE: every entry of row b of vals f32 / idx int64 [B,k] that is
    not >= min_score[b] (or is padding) becomes (-inf, -1) (tt_topk_cut_below, one launch).  Returns (vals, idx)."""
    _need_cuda(vals, idx)
    if (vals.dtype != torch.float32 or idx.dtype != torch.int64 or vals.shape != idx.shape or vals.dim() != 2
            or not vals.is_contiguous() or not idx.is_contiguous()):
        raise ValueError("topk_cut_below wants contiguous vals f32 [B,k] and idx int64 [B,k]")
    B, k = vals.shape
    thr = _min_score(min_score, B, vals.device)
    if B and k:
        with torch.cuda.device(vals.device):
            _lib.check(_lib.lib().tt_topk_cut_below(vals.data_ptr(), idx.data_ptr(), B, k, thr.data_ptr(), _stream(vals)))
    return vals, idx


def _range_search(index, q: torch.Tensor, min_score, k: int, keep: Optional[torch.Tensor]):
    """range_search of every index: its count, and its own search for k cut at the thresholds."""
    if q.dim() == 1:
        c, v, i = _range_search(index, q.unsqueeze(0), min_score, k, keep)
        return c[0], v[0], i[0]
    _need_cuda(q)
    thr = _min_score(min_score, q.shape[0], index.device)
    counts = index.count(q, thr, keep=keep)
    vals, idx = index.search(q, k, keep=keep)
    vals, idx = topk_cut_below(vals.contiguous(), idx.contiguous(), thr)
    return counts, vals, idx


_RANGE_DOC = """(counts int64 [B], vals f32 [B,k], idx int64 [B,k]): counts[b] = the number of (kept, not removed) documents with
        score >= min_score[b] (count()), and row b = search(q, k, keep=keep) -- whatever route this index takes -- with the
        entries below the threshold replaced by the (-inf, -1) tail: min(counts[b], k) real entries, the best of the
        counts[b] matches, in the usual order.  min_score: a float, or a float32 [B] device tensor.  exclude= is not taken.
        Cost: the rows are the search's; the count is one more pass of the EXACT kernel over the corpus whatever route the
        search took -- on a screened index at B = 1024 that is tens of ms next to a search of a few ms."""


def score_rank(q: torch.Tensor, docs: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """1-based rank of docs[target[b]] for query b (BatchEvaluator's sort + nonzero, evaluators.py:58-65)."""
    _need_cuda(q, docs, target)
    q, docs = _f32c(q), _f32c(docs)
    target = target.to(torch.int64).contiguous()
    B, d = q.shape
    if ((target < 0) | (target >= docs.shape[0])).any():
        raise IndexError("score_rank: target out of range")
    rank = torch.empty(B, dtype=torch.int64, device=q.device)
    with torch.cuda.device(q.device):
        _lib.check(_lib.lib().tt_score_rank_f32(q.data_ptr(), B, d, docs.data_ptr(), docs.shape[0], target.data_ptr(),
                                                rank.data_ptr(), _stream(q)))
    return rank


def score_all(q: torch.Tensor, docs: torch.Tensor) -> torch.Tensor:
    """q @ docs.T as a [B,N] matrix (same fp32 FMA chain as score_topk's scores): for callers that blend the dense score
    of EVERY document with another signal (backend/simple_hybrid.py:53-56).  Small corpora only: it materialises B*N."""
    squeeze = q.dim() == 1
    if squeeze:
        q = q.unsqueeze(0)
    q, docs = _front(q, docs, _f32c)
    out = torch.empty((q.shape[0], docs.shape[0]), dtype=torch.float32, device=q.device)
    with torch.cuda.device(q.device):
        _lib.check(_lib.lib().tt_score_all_f32(q.data_ptr(), q.shape[0], q.shape[1], docs.data_ptr(), docs.shape[0],
                                               out.data_ptr(), _stream(q)))
    return out[0] if squeeze else out


def _check_ids(ids: torch.Tensor, B: int, device, what: str = "ids") -> torch.Tensor:
    """Per-query candidate lists for B queries on `device` as tt_score_ids_f32 / _bf16 read them (int64 [B,C], contiguous)."""
    if not isinstance(ids, torch.Tensor) or ids.dtype != torch.int64:
        raise TypeError(f"{what} must be an int64 tensor of document ids, got {getattr(ids, 'dtype', type(ids))}")
    if ids.device != device:
        raise ValueError(f"{what} on {ids.device} but the search runs on {device}")
    if ids.dim() != 2 or ids.shape[0] != B:
        raise ValueError(f"{what} must be [B,C] = [{B},C] (one list per query; [C] for a single query), got {tuple(ids.shape)}")
    return ids if ids.is_contiguous() else ids.contiguous()


def _ids_row(ids: Optional[torch.Tensor], what: str = "ids") -> Optional[torch.Tensor]:
    """The [1,C] lists of a single query's [C] list."""
    if ids is None:
        return None
    if not isinstance(ids, torch.Tensor) or ids.dim() != 1:
        raise ValueError(f"a single query takes {what} [C], got {tuple(getattr(ids, 'shape', ()))}")
    return ids.unsqueeze(0)


def _score_ids_into(q: torch.Tensor, docs: torch.Tensor, ids: torch.Tensor, idx_offset: int, keep: Optional[torch.Tensor],
                    out_val: torch.Tensor, out_idx: Optional[torch.Tensor]) -> None:
    """tt_score_ids_f32 / _bf16 of checked arguments: q [B,d] f32, docs [N,d] f32 or bf16, ids int64 [B,C], keep a checked
    keep-bitmask or None -> out_val f32 [B,C] and, unless None, out_idx int64 [B,C], both contiguous."""
    B, d = q.shape
    L = _lib.lib()
    fn = L.tt_score_ids_bf16 if docs.dtype == torch.bfloat16 else L.tt_score_ids_f32
    with torch.cuda.device(q.device):
        _lib.check(fn(q.data_ptr(), B, d, docs.data_ptr() if docs.shape[0] else None, docs.shape[0],
                      None if keep is None else keep.data_ptr(), ids.data_ptr(), ids.shape[1], idx_offset, out_val.data_ptr(),
                      None if out_idx is None else out_idx.data_ptr(), _stream(q)))


def score_ids(q: torch.Tensor, docs: torch.Tensor, ids: torch.Tensor, idx_offset: int = 0,
              keep: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(q @ docs.T)[b, ids[b] - idx_offset] without the other rows: float32 [B,C], the exact score -- score_topk's fp32 chain,
    bit for bit -- of every listed document, position-aligned with ids (tt_score_ids_f32 / _bf16: one launch that gathers
    B*C rows by id).  q [B,d] or [d] float32; docs [N,d] float32 (d a multiple of 4) or bfloat16 (a multiple of 8), d <= 512;
    ids int64 [B,C] on the documents' device ([C] with a 1-D q).  An entry that is negative, lies outside
    [idx_offset, idx_offset + N) or names a document whose bit in `keep` (pack_keep_mask) is clear scores -inf; a repeated
    id is scored at each of its positions."""
    if q.dim() == 1:
        return score_ids(q.unsqueeze(0), docs, _ids_row(ids), idx_offset, keep)[0]
    q, docs = _front(q, docs)
    ids = _check_ids(ids, q.shape[0], docs.device)
    keep = _check_keep(keep, docs.shape[0], docs.device)
    out = torch.empty(ids.shape, dtype=torch.float32, device=q.device)
    _score_ids_into(q, docs, ids, int(idx_offset), keep, out, None)
    return out


def _unique_pairs(vals: torch.Tensor, idx: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """Rows of (value, id) pairs in which a repeated id -- an identical pair: one document, one score -- is kept once and its
    repeats become (-inf, -1) padding, for the merge above k = 64 (tt_topk_merge_large counts identical pairs as it finds
    them; the k <= 64 merge skips them by itself).  The rows come back sorted by id."""
    si, order = idx.sort(dim=1)
    sv = vals.gather(1, order)
    dup = torch.zeros_like(si, dtype=torch.bool)
    dup[:, 1:] = si[:, 1:] == si[:, :-1]
    return sv.masked_fill_(dup, float("-inf")), si.masked_fill_(dup, -1)


def _merge_candidates(vals: torch.Tensor, idx: torch.Tensor, k: int, out=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """The exact top-k of the distinct candidates of scored rows (vals f32 / idx int64 [B,C] as tt_score_ids_* wrote them),
    (score desc, index asc), tail (-inf, -1): the existing merges, into `out` when given."""
    B, C = vals.shape
    ov, oi = _out_pair(B, k, vals.device, out)
    if C == 0 or B == 0:
        return _pad_pair(ov, oi)
    if k > SMALL_KMAX:
        vals, idx = _unique_pairs(vals, idx)
    with torch.cuda.device(vals.device):
        _lib.check(getattr(_lib.lib(), _merge_fn(k))(vals.data_ptr(), idx.data_ptr(), B, C, k, ov.data_ptr(), oi.data_ptr(),
                                                     _stream(vals)))
    return ov, oi


MMR_CMAX = 128  # tt_mmr_select_*: candidates per query
MMR_KMAX = 128  # ... and picks


def _check_lambda(lambda_) -> float:
    """lambda of the diversified selection: a number in [0, 1] (1 = relevance only, 0 = diversity only); NaN is refused."""
    lam = float(lambda_)
    if not 0.0 <= lam <= 1.0:
        raise ValueError(f"lambda_ must lie in [0, 1], got {lambda_}")
    return lam


def _mmr_fetch_k(k: int, fetch_k: Optional[int]) -> int:
    """How many candidates a diverse_search for k fetches: fetch_k, by default min(128, 4 k); k <= fetch_k <= 128."""
    k = int(k)
    if not 1 <= k <= MMR_KMAX:
        raise ValueError(f"diverse_search answers 1 <= k <= {MMR_KMAX}, got k = {k}")
    fk = min(MMR_CMAX, 4 * k) if fetch_k is None else int(fetch_k)
    if fk > MMR_CMAX:
        raise ValueError(f"diverse_search selects out of at most {MMR_CMAX} candidates, got fetch_k = {fk}")
    if fk < k:
        raise ValueError(f"diverse_search needs fetch_k >= k, got fetch_k = {fk} < k = {k}")
    return fk


def mmr_select(vals: torch.Tensor, idx: torch.Tensor, docs: Optional[torch.Tensor], k: int, lambda_: float = 0.5,
               idx_offset: int = 0, rows: Optional[torch.Tensor] = None, return_pos: bool = False):
    """Maximal-marginal-relevance selection out of per-query candidate lists (tt_mmr_select_f32 / _bf16 / _rows_f32: one
    launch, the rule of include/tt.h, bit-defined): (values f32 [B,k], ids int64 [B,k]) in selection order, and with
    return_pos the picks' positions int32 [B,k] in the list.  vals f32 [B,C] and idx int64 [B,C] are a search's output
    (relevance and GLOBAL id, padding (-inf, -1)); C <= 128, 1 <= k <= 128 (k > C: tail (-inf, -1, -1)).  Step t picks the
    largest lambda_ * rel_c - (1 - lambda_) * max over the picked s of <x_c, x_s>, ties to the lower position; the values
    returned are the relevances.  docs [N,d] float32 or bfloat16 are the rows the ids name (idx - idx_offset); or rows=
    float32 [B,C,d] gives the candidates' rows themselves and docs may be None.  1-D vals / idx ([C], rows [C,d]) are one
    query's.  It composes with the output of any search of this package (tagged, biased, hybrid lists included)."""
    if isinstance(vals, torch.Tensor) and vals.dim() == 1:
        if rows is not None and rows.dim() != 2:
            raise ValueError(f"a single query takes rows [C,d], got {tuple(rows.shape)}")
        out = mmr_select(vals.unsqueeze(0), _ids_row(idx, "idx"), docs, k, lambda_, idx_offset,
                         None if rows is None else rows.unsqueeze(0), return_pos)
        return tuple(t[0] for t in out)
    lam = _check_lambda(lambda_)
    if rows is None and docs is None:
        raise ValueError("mmr_select needs docs or rows=")
    _need_cuda(vals, rows if rows is not None else docs)
    vals = _f32c(vals)
    if vals.dim() != 2:
        raise ValueError(f"vals must be [B,C] ([C] for a single query), got {tuple(vals.shape)}")
    B, C = vals.shape
    idx = _check_ids(idx, B, vals.device, "idx")
    if idx.shape[1] != C:
        raise ValueError(f"vals {tuple(vals.shape)} and idx {tuple(idx.shape)} must be one list per query")
    k = int(k)
    if C > MMR_CMAX or not 1 <= k <= MMR_KMAX:
        raise ValueError(f"mmr_select takes C <= {MMR_CMAX} candidates and 1 <= k <= {MMR_KMAX}, got C = {C}, k = {k}")
    out_v, out_i = _out_pair(B, k, vals.device)
    out_p = torch.empty((B, k), dtype=torch.int32, device=vals.device) if return_pos else None
    pos_ptr = None if out_p is None else out_p.data_ptr()
    L = _lib.lib()
    if rows is not None:
        rows = _f32c(rows)
        if rows.dim() != 3 or tuple(rows.shape[:2]) != (B, C) or rows.device != vals.device:
            raise ValueError(f"rows must be float32 [B,C,d] = [{B},{C},d] on {vals.device}, got {tuple(rows.shape)} on {rows.device}")
        with torch.cuda.device(vals.device):
            _lib.check(L.tt_mmr_select_rows_f32(vals.data_ptr(), idx.data_ptr(), B, C, rows.data_ptr(), rows.shape[2], lam, k,
                                                out_v.data_ptr(), out_i.data_ptr(), pos_ptr, _stream(vals)))
    else:
        docs = _docs_c(docs)
        if docs.dim() != 2 or docs.device != vals.device:
            raise ValueError(f"docs must be [N,d] on {vals.device}, got {tuple(docs.shape)} on {docs.device}")
        fn = L.tt_mmr_select_bf16 if docs.dtype == torch.bfloat16 else L.tt_mmr_select_f32
        with torch.cuda.device(vals.device):
            _lib.check(fn(vals.data_ptr(), idx.data_ptr(), B, C, docs.data_ptr() if docs.shape[0] else None, docs.shape[0],
                          docs.shape[1], int(idx_offset), lam, k, out_v.data_ptr(), out_i.data_ptr(), pos_ptr, _stream(vals)))
    return (out_v, out_i, out_p) if return_pos else (out_v, out_i)


def _owned_rows(docs: torch.Tensor, ids: torch.Tensor, idx_offset: int) -> torch.Tensor:
    """float32 [B,C,d]: row ids[b][c] - idx_offset of docs [N,d] (bf16 widened exactly) where that lies in [0, N), zeros
    elsewhere -- one rank's share of the candidate rows of a sharded diverse_search."""
    N, d = docs.shape
    n = ids - idx_offset
    own = (ids >= 0) & (n >= 0) & (n < N)
    if N == 0:
        return torch.zeros(tuple(ids.shape) + (d,), dtype=torch.float32, device=ids.device)
    rows = docs[torch.where(own, n, torch.zeros_like(n))].to(torch.float32)
    return rows.masked_fill_(~own.unsqueeze(-1), 0.0)


_DIVERSE_DOC = """(values f32 [B,k], ids int64 [B,k]) in SELECTION order: relevant, but not k times the same thing.  It is
        search(q, fetch_k, keep=, exclude=) followed by one launch of the diversified selection (mmr_select: maximal marginal
        relevance over the fetched candidates, lambda_ in [0, 1]: 1 = the plain search's first k, lower = more diverse).
        fetch_k defaults to min(128, 4 k); k <= fetch_k <= 128.  The values are the search's scores of the picks; the tail is
        (-inf, -1) when fewer than k candidates exist."""


COLLAPSE_MMAX = 1024       # entries of a row the collapse filter reads: TT_TOPK_LARGE_KMAX, what every search answers exactly
COLLAPSE_EXACT_KMAX = 512  # k + E of an exact collapsed search: every continuation round then fetches at least 512 new rows


def _check_groups(groups: torch.Tensor, n: int, device) -> torch.Tensor:
    """One group id per row of n documents on `device`, as tt_topk_collapse_table reads it (int64 [n], contiguous)."""
    if not isinstance(groups, torch.Tensor) or groups.dtype != torch.int64:
        raise TypeError(f"groups must be an int64 tensor, got {getattr(groups, 'dtype', type(groups))}")
    if groups.device != device:
        raise ValueError(f"groups on {groups.device} but the documents live on {device}")
    if groups.dim() != 1 or groups.numel() != n:
        raise ValueError(f"groups must hold one id per row, [{n}], got {tuple(groups.shape)}")
    return groups if groups.is_contiguous() else groups.contiguous()


def topk_collapse(vals: torch.Tensor, idx: torch.Tensor, k: int, groups: Optional[torch.Tensor] = None,
                  gids: Optional[torch.Tensor] = None, max_per_group: int = 1, idx_offset: int = 0, out=None):
    """At most max_per_group entries per document group out of sorted lists the caller holds (tt_topk_collapse_table /
    _gids, one launch): vals f32 / idx int64 [B,M] as the searches and merges return them ((score desc, index asc), padding
    at the tail), M <= 1024, 1 <= k <= M -> (vals f32 [B,k], idx int64 [B,k], gids int64 [B,k], info int32 [B,2]).  Walking a
    row, an entry is kept if its group id is negative (ungrouped) or fewer than max_per_group earlier entries of the row
    carry its id; the result is the first k kept entries in input order -- values and indices copied, no arithmetic -- then
    (-inf, -1, -1).  info[b] = (kept, complete): complete = 1 when k entries were kept or the row ends in padding, else the
    result is the exact prefix of the answer and a longer row completes it.  Pass exactly one of groups= (int64 [N]: the
    group of entry idx is groups[idx - idx_offset], ungrouped outside the table) and gids= (int64 [B,M], one id per entry).
    1-D vals / idx ([M], gids [M]) are one query's.  out: optional (vals, idx, gids, info) to write into."""
    if (groups is None) == (gids is None):
        raise ValueError("topk_collapse takes exactly one of groups= (a table over the rows) and gids= (one id per entry)")
    if isinstance(vals, torch.Tensor) and vals.dim() == 1:
        res = topk_collapse(vals.unsqueeze(0), _ids_row(idx, "idx"), k, groups, _ids_row(gids, "gids"), max_per_group, idx_offset)
        return tuple(t[0] for t in res)
    src = groups if gids is None else gids
    _need_cuda(vals, idx, src)
    vals = _f32c(vals)
    if idx.dtype != torch.int64 or vals.shape != idx.shape or vals.dim() != 2 or idx.device != vals.device:
        raise ValueError("topk_collapse wants vals f32 [B,M] and idx int64 [B,M] on one device")
    idx = idx.contiguous()
    B, M = vals.shape
    k, m = int(k), int(max_per_group)
    if src.dtype != torch.int64 or src.device != vals.device:
        raise ValueError(f"topk_collapse wants int64 group ids on {vals.device}, got {src.dtype} on {src.device}")
    if gids is not None and tuple(gids.shape) != (B, M):
        raise ValueError(f"gids must be [B,M] = [{B},{M}] (one id per entry), got {tuple(gids.shape)}")
    if groups is not None and groups.dim() != 1:
        raise ValueError(f"groups must be [N] (one id per row of the index), got {tuple(groups.shape)}")
    src = src.contiguous()
    dev = vals.device
    if out is None:
        out = (*_out_pair(B, k, dev), torch.empty((B, k), dtype=torch.int64, device=dev),
               torch.empty((B, 2), dtype=torch.int32, device=dev))
    ov, oi, og, info = out
    L = _lib.lib()
    with torch.cuda.device(dev):
        if gids is None:
            _lib.check(L.tt_topk_collapse_table(vals.data_ptr(), idx.data_ptr(), B, M, src.data_ptr() if src.numel() else None,
                                                src.numel(), int(idx_offset), m, k, ov.data_ptr(), oi.data_ptr(), og.data_ptr(),
                                                info.data_ptr(), _stream(vals)))
        else:
            _lib.check(L.tt_topk_collapse_gids(vals.data_ptr(), idx.data_ptr(), src.data_ptr(), B, M, m, k, ov.data_ptr(),
                                               oi.data_ptr(), og.data_ptr(), info.data_ptr(), _stream(vals)))
    return ov, oi, og, info


def _collapse_fetch_k(k: int, ntotal: Optional[int] = None, fetch_k: Optional[int] = None, E: int = 0) -> int:
    """How many rows round 0 of a collapsed search for k fetches: fetch_k, by default min(ntotal, max(k, min(64, 4 k))) up to
    k = 64 -- the inner search stays at or below the k = 64 routing cliff -- and min(ntotal, 1024, 2 k) above (the default
    also gives way to an exclusion list: at most 1024 - E).  ValueError: k < 1, fetch_k < k, fetch_k + E > 1024."""
    k = int(k)
    if k < 1:
        raise ValueError(f"collapsed_search: k = {k} < 1")
    if fetch_k is None:
        fk = max(k, min(SMALL_KMAX, 4 * k)) if k <= SMALL_KMAX else min(COLLAPSE_MMAX, 2 * k)
        fk = max(k, min(fk, COLLAPSE_MMAX - E))
        if ntotal is not None:
            fk = min(fk, max(int(ntotal), 1))
    else:
        fk = int(fetch_k)
        if fk < k:
            raise ValueError(f"collapsed_search needs fetch_k >= k, got fetch_k = {fk} < k = {k}")
    if fk + E > COLLAPSE_MMAX:
        raise ValueError(f"collapsed_search: fetch_k + E = {fk} + {E} = {fk + E} > {COLLAPSE_MMAX}")
    return fk


def _collapse_rounds(search_fn: Callable, collapse_fn: Callable, mask_fn: Callable, max_per_group: int, fetch_k: int, E: int,
                     ntotal: Optional[int], exact: bool, stats: Optional[dict] = None):
    """The rounds of a collapsed search, over callables, on whatever device their tensors live (the tests run it on the host):
      search_fn(rows, kk, keep) -> (vals [R,kk], idx [R,kk]): the exact top-kk of the eligible documents for the queries
        `rows` (an int64 tensor of query numbers; None = all of them) under the per-call mask `keep` (None = the caller's own);
      collapse_fn(vals, idx) -> (vals [R,k], idx [R,k], gids [R,k], info [R,2]): the filter (topk_collapse) for the final k;
      mask_fn(saturated, selected) -> keep: the caller's mask without the rows of the group ids `saturated` and the ids `selected`.
    Round 0 searches every query for fetch_k; exact=False returns it.  Round 1 searches the incomplete queries, as one batch,
    for 1024 - E.  After that every still incomplete query runs alone: with j entries selected, it searches for 1024 - E - j rows
    under a mask without its saturated groups (max_per_group entries selected) and its selected rows, and filters [selected ;
    new rows] -- a sorted row, every new row follows the old list -- until the filter reports complete.  A round that does not
    finish dropped a row, whose group is then saturated: the saturated groups grow every round, so the loop ends.  Reading
    `complete` SYNCHRONISES with the host once per round.  ntotal: the number of rows when the caller knows it (a search for all
    of them is complete whatever its tail).  stats: optional dict, receives batched_rounds / masked_rounds.
    Returns (vals [B,k], idx [B,k], gids [B,k], complete int32 [B])."""
    width = COLLAPSE_MMAX - E
    whole = (lambda kk: ntotal is not None and kk >= ntotal)
    counts = {"batched_rounds": 1, "masked_rounds": 0}
    ov, oi, og, info = collapse_fn(*search_fn(None, fetch_k, None))
    complete = info[:, 1].clone()
    if whole(fetch_k):
        complete.fill_(1)
    if exact:
        todo = torch.nonzero(complete == 0).flatten()  # (the host reads it: one synchronisation per round)
        if todo.numel() and width > fetch_k:
            counts["batched_rounds"] += 1
            rv, ri, rg, rinfo = collapse_fn(*search_fn(todo, width, None))
            ov[todo], oi[todo], og[todo], info[todo] = rv, ri, rg, rinfo
            done = rinfo[:, 1] != 0 if not whole(width) else torch.ones_like(rinfo[:, 1], dtype=torch.bool)
            complete[todo] = done.to(complete.dtype)
            todo = todo[~done]
        for b in todo.tolist():
            while True:
                j = int(info[b, 0])
                g = og[b, :j]
                uniq, cnt = torch.unique(g[g >= 0], return_counts=True)
                kk = width - j
                nv, ni = search_fn(todo.new_tensor([b]), kk, mask_fn(uniq[cnt >= max_per_group], oi[b, :j]))
                counts["masked_rounds"] += 1
                rv, ri, rg, rinfo = collapse_fn(torch.cat([ov[b:b + 1, :j], nv], 1), torch.cat([oi[b:b + 1, :j], ni], 1))
                ov[b], oi[b], og[b], info[b] = rv[0], ri[0], rg[0], rinfo[0]
                if whole(kk) or int(rinfo[0, 1]):
                    complete[b] = 1
                    break
    if stats is not None:
        stats.update(counts)
    return ov, oi, og, complete


def _owned_gids(groups: torch.Tensor, ids: torch.Tensor, idx_offset: int) -> torch.Tensor:
    """int64 like ids: groups[ids - idx_offset] where that lies in the table, zeros elsewhere -- one rank's share of the group
    ids of a sharded collapsed search (the shares add up to the ids: exactly one rank owns a row)."""
    N = groups.numel()
    n = ids - idx_offset
    own = (ids >= 0) & (n >= 0) & (n < N)
    if N == 0:
        return torch.zeros_like(ids)
    return groups[torch.where(own, n, torch.zeros_like(n))].masked_fill_(~own, 0)


def _collapsed_search(index, q: torch.Tensor, k: int, max_per_group: int, fetch_k: Optional[int], keep, exclude, exact: bool,
                      groups: Optional[torch.Tensor], n_rows: int, idx_offset: int, device, ntotal: Optional[int], gid_fn=None):
    """collapsed_search of the three indexes: index.search is the inner search, groups the group table over the n_rows rows
    this index (this rank) holds, numbered from idx_offset.  gid_fn(idx) -> the entries' group ids where the table does not
    cover the result (ShardedIndex); None = look them up in the table."""
    if groups is None:
        raise ValueError("collapsed_search: this index has no groups (set_groups)")
    if q.dim() == 1:
        res = _collapsed_search(index, q.unsqueeze(0), k, max_per_group, fetch_k, keep, _exclude_row(exclude), exact, groups, n_rows,
                                idx_offset, device, ntotal, gid_fn)
        return tuple(t[0] for t in res)
    _need_cuda(q)
    k, m = int(k), int(max_per_group)
    if m < 1:
        raise ValueError(f"collapsed_search: max_per_group = {m} < 1")
    E = 0
    if exclude is not None:
        exclude, _ = _check_exclude(exclude, q.shape[0], 1, device)
        E = exclude.shape[1]
    fk = _collapse_fetch_k(k, ntotal, fetch_k, E)
    if exact and k + E > COLLAPSE_EXACT_KMAX:
        raise ValueError(f"an exact collapsed search answers k + E <= {COLLAPSE_EXACT_KMAX}, got {k} + {E} (exact=False has no such bound)")

    def search_fn(rows, kk, keep_r):
        return index.search(q if rows is None else q[rows], kk, keep=keep if keep_r is None else keep_r,
                            exclude=exclude if exclude is None or rows is None else exclude[rows])

    def collapse_fn(v, i):
        if v.shape[1] < k:  # (fewer rows than k were asked for: a corpus smaller than k)
            pad = k - v.shape[1]
            v = torch.cat([v, v.new_full((v.shape[0], pad), float("-inf"))], 1)
            i = torch.cat([i, i.new_full((i.shape[0], pad), -1)], 1)
        if gid_fn is not None:
            return topk_collapse(v, i, k, gids=gid_fn(i), max_per_group=m)
        return topk_collapse(v, i, k, groups=groups, max_per_group=m, idx_offset=idx_offset)

    def mask_fn(saturated, selected):
        keep_r = pack_keep_mask(~torch.isin(groups, saturated))
        if keep is not None:
            keep_r &= _check_keep(keep, n_rows, device)
        return _clear_ids(keep_r, n_rows, device, selected, idx_offset)

    stats = {}
    res = _collapse_rounds(search_fn, collapse_fn, mask_fn, m, fk, E, ntotal, exact, stats)
    index.collapse_rounds = (stats["batched_rounds"], stats["masked_rounds"])
    return res


_COLLAPSED_DOC = """(values f32 [B,k], ids int64 [B,k], group ids int64 [B,k], complete int32 [B]): the best k rows with at most
        max_per_group rows per document group (set_groups; a negative group id = ungrouped, never collapsed) -- field collapsing.
        The eligible rows (not removed, kept by keep=, not in exclude=) in (score desc, index asc) order are walked, a row is
        kept if it is ungrouped or fewer than max_per_group rows of its group were kept before it, and the result is the
        first k kept rows, tail (-inf, -1, -1).  Values and ids are the search's own, copied.  It is search(q, fetch_k, keep=,
        exclude=) followed by one filter launch (topk_collapse).  fetch_k defaults to min(ntotal, max(k, min(64, 4 k))) up to
        k = 64 and to min(ntotal, 1024, 2 k) above; fetch_k + E <= 1024.
        exact=False returns that one round and does NOT synchronise with the host: complete[b] = 1 says the row is the answer
        (k rows kept, or the fetch saw every eligible row), 0 that it is an exact PREFIX of it (a group owned the head of the
        list; values beyond `kept` are the tail).  exact=True (the default) goes on by rounds until every query is complete,
        and SYNCHRONISES with the host once per round: the incomplete queries once more as a batch for 1024 - E rows, then
        each still incomplete query alone under a keep-bitmask without its saturated groups and selected rows (torch.isin
        over the group table: a pass over N ids per round).  It needs k + E <= 512.  collapse_rounds afterwards holds
        (batched rounds, masked rounds) of the most recent call."""


SCREEN_MIN_BATCH = 1     # the screened path wins at every batch size once the corpus is large enough to sample:
                         # B <= 64 streaming form (half the bytes of the fp32 kernel), above it the shared-tile form
SCREEN_PADDED_MIN_BATCH = 33  # d < 256 (zero-padded screen copy): only where the exact kernel is MFMA-bound
SCREEN_MIN_DOCS = 65536  # below this there is no sample pass to seed thresholds and the exact kernel is faster


def _fp16_range_ok(dmax: float, amax: float) -> bool:
    """Whether a corpus with largest row norm dmax and largest |element| amax can be screened in fp16 (NaN: no)."""
    return dmax == dmax and amax < 6.0e4 and dmax < 6.0e4


class _Screen:
    """The screened half of a corpus layout, as the screened entry points (_screened_fn) read it: `rows` [N,256] is what the
    finish pass rescores, `filt` [N,256] what the screen reads.  fp32: rows are the fp32 matrix (a zero-padded copy when
    d < 256) and filt its fp16 shadow; bf16: both are the bf16 matrix, screened as it is."""

    def __init__(self, rows: torch.Tensor, filt: torch.Tensor, bf16: bool, dmax_norm: float):
        self.rows, self.filt, self.bf16, self.dmax_norm = rows, filt, bool(bf16), float(dmax_norm)
        self.n = rows.shape[0]

    @classmethod
    def for_f32(cls, docs: torch.Tensor) -> Optional["_Screen"]:
        """fp32 rows + fp16 shadow (N*512 bytes), or None: d does not qualify, or the corpus is outside the fp16 range."""
        N, d = docs.shape
        if not (d == 256 or (d < 256 and d % 4 == 0)):
            return None
        rows = docs
        if d < 256:
            # narrower embeddings (HIDDEN_DIM 64, 128, ...): zero-padded to the screen kernels' 256 features.  Padding adds
            # fmaf(0, 0, acc) terms to the fp32 chain, which leave every score bit-identical; the padded copy costs N KiB and is
            # used for batches above 32 queries (MFMA-bound), smaller batches stream the original rows through the exact
            # kernel, which already moves only N*d*4 bytes.
            rows = torch.zeros((N, 256), dtype=torch.float32, device=docs.device)
            rows[:, :d] = docs
        filt = torch.empty((N, 256), dtype=torch.float16, device=docs.device)
        stats = torch.zeros(2, dtype=torch.float32, device=docs.device)
        with torch.cuda.device(docs.device):
            _lib.check(_lib.lib().tt_index_build_f16(rows.data_ptr(), N, 256, filt.data_ptr(), stats.data_ptr(), _stream(docs)))
        dmax, amax = (float(x) for x in stats.tolist())  # one sync, at index-build time
        return cls(rows, filt, False, dmax) if _fp16_range_ok(dmax, amax) else None

    @classmethod
    def for_bf16(cls, docs: torch.Tensor) -> Optional["_Screen"]:
        """bf16 rows screened as they are (one statistics pass, no copy), or None with a warning: d != 256, or out of range."""
        N, d = docs.shape
        if d == 256:
            stats = torch.zeros(2, dtype=torch.float32, device=docs.device)
            with torch.cuda.device(docs.device):
                _lib.check(_lib.lib().tt_index_stats_bf16(docs.data_ptr(), N, d, stats.data_ptr(), 1, _stream(docs)))
            dmax, amax = (float(x) for x in stats.tolist())  # one sync, at index-build time
            if _fp16_range_ok(dmax, amax):
                return cls(docs, docs, True, dmax)
        import warnings
        warnings.warn(f"BruteForceIndex: a bf16 [{N},{d}] corpus is screened only at d = 256 within the fp16 range; "
                      "this index runs the exact bf16 kernel", RuntimeWarning, stacklevel=3)  # BruteForceIndex(...)'s caller
        return None

    def workspace_bytes(self, B: int, k: int, masked: bool = False) -> int:
        if masked:
            return _lib.lib().tt_score_topk_screened_masked_workspace_bytes(B, self.n, 256, k, int(self.bf16))
        name = "tt_score_topk_screened_bf16_workspace_bytes" if self.bf16 else "tt_score_topk_screened_workspace_bytes"
        return getattr(_lib.lib(), name)(B, self.n, 256, k)

    def seed_list(self, q: torch.Tensor, k: int, ks: int, flags: torch.Tensor, ws: torch.Tensor,
                  keep: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Query image + sample pass of a search of q [B,256] for k: [B,ks] f32, each query's ks largest sample maxima (with
        `keep`, a checked keep-bitmask over the rows: the maxima of the kept documents, the masked entry point)."""
        B, d = q.shape
        lst = torch.empty((B, ks), dtype=torch.float32, device=q.device)
        fn = getattr(_lib.lib(), _screened_fn("seed_list", self.bf16, keep is not None))
        mask = () if keep is None else (keep.data_ptr(),)
        _lib.check(fn(q.data_ptr(), B, d, self.filt.data_ptr(), self.n, *mask, k, ks, self.dmax_norm, flags.data_ptr(),
                      lst.data_ptr(), ws.data_ptr(), ws.numel(), _stream(q)))
        return lst

    def run(self, q: torch.Tensor, k: int, idx_offset: int, vals: torch.Tensor, idx: torch.Tensor, flags: torch.Tensor,
            ws: torch.Tensor, seed: Optional[torch.Tensor] = None, prof_events=None, keep: Optional[torch.Tensor] = None) -> None:
        """The screened search of q [B,256] into (vals, idx); with `seed` [B] f32, what follows seed_list() on the same ws;
        with `keep` (a checked keep-bitmask over the rows), the masked entry point of the same phase."""
        B, d = q.shape
        fn = getattr(_lib.lib(), _screened_fn("whole" if seed is None else "seeded", self.bf16, keep is not None))
        corpus = (self.rows.data_ptr(),) if self.bf16 else (self.rows.data_ptr(), self.filt.data_ptr())
        mask = () if keep is None else (keep.data_ptr(),)
        thr = () if seed is None else (seed.data_ptr(),)
        _lib.check(fn(q.data_ptr(), B, d, *corpus, self.n, *mask, k, self.dmax_norm, idx_offset, vals.data_ptr(),
                      idx.data_ptr(), flags.data_ptr(), *thr, ws.data_ptr(), ws.numel(), prof_events, _stream(q)))


class BruteForceIndex(_CursorSearch):
    """A [N,d] fp32 document matrix resident in HBM (document_embeddings.npy layout, backend/main.py:125-138: row i <->
    documents[i]) with exact top-k search.

    screen=True additionally keeps an fp16 shadow copy (N*d*2 bytes) so that large query batches run the screened path (fp16
    MFMA filter + exact fp32 rescoring, tt_score_topk_screened_f32 and its kin: _Screen): same bit-exact result, an order
    of magnitude more queries/s than the fp32-MFMA-bound kernel.

    A bfloat16 [N,d] matrix (d in {64, 128, 192, 256}) is kept as it is: `docs` is the caller's tensor (no copy, N*d*2
    bytes, no shadow).  screen=True at d = 256 runs one statistics pass (tt_index_stats_bf16) and screens straight from the
    bf16 rows (converted to fp16 in LDS); otherwise, and outside the fp16 range, searches run the exact kernel over the bf16
    rows (tt_score_topk_bf16).  Either way the result is that of the widened fp32 rows, bit for bit.

    Deletions and filtered search: remove_ids(ids) withdraws documents for good (a persistent keep-bitmask, N/8 bytes,
    allocated on first use and mutated in place), search(q, k, keep=mask) answers over a subset for one call
    (pack_keep_mask; ANDed with the persistent mask).  By default a search under any mask runs the masked exact kernel
    (tt_score_topk_masked_f32 / _bf16), also on a screen=True index, at the exact kernel's cost -- HBM-bound at small B,
    fp32-MFMA-bound at large B, as the k > 64 route already is.  screen_masked=True (with screen=True) keeps masked searches
    on the screened path: the screen kernels' MASKED instantiations take the keep-bitmask (tt_score_topk_screened_masked_f32
    and its kin; every threshold is formed from kept documents only, DESIGN.md "Masked screened top-k"), the result is the
    masked exact kernel's bit for bit, and fallback_flags / search_stats() report the screen's own values.  It is opt-in:
    without it nothing changes.  k > 64 runs the exact route either way, and a masked document is still streamed and
    multiplied: a selective mask pays the full scan.

    Callers, streams and threads: every search of one index may be in flight on any number of streams and host threads at
    once; each call takes its workspace, flags and outputs per call (the caching allocator's blocks of the caller's stream)
    and orders nothing against another call.  All of them are asynchronous to the host except collapsed_search(exact=True),
    which reads its `complete` flags once per round.  fallback_flags, collapse_rounds and keep_stats / search_stats() name
    "the most recent call": diagnostics of one caller at a time, not to be read while another thread searches.  remove_ids
    and set_tags / set_bias / set_groups are the one mutating caller's: launches on its stream, ordered against searches
    by that caller.
    """

    def __init__(self, doc_embeddings: torch.Tensor, idx_offset: int = 0, screen: bool = False, screen_masked: bool = False):
        # (screen may also be a ready _Screen over doc_embeddings: _from_buffers)
        _need_cuda(doc_embeddings)
        self.docs = _docs_c(doc_embeddings)
        self.idx_offset = int(idx_offset)
        if not isinstance(screen, _Screen):
            build = _Screen.for_bf16 if self.docs.dtype == torch.bfloat16 else _Screen.for_f32
            screen = build(self.docs) if screen and self.docs.shape[0] > 0 else None
        self._screen: Optional[_Screen] = screen
        self.screen_masked = bool(screen_masked)  # masked searches stay on the screened path (where an unmasked one screens)
        # for callers to read: the fp16 shadow [N,256] (None for screened bf16 rows) and the largest row norm
        self.docs16 = screen.filt if screen is not None and not screen.bf16 else None
        self.dmax_norm = screen.dmax_norm if screen is not None else float("nan")
        self.fallback_flags = torch.zeros(1, dtype=torch.int32, device=self.docs.device)  # per 32-query tile
        self.keep_stats = False   # True: the most recent screened search's workspace is kept for search_stats()
        self._last_ws = None
        self._keep: Optional[torch.Tensor] = None  # the persistent keep-bitmask (remove_ids), None until the first removal
        self._tags: Optional[torch.Tensor] = None  # one 32-bit tag per row, padded to whole tiles (set_tags), for tagged_search
        self._bias: Optional[torch.Tensor] = None  # one float per row, padded to whole tiles (set_bias), for biased_search
        self._groups: Optional[torch.Tensor] = None  # one int64 group id per row (set_groups), for collapsed_search
        self.collapse_rounds = (0, 0)  # (batched, masked) rounds of the most recent collapsed_search

    @classmethod
    def _from_buffers(cls, docs32: torch.Tensor, docs16: Optional[torch.Tensor], dmax_norm: float, idx_offset: int,
                      screen_masked: bool = False):
        """An index over caller-managed device buffers (StreamedIndex's per-block view)."""
        return cls(docs32, idx_offset, _Screen(docs32, docs16, False, dmax_norm) if docs16 is not None else False,
                   screen_masked=screen_masked)

    @property
    def _screen_bf16(self) -> bool:  # bf16 rows screened as they are (no docs16)
        return self._screen is not None and self._screen.bf16

    @property
    def ntotal(self) -> int:
        return self.docs.shape[0]

    @property
    def device(self) -> torch.device:
        return self.docs.device

    @property
    def keep_mask(self) -> Optional[torch.Tensor]:
        """The persistent keep-bitmask (int32 [ceil(N/32)], bit n = document n not removed), or None: nothing removed yet."""
        return self._keep

    def remove_ids(self, ids) -> None:
        """Withdraw documents: `ids` are GLOBAL ids (with this index's idx_offset; a tensor or a sequence), and ids that are
        not this index's are ignored.  The mask is allocated all-ones on first use and then mutated in place with one launch on
        the current stream, so later removals are seen by everything that holds it (a captured GraphedSearch included)."""
        self._keep = _clear_ids(self._keep, self.docs.shape[0], self.docs.device, ids, self.idx_offset)

    def search_stats(self) -> Optional[torch.Tensor]:
        """int32 [B,2] = (pooled candidates, survivors rescored exactly) per query of the most recent screened search made
        with keep_stats = True, or None.  Diagnostic: what the fp16 filter let through on this corpus."""
        if self._last_ws is None:
            return None
        ws, B, k = self._last_ws
        with torch.cuda.device(self.docs.device):
            off = _lib.lib().tt_score_topk_screened_stats_offset(B, self.docs.shape[0], 256, k)
        return ws[off:off + 8 * B].view(torch.int32).view(B, 2).clone()

    def _check_q(self, q: torch.Tensor, width: bool = True) -> None:
        """The queries of every search of this index: on the GPU, on the rows' device, of their width (width=False: the
        caller's own pass checks it, behind the dtype)."""
        _need_cuda(q)
        if q.device != self.docs.device:
            raise ValueError(f"queries on {q.device} but the index lives on {self.docs.device}")
        if width and q.shape[-1] != self.docs.shape[1]:
            raise ValueError(f"shape mismatch: q {tuple(q.shape)} vs docs {tuple(self.docs.shape)}")

    def _mask(self, keep: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
        """The mask a call runs under: the persistent one ANDed with the call's checked `keep`, or None."""
        return _and_keep(self._keep, keep, self.docs.shape[0], self.docs.device)

    def _exact_took_over(self, B: int) -> None:
        """fallback_flags after a search of B queries that ran the exact kernel whatever the layout: on a screened index
        every 32-query tile reads "the exact kernel took over"."""
        if self._screen is not None:
            self.fallback_flags = torch.ones((B + 31) // 32, dtype=torch.int32, device=self.docs.device)

    def search(self, q: torch.Tensor, k: int = 10, _prof_events=None, out=None, _seed_union=None,
               _k_seed: int = 0, _k_list: int = 0, keep: Optional[torch.Tensor] = None,
               exclude: Optional[torch.Tensor] = None, candidates: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """out: optional (vals f32 [B,k], idx int64 [B,k]) contiguous device tensors to write into (2-D q only).
        candidates: optional per-query candidate lists, int64 [B,C] on the index's device ([C] with a 1-D q): GLOBAL ids (with
        idx_offset).  The search then reads those rows only: tt_score_ids_f32 / _bf16 into scratch [B,C] pairs, then the
        existing merge into `out` -- the exact top-k of the distinct, present (not removed, kept by keep=) candidates,
        (score desc, index asc), tail (-inf, -1) when fewer than k are left (k > C is fine).  Negative ids and ids that are
        not this index's are padding, a repeated id counts once.  It never screens and leaves fallback_flags as they were;
        exclude= composes (the candidate search runs for k + E).
        exclude: optional per-query exclusion lists, int64 [B,E] on the index's device ([E] with a 1-D q): GLOBAL ids (with
        idx_offset) query b must not return; negative entries are padding, duplicates and ids of other indexes are fine.  The
        search is this index's ordinary search for k + E into a scratch pair -- every routing decision sees k + E: it screens
        up to k + E = 64 and takes the exact large-k route above, fallback_flags are that search's, k + E > 1024 raises
        ValueError -- followed by one filter launch (tt_topk_exclude_ids).  The result is the exact top-k of the documents
        that are not listed, in the usual order, tail (-inf, -1); keep= and remove_ids compose with it.
        keep: optional packed keep-bitmask over this index's rows for this call (pack_keep_mask), ANDed with the persistent
        mask of remove_ids.  With either in effect the search is the masked exact kernel's, also on a screen=True index (the
        class docstring has the cost); fallback_flags then reads all ones.  On a screen_masked=True index it is the masked
        screened search wherever the unmasked one would screen, and fallback_flags are the screen's.
        _seed_union (ShardedIndex): a callable that turns this shard's seed list [B, _k_seed] f32 (its _k_seed largest
        sample maxima per query, _Screen.seed_list) into the seed thresholds [B] f32 -- the _k_seed-th largest of the UNION
        of the ranks' lists (one all-gather + tt_seed_union_f32) -- on the current stream; the screen then runs with that
        global seed and `out` holds this shard's documents above it."""
        if q.dim() == 1:  # single query (QueryInferencer / hybrid rerank)
            return _squeezed(self.search, q, k, _prof_events, None, None, 0, 0, keep, _exclude_row(exclude),
                             _ids_row(candidates, "candidates"))
        self._check_q(q)
        if exclude is not None:
            exclude, kk = _check_exclude(exclude, q.shape[0], k, self.docs.device)
            v, i = self.search(q, kk, _prof_events, None, _seed_union, _k_seed, _k_list, keep, None, candidates)
            return topk_exclude(v, i, exclude, k, out)
        keep = self._mask(keep)
        if candidates is not None:
            return _merge_candidates(*self._score_ids(q, candidates, keep, True, "candidates"), k, out)
        if self._screens(q.shape[0], k, keep is not None):
            return self._search_screened(q, k, _prof_events, out, _seed_union, _k_seed, _k_list, keep)
        if keep is not None:
            self._exact_took_over(q.shape[0])
        return _copied(out, *score_topk(q, self.docs, k, self.idx_offset, keep=keep))

    @property
    def tags(self) -> Optional[torch.Tensor]:
        """The rows' tags as the tagged kernels read them (int32 [32*ceil(N/32)], zero padding beyond N), or None: not set."""
        return self._tags

    def set_tags(self, tags: torch.Tensor) -> None:
        """One 32-bit tag per row (int32 [N], or already padded to [32*ceil(N/32)]; the bits are read as unsigned), on the
        index's device: a tenant / language / collection id, or several packed bit-fields.  Kept padded (4 bytes per row)."""
        self._tags = _check_tags(tags, self.docs.shape[0], self.docs.device)

    def tagged_search(self, q: torch.Tensor, k: int = 10, match_mask=0xffffffff, match_value=0,
                      keep: Optional[torch.Tensor] = None, out=None) -> Tuple[torch.Tensor, torch.Tensor]:
        """search() with a filter per query, in ONE pass over the rows: query b sees row n iff
        (tags[n] & match_mask[b]) == match_value[b] (score_topk_tagged; match_mask / match_value: int32 [B] device tensors or
        Python ints for every query; q [B,d] or a single [d]).  keep= and remove_ids compose: the row's bit in the ANDed mask
        must be set as well.  Always the exact kernel in its tagged mode (k <= 64), also on a screen=True index, whose
        fallback_flags then read all ones as after search(keep=).  exclude= and candidates= are not taken.
        ValueError: no tags (set_tags), or k > 64."""
        if self._tags is None:
            raise ValueError("tagged_search: this index has no tags (set_tags)")
        if q.dim() == 1:
            return _squeezed(self.tagged_search, q, k, match_mask, match_value, keep)
        self._check_q(q)
        B = q.shape[0]
        mm = _match_words(match_mask, B, self.docs.device, "match_mask")
        mv = _match_words(match_value, B, self.docs.device, "match_value")
        return self._mode_search(_TAGGED, q, (self._tags, mm, mv), keep, k, out)

    @property
    def bias(self) -> Optional[torch.Tensor]:
        """The rows' biases as the biased kernels read them (float32 [32*ceil(N/32)], zero padding beyond N), or None: not set."""
        return self._bias

    def set_bias(self, bias: Optional[torch.Tensor]) -> None:
        """One float32 bias per row (float32 [N], or already padded to [32*ceil(N/32)]), on the index's device: a prior, a boost
        or a demotion added to every score by biased_search; l2_bias(docs) for Euclidean neighbours.  Kept padded (4 bytes per
        row).  Checked once here: a NaN or an infinity among the N values raises ValueError (a host synchronisation).
        None clears it."""
        self._bias = _set_bias(bias, self.docs.shape[0], self.docs.device)

    def biased_search(self, q: torch.Tensor, k: int = 10, keep: Optional[torch.Tensor] = None,
                      exclude: Optional[torch.Tensor] = None, out=None, candidates=None) -> Tuple[torch.Tensor, torch.Tensor]:
        """search() ranked by q.d + bias[n] (score_topk_biased; q [B,d] or a single [d]); the values returned are the biased
        scores.  keep= and remove_ids compose as in tagged_search.  exclude= (int64 [B,E]; [E] with a 1-D q) takes search()'s
        route: a biased search for k + E, then the filter (tt_topk_exclude_ids); the bound here is k + E <= 64.  Always the
        exact kernel in its biased mode, also on a screen=True index, whose fallback_flags then read all ones as after
        search(keep=).  Not taken: tags (tagged_search ignores the bias, this search the tags), a count / range_search, k > 64.
        ValueError: no bias (set_bias), k (+ E) > 64, or candidates= (named only to be refused: tt_score_ids_* adds no bias)."""
        if self._bias is None:
            raise ValueError("biased_search: this index has no bias (set_bias)")
        if candidates is not None:
            raise ValueError("biased_search takes no candidates=: the candidate scores (score_ids) carry no bias")
        if q.dim() == 1:
            return _squeezed(self.biased_search, q, k, keep, _exclude_row(exclude))
        self._check_q(q)
        if exclude is not None:
            exclude, kk = _check_exclude(exclude, q.shape[0], k, self.docs.device)
            if kk > BIASED_KMAX:
                raise ValueError(f"a biased search with an exclusion list runs for k + E = {kk} > {BIASED_KMAX}")
            v, i = self.biased_search(q, kk, keep)
            return topk_exclude(v, i, exclude, k, out)
        return self._mode_search(_BIASED, q, (self._bias,), keep, k, out)

    def _mode_search(self, mode: _Mode, q: torch.Tensor, own: tuple, keep: Optional[torch.Tensor], k: int, out):
        """A checked q [B,d] through one mode of the exact kernel (_mode_into) over the rows, under the ANDed mask."""
        keep = self._mask(keep)
        res = _mode_into(mode, _f32c(q), self.docs, own, keep, k, self.idx_offset, out)
        self._exact_took_over(q.shape[0])
        return res

    def _cursor_device(self) -> torch.device:
        return self.docs.device

    def _search_after(self, q: torch.Tensor, k: int, av: torch.Tensor, ai: torch.Tensor, keep: Optional[torch.Tensor], out=None):
        """search_after (_CursorSearch) of q [B,d] under a checked cursor: the exact kernel in its cursor mode over the rows."""
        self._check_q(q)
        return self._mode_search(_AFTER, q, (av, ai), keep, k, out)

    def _score_ids(self, q: torch.Tensor, ids: torch.Tensor, keep: Optional[torch.Tensor], want_idx: bool, what: str = "ids"):
        """tt_score_ids_* of q [B,d] over this index's rows under the ANDed mask `keep` (checked) or None: (scores f32 [B,C],
        global ids int64 [B,C] with -1 where the entry yields nothing -- None unless want_idx)."""
        q = _f32c(q)
        ids = _check_ids(ids, q.shape[0], self.docs.device, what)
        vals = torch.empty(ids.shape, dtype=torch.float32, device=q.device)
        idx = torch.empty_like(ids) if want_idx else None
        _score_ids_into(q, self.docs, ids, self.idx_offset, keep, vals, idx)
        return vals, idx

    def score_ids(self, q: torch.Tensor, ids: torch.Tensor, keep: Optional[torch.Tensor] = None) -> torch.Tensor:
        """float32 [B,C] ([C] for a single query): the exact dense score -- the value search() returns for the document, bit
        for bit -- of every id of ids int64 [B,C] (GLOBAL ids, with idx_offset), position-aligned.  -inf where the id is
        negative, not this index's, removed (remove_ids) or not kept by `keep`.  One launch that gathers B*C rows."""
        if q.dim() == 1:
            return self.score_ids(q.unsqueeze(0), _ids_row(ids), keep)[0]
        self._check_q(q)
        return self._score_ids(q, ids, self._mask(keep), False)[0]

    def diverse_search(self, q: torch.Tensor, k: int = 10, lambda_: float = 0.5, fetch_k: Optional[int] = None,
                       keep: Optional[torch.Tensor] = None, exclude: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        if q.dim() == 1:
            return _squeezed(self.diverse_search, q, k, lambda_, fetch_k, keep, _exclude_row(exclude))
        fk, lam = _mmr_fetch_k(k, fetch_k), _check_lambda(lambda_)
        v, i = self.search(q, fk, keep=keep, exclude=exclude)
        return mmr_select(v, i, self.docs, k, lam, self.idx_offset)

    def _candidate_rows(self, ids: torch.Tensor) -> torch.Tensor:
        """float32 [B,C,d]: the rows of the global ids this index owns, zeros elsewhere (ShardedIndex.diverse_search)."""
        return _owned_rows(self.docs, ids, self.idx_offset)

    diverse_search.__doc__ = _DIVERSE_DOC + """
        The candidates' rows are gathered from this index's own rows (fp32, or bf16 widened exactly) by the kernel, whichever
        layout searched: the screened and the exact route return the same list, so the result does not depend on it."""

    @property
    def groups(self) -> Optional[torch.Tensor]:
        """The rows' document-group ids (int64 [N]; negative = ungrouped), or None: not set."""
        return self._groups

    def set_groups(self, groups: Optional[torch.Tensor]) -> None:
        """One int64 group id per row (int64 [N] on the index's device): the page a passage came from, the thread of a message.
        A negative id means ungrouped: such a row is never collapsed.  Kept as given (8 bytes per row).  None clears it."""
        self._groups = None if groups is None else _check_groups(groups, self.docs.shape[0], self.docs.device)

    def collapsed_search(self, q: torch.Tensor, k: int = 10, max_per_group: int = 1, fetch_k: Optional[int] = None,
                         keep: Optional[torch.Tensor] = None, exclude: Optional[torch.Tensor] = None, exact: bool = True):
        return _collapsed_search(self, q, k, max_per_group, fetch_k, keep, exclude, exact, self._groups, self.docs.shape[0],
                                 self.idx_offset, self.docs.device, self.docs.shape[0])

    collapsed_search.__doc__ = _COLLAPSED_DOC

    def count(self, q: torch.Tensor, min_score, keep: Optional[torch.Tensor] = None) -> torch.Tensor:
        """int64 [B] (0-d for a single query): how many documents of this index -- not removed (remove_ids), and kept by
        `keep` when given -- score at least min_score (a float, or a float32 [B] device tensor) for each query.  The scores
        are the ones search() returns, bit for bit, so a returned entry at the threshold is always counted.  One exact pass
        over the rows (score_count), also on a screen=True index."""
        self._check_q(q, width=False)  # (score_count checks the width, behind the dtype as it always has: the order stays)
        return score_count(q, self.docs, min_score, self._mask(keep))

    def range_search(self, q: torch.Tensor, min_score, k: int = 10, keep: Optional[torch.Tensor] = None):
        return _range_search(self, q, min_score, k, keep)

    range_search.__doc__ = _RANGE_DOC

    def _screens(self, B: int, k: int, masked: Optional[bool] = None) -> bool:
        """Whether a search of B queries for k takes the screened path.  ShardedIndex's ranks decide by this same rule
        whether they enter the seed exchange; the thresholds are the module's at the time of the call.
        masked: a keep-bitmask is in effect (None: the persistent one, if any) -- a masked search screens only on a
        screen_masked=True index."""
        N, d = self.docs.shape
        if masked is None:
            masked = self._keep is not None
        return (self._screen is not None and (not masked or self.screen_masked)
                and B >= (SCREEN_MIN_BATCH if d == 256 else SCREEN_PADDED_MIN_BATCH) and N >= SCREEN_MIN_DOCS and k <= SMALL_KMAX)

    def _search_screened(self, q: torch.Tensor, k: int, _prof_events=None, out=None, _seed_union=None,
                         _k_seed: int = 0, _k_list: int = 0, keep: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """search()'s screened path for a 2-D q; the arguments are search()'s, keep the ANDed mask (checked) or None."""
        B, d = q.shape
        sc = self._screen
        q = _f32c(q)
        if d < 256:
            qp = torch.zeros((B, 256), dtype=torch.float32, device=q.device)
            qp[:, :d] = q
            q = qp
        vals, idx = _out_pair(B, k, q.device, out)
        with torch.cuda.device(self.docs.device):  # workspace sizing depends on the device's CU count
            # per-call workspace and flags (cached allocator blocks): safe for concurrent callers and streams
            ws = torch.empty(sc.workspace_bytes(B, k, keep is not None), dtype=torch.uint8, device=self.docs.device)
            flags = torch.empty((B + 31) // 32, dtype=torch.int32, device=self.docs.device)
            if self.keep_stats:
                self._last_ws = (ws, B, k)
            seed = None
            if _seed_union is not None:
                ks = min(_k_list or _k_seed or k, k)  # entries per seed list (the caller ranks the union)
                seed = _seed_union(sc.seed_list(q, k, ks, flags, ws, keep))
                if seed.shape != (B,) or seed.dtype != torch.float32 or not seed.is_contiguous():
                    raise ValueError("_seed_union must return a contiguous float32 [B] tensor")
            sc.run(q, k, self.idx_offset, vals, idx, flags, ws, seed, _prof_events, keep)
        self.fallback_flags = flags  # of the most recent search (per 32-query tile; non-zero = exact kernel took over)
        return vals, idx


class GraphedSearch:
    """One search of a fixed shape (B, k) captured in a HIP graph and replayed: the launches of a
    screened search (query image with the flag reset, sample pass, threshold select, screen, finish, predicated
    exact kernels) become one graph launch, which matters at serving sizes where the whole search is < 1 ms.
    Everything in the library is asynchronous on the caller's stream with caller-owned memory, so plain
    stream capture works; queries are copied into a static buffer, results are returned in static buffers
    (valid until the next call).
    Removals: a graph captured while the index has a persistent keep-bitmask reads that buffer at every replay, so later
    remove_ids are honoured (on a screen_masked=True index the replayed launches are the masked screened search's).  A graph captured BEFORE the index had one holds the unmasked launches: calling it after a
    remove_ids raises RuntimeError (capture a new GraphedSearch) rather than return removed documents.

    Callers, streams and threads: ONE caller at a time per object -- the query, exclusion and result buffers and the graph's
    workspaces are static, so a second replay of the same object may start only after the first one's results have been
    read.  Different GraphedSearch objects over one index share nothing but its rows and may replay on different streams
    at once; a replay is asynchronous to the host."""

    def __init__(self, index: "BruteForceIndex", batch: int, k: int = 10, exclude_width: int = 0):
        self.index, self.B, self.k = index, int(batch), int(k)
        self._masked = index.keep_mask is not None
        dev = index.docs.device
        d = index.docs.shape[1]
        self.q = torch.zeros((self.B, d), dtype=torch.float32, device=dev)
        self.vals, self.idx = _out_pair(self.B, self.k, dev)
        if exclude_width < 0:
            raise ValueError(f"exclude_width = {exclude_width} < 0")
        # a static [B, exclude_width] list (-1 = padding): the graph holds the k + exclude_width search and the filter
        self.exclude = torch.full((self.B, int(exclude_width)), -1, dtype=torch.int64, device=dev) if exclude_width else None
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):  # warm-up outside capture: workspaces get allocated, kernels loaded
            for _ in range(2):
                index.search(self.q, self.k, out=(self.vals, self.idx), exclude=self.exclude)
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize(dev)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            index.search(self.q, self.k, out=(self.vals, self.idx), exclude=self.exclude)

    def __call__(self, q: torch.Tensor, exclude: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """exclude: int64 [B,E] with E <= exclude_width (a narrower list is padded with -1; None = nothing excluded)."""
        if tuple(q.shape) != tuple(self.q.shape):
            raise ValueError(f"GraphedSearch was captured for queries of shape {tuple(self.q.shape)}, got {tuple(q.shape)}")
        if not self._masked and self.index.keep_mask is not None:
            raise RuntimeError("GraphedSearch was captured before the index had a keep-bitmask (remove_ids): its graph would "
                               "return removed documents; capture a new GraphedSearch")
        if exclude is not None:
            width = 0 if self.exclude is None else self.exclude.shape[1]
            if (not isinstance(exclude, torch.Tensor) or exclude.dtype != torch.int64 or exclude.device != self.q.device
                    or exclude.dim() != 2 or exclude.shape[0] != self.B or exclude.shape[1] > width):
                raise ValueError(f"GraphedSearch was captured with exclude_width = {width}: exclude must be int64 "
                                 f"[{self.B}, E <= {width}] on {self.q.device}, got {getattr(exclude, 'dtype', None)} "
                                 f"{tuple(getattr(exclude, 'shape', ()))}")
        if self.exclude is not None:
            E = 0 if exclude is None else exclude.shape[1]
            if E < self.exclude.shape[1]:
                self.exclude[:, E:].fill_(-1)
            if E:
                self.exclude[:, :E].copy_(exclude)
        self.q.copy_(q)
        self.graph.replay()
        return self.vals, self.idx


def shard_bounds(n_total: int, rank: int, world: int) -> Tuple[int, int]:
    """Contiguous row shard of rank r: [r*N/W, (r+1)*N/W) with the remainder spread over the
    first ranks."""
    base, rem = divmod(n_total, world)
    lo = rank * base + min(rank, rem)
    return lo, lo + base + (1 if rank < rem else 0)


def _my_shard(n_total: int, group=None) -> Tuple[int, int]:
    """shard_bounds of this process in `group` (one shard holding everything without torch.distributed)."""
    import torch.distributed as dist
    on = dist.is_initialized()
    return shard_bounds(n_total, dist.get_rank(group) if on else 0, dist.get_world_size(group) if on else 1)


def _exchange_and_merge(vals: torch.Tensor, idx: torch.Tensor, k: int, merge: Callable, group=None):
    """Host logic of the sharded search on ordinary tensors: pack this rank's [B,kp] lists into one byte block,
    ONE all_gather_into_tensor, unpack to [B, world*kp] candidates, merge.  Private: the CPU tests drive it over
    gloo with the oracle's search and merge; the product path is ShardedIndex below, which exchanges in place."""
    import torch.distributed as dist
    world = dist.get_world_size(group)
    B, kp = vals.shape
    packed = torch.cat([vals.contiguous().view(torch.uint8).reshape(-1), idx.contiguous().view(torch.uint8).reshape(-1)])
    out = torch.empty(world * packed.numel(), dtype=torch.uint8, device=packed.device)
    dist.all_gather_into_tensor(out, packed, group=group)
    out = out.view(world, -1)
    nv = B * kp * 4
    gv = out[:, :nv].contiguous().view(torch.float32).view(world, B, kp)
    gi = out[:, nv:].contiguous().view(torch.int64).view(world, B, kp)
    gv = gv.permute(1, 0, 2).reshape(B, world * kp).contiguous()
    gi = gi.permute(1, 0, 2).reshape(B, world * kp).contiguous()
    return merge(gv, gi, k)


SEED_UNION_MAX = 512  # values per query tt_seed_union_f32 ranks (one LDS tile)


def seed_union(lists: torch.Tensor, world: int, kth: Optional[int] = None) -> torch.Tensor:
    """lists [world, B, ks] f32 (every rank's ks largest sample maxima per query) -> seed [B]: the kth-th (default ks-th)
    largest of each query's world * ks values (tt_seed_union_f32), on the current stream."""
    world_, B, ks = lists.shape
    assert world_ == world and lists.is_contiguous() and lists.dtype == torch.float32
    seed = torch.empty(B, dtype=torch.float32, device=lists.device)
    with torch.cuda.device(lists.device):
        _lib.check(_lib.lib().tt_seed_union_f32(lists.data_ptr(), world, B, ks, ks if kth is None else int(kth), seed.data_ptr(),
                                                _stream(lists)))
    return seed


def seed_plan(world: int, k: int, exchange: bool = True):
    """(list length per rank, rank taken from the union) of a sharded search's seed exchange, or None when the union does not
    apply: world * list length is bounded by tt_seed_union_f32's tile (SEED_UNION_MAX values per query); a job too wide for k
    values per rank lists fewer -- the k-th of the union is still reached by k distinct documents -- and one too wide even for
    that (or a k beyond the screen's 64) seeds every shard by itself."""
    if not exchange or k > SMALL_KMAX or world < 1:
        return None
    ks = min(k, SEED_UNION_MAX // world)
    if ks < 1 or world * ks < k:
        return None
    return ks, k


def _local_seed(lst: torch.Tensor) -> torch.Tensor:
    """No exchange: the union over one shard is that shard's own ks-th largest sample maximum."""
    return seed_union(lst.unsqueeze(0), 1)


class _Slot:
    """One set of exchange buffers of a ShardedIndex (three per shape: two that submit() alternates between, per shape
    (_SlotTurns) -- a step's all-gather + merge overlaps the next step's search -- and one of search()'s own): send block
    [vals f32 [B,kp] | idx int64 [B,kp]], receive buffer of `world` such blocks, outputs."""

    def __init__(self, B: int, kp: int, k: int, world: int, dev):
        self.nv = (B * kp * 4 + 7) // 8 * 8           # idx block 8-byte aligned
        self.stride = self.nv + B * kp * 8
        self.send = torch.empty(self.stride, dtype=torch.uint8, device=dev)
        self.recv = torch.empty(world * self.stride, dtype=torch.uint8, device=dev)
        self.send_v = self.send[:B * kp * 4].view(torch.float32).view(B, kp)
        self.send_i = self.send[self.nv:].view(torch.int64).view(B, kp)
        self.out_v, self.out_i = _out_pair(B, k, dev)
        self.sampled = torch.cuda.Event()   # caller's stream: the seed list is written
        self.seeded = torch.cuda.Event()    # exchange stream: the ranks' seed lists have been gathered
        self.searched = torch.cuda.Event()  # caller's stream: the send block is written
        self.merged = torch.cuda.Event()    # exchange stream: outputs are valid, send / receive buffers free

    def tensors(self):
        return (self.send, self.recv, self.out_v, self.out_i)


class _SlotTurns:
    """Whose turn it is in submit()'s two slots, kept PER SHAPE, on the host alone (no tensors: the CPU tests drive it).
    The n-th submit of a shape (n = 0, 1, ...: the step's generation) takes slot n % 2 of that shape's set, so a step's
    buffers are written again by the second further submit OF THE SAME SHAPE and by nothing else, whatever other shapes
    are submitted in between.  (One parity over all shapes -- what this replaces -- sent A, B, A to A's slot 0 twice: the
    first A's rows were overwritten after ONE further submit of its shape.)  The counts outlive a retired slot set (an int
    per shape ever seen), so the rule does not depend on which sets are resident."""

    def __init__(self):
        self._submitted = {}  # shape -> submits so far

    def take(self, shape) -> Tuple[int, int]:
        """(slot 0 / 1, generation) of the next submit of `shape`; the step that held the slot (generation - 2) expires."""
        n = self._submitted.get(shape, 0)
        self._submitted[shape] = n + 1
        return n % 2, n

    def holds(self, shape, generation: int) -> bool:
        """Whether the step of that generation still owns its slot: fewer than two submits of the shape have followed it."""
        return self._submitted.get(shape, 0) - generation <= 2


class PendingSearch:
    """Result of ShardedIndex.submit(): result() makes the CURRENT stream wait for the exchange + merge (no host
    synchronisation) and returns (values, indices) views valid until two more submits of the same shape -- the same
    (B, max(k + E, shard_k), k + E) -- on the same index.  Submits of other shapes in between do not count: the two slots
    alternate per shape (_SlotTurns), and search() has a slot of its own and never overwrites them.  Once the second further
    submit of the shape has been made the slot holds (or is being written with) that step's rows: result() then raises
    RuntimeError instead of returning them.  (A step submitted with exclude= that has been collected once keeps its filtered
    rows, which are its own tensors.)"""

    def __init__(self, slot: _Slot, index: "ShardedIndex", exclude: Optional[torch.Tensor] = None, k: int = 0,
                 shape=None, generation: int = 0):
        self._slot, self._index = slot, index
        self._exclude, self._k, self._filtered = exclude, k, None  # submit(exclude=): the filter runs in result(), once
        self._shape, self._generation = shape, generation          # the slot's generation when this step took it

    def result(self) -> Tuple[torch.Tensor, torch.Tensor]:
        """(A COLLECTIVE when this step's exchange has not been issued yet -- it normally goes out inside the NEXT submit():
        every rank must then call result() at the same point of its sequence of submit / search / result calls.)
        A step submitted with exclude= is filtered here, on the current stream, from the merged k + E rows into tensors of
        its own: the list must stay as it was until then.
        RuntimeError: two more submits of this step's shape have been made since, and its slot is another step's now."""
        if self._filtered is not None:
            return self._filtered
        if not self._index._turns.holds(self._shape, self._generation):
            B, kp, k = self._shape[:3]
            raise RuntimeError(f"PendingSearch.result(): this step's slot has been taken -- a result stays valid until two more "
                               f"submits of the same shape on the same index, and (B, k', k) = ({B}, {kp}, {k}) has been "
                               "submitted twice since; collect a step before the second further submit of its shape")
        self._index._flush(self._slot)
        torch.cuda.current_stream(self._slot.out_v.device).wait_event(self._slot.merged)
        if self._exclude is not None:
            self._filtered = topk_exclude(self._slot.out_v, self._slot.out_i, self._exclude, self._k)
            return self._filtered
        return self._slot.out_v, self._slot.out_i


class ShardedIndex(_CursorSearch):
    """Row-sharded corpus: every rank holds rows [lo,hi) and the SAME queries; search =
    local top-k' (global indices) -> one all-gather (RCCL over xGMI) -> merge on every rank.  Result is identical on
    all ranks and identical to the single-GPU search for any world size (the global top-k is a subset of the union of
    the shard top-k's).

    No glue kernels: the local search writes its [B,k'] lists straight into this rank's send block, ONE all-gather
    (tt_allgather_topk on torch.distributed's RCCL communicator; torch.distributed's own call for other backends),
    and the merge kernel reads the receive buffer in place (tt_topk_merge_shards).

    submit() pipelines consecutive searches on two streams, and keeps the collectives off the search's critical path.  One
    steady-state step (caller's stream C, exchange stream X; AG = all-gather on the one communicator):

        C: sample(i+1) ──sampled──┐                      ┌──seeded── union + screen(i+1) + rescoring ──searched(i+1)──> ...
        X:                        └─ seedAG(i+1) ────────┴─ listAG(i) ─ merge(i) ──merged(i)──> result(i)

    screen(i+1) waits for seedAG(i+1) only (k floats per query and rank: 40 KB per rank at B = 1024, k = 10); step i's list
    exchange (410-614 KB per rank) and merge are ISSUED BEHIND it and run under screen(i+1).  (Round 3 issued listAG(i) + merge(i)
    at the end of submit(i), in front of seedAG(i+1) on the same stream: the screen then waited for the whole previous exchange.)
    Every rank issues the same collectives in the same order -- seedAG(1), seedAG(2), listAG(1), seedAG(3), listAG(2), ... -- as
    long as all ranks make the same sequence of submit / result / search calls, which a sharded search requires anyway; a
    result() or search() that finds the last step's exchange still unissued issues it first, at the same point on every rank.

    Whether the seed exchange happens at all is agreed ONCE, in the constructor (a collective): every rank has an fp16 shadow
    copy and at least SCREEN_MIN_DOCS rows, or no rank exchanges seeds -- a rank-local decision (shard sizes straddling the
    minimum, one shard outside the fp16 range) would leave some ranks in an all-gather the others never enter.

    Callers, streams and threads: ONE issuing host thread per object (every search is a collective: the ranks must issue the
    same calls in the same order), on any streams.  Calls that share a slot (search / tagged_search / search_after of one
    shape; biased_search has its own) are ordered by the slot's `merged` event, which a call waits for on entry and records
    after its last read of the slot, so a call on another stream never overwrites rows that are still being copied out;
    submit()'s two slots per shape are ordered the same way and search() never touches them.  Asynchronous to the host,
    except where the shard's own index synchronises (a streamed shard's score_ids / candidates= / diverse_search) and
    collapsed_search(exact=True)."""

    def __init__(self, local_docs, row_offset: int, group=None, shard_k: int = 50, screen: bool = False,
                 comm=None, block_docs: int = 1 << 20, device=None, screen_masked: bool = False):
        """local_docs: this rank's rows [row_offset, row_offset + n) of the corpus, as
          * a device fp32 [n,d] tensor: resident shard (BruteForceIndex; BASELINE configs[3]),
          * a device bf16 [n,d] tensor: resident shard kept as bf16 (BruteForceIndex over it; with screen=True it screens from
            the bf16 rows and takes part in the seed exchange like an fp32 shard), or
          * a CPU bfloat16 [n,d] tensor / a StreamedIndex: the shard stays in pinned host DRAM and every search streams it
            through the GPU in blocks of block_docs rows (BASELINE configs[4]: 100M x 256 bf16 over 8 GPUs = 12.5M rows,
            6.4 GB per rank, PCIe-bound).  The streamed shard's list is the exact top-k' of its rows (bf16 -> fp32 is exact),
            so the exchange and the merge are the resident path's, unchanged.
        A job may mix the two kinds (a rank that has the HBM keeps its shard resident).  The seed exchange is a property of the
        whole job: with ANY streamed shard no rank exchanges seeds.  (A streamed shard searches block by block, each block
        seeded by its own sample pass, which is valid on its own; a union seed would need the sample maxima of the whole
        shard before the first block is screened, i.e. one more pass over PCIe, which is what binds.)
        screen_masked: the shard's index keeps masked searches on the screened path (BruteForceIndex); like `screen` it is a
        property of the job, the same on every rank (a ready StreamedIndex brings its own)."""
        from .collective import Collective
        self.group = group
        self.row_offset = int(row_offset)
        self.shard_k = int(shard_k)
        if isinstance(local_docs, StreamedIndex):
            if local_docs.idx_offset != self.row_offset:
                raise ValueError(f"the StreamedIndex numbers its rows from {local_docs.idx_offset}, the shard starts at {row_offset}")
            self._index = local_docs
        elif not local_docs.is_cuda and local_docs.dtype == torch.bfloat16:
            self._index = StreamedIndex(local_docs, block_docs=block_docs, device=device, idx_offset=row_offset, screen=True,
                                        screen_masked=screen_masked)
        else:
            self._index = BruteForceIndex(local_docs, idx_offset=row_offset, screen=screen, screen_masked=screen_masked)
        self.screen_masked = self._index.screen_masked
        self.streamed = isinstance(self._index, StreamedIndex)
        self._dev = self._index.device
        self._coll = Collective(group, self._dev, comm=comm)
        self._slots = {}
        self._turns = _SlotTurns()  # which of a shape's two submit() slots is next, and the generation it then holds
        self._xs: Optional[torch.cuda.Stream] = None
        self._deferred = None  # (slot, B, kp, k) of the last submit(): its list exchange goes out behind the next seed gather
        # a resident d = 256 shard that screens its smallest screened batch
        mine = int(not self.streamed and self._index.docs.shape[1] == 256 and self._index._screens(SCREEN_MIN_BATCH, 1))
        if self._coll.world > 1:
            dev = self._dev
            send = torch.tensor([mine], dtype=torch.int64, device=dev)
            recv = torch.empty(self._coll.world, dtype=torch.int64, device=dev)
            self._coll.all_gather_blocks(send.view(torch.uint8), recv.view(torch.uint8))
            mine = int(recv.min().item())
        self._seed_exchange = bool(mine)  # the same on every rank
        self.collapse_rounds = (0, 0)  # (batched, masked) rounds of the most recent collapsed_search

    def _seed_plan(self, k: int):
        return seed_plan(self._coll.world, k, self._seed_exchange)

    @property
    def keep_mask(self) -> Optional[torch.Tensor]:
        """This rank's persistent keep-bitmask over its own rows (remove_ids), or None."""
        return self._index.keep_mask

    def remove_ids(self, ids) -> None:
        """Withdraw documents by GLOBAL id.  Called by EVERY rank with the same ids, like every other call on this class: each
        rank clears the bits of the ids in its shard and ignores the rest, and every rank allocates its mask, also where no
        id falls in its shard -- whether a search is masked decides whether a rank enters the seed all-gather, so it has to be
        a property of the job, not of a rank.  So does screen_masked: with it a masked search enters the seed exchange like an
        unmasked one, without it none does, and the ranks must agree."""
        self._index.remove_ids(ids)

    def _local_search(self, q: torch.Tensor, kp: int, k: int, sl: "_Slot", comm_stream=None, keep=None, candidates=None) -> None:
        """This shard's list for the exchange: up to kp = max(k, shard_k) entries, best first.  The screen is seeded for
        the FINAL k with the UNION seed: every rank lists its k largest sample maxima per query, ONE small all-gather
        (k floats per query and rank: 40 KB per rank at B = 1024), and seed[q] = the k-th largest of the union -- k distinct
        documents of the whole corpus reach it, so it bounds the global k-th score from below as well as the unsharded
        search's own sample would (a shard's own k-th sample maximum is much weaker, and on a small shard the candidates
        that get through, not the matrix pipes, set the screen's pace: 1.25M rows, emulated 8 shards, 0.640 -> 0.582 ms).
        The shard then owes the exchange only its documents above that global threshold: entries beyond them are padding
        (-inf / -1), which the merge ignores; the merged top-k is exact (two real-kernel ranks vs the oracle,
        tests/test_multirank_gpu.py).
        comm_stream: the stream the seed all-gather is issued on (submit(): the index's exchange stream; the previous step's
        deferred list exchange is issued right behind it); None = the caller's."""
        coll, world = self._coll, self._coll.world
        if candidates is not None:
            # a candidate search never screens, so no rank exchanges seeds: this shard's candidates (the other shards' ids
            # are padding to it), merged to kp
            if comm_stream is not None:
                self._flush()
            self._index.search(q, kp, out=(sl.send_v, sl.send_i), keep=keep, candidates=candidates)
            return
        plan = self._seed_plan(k)
        B = q.shape[0]
        # (a seed plan implies a resident shard: no rank exchanges seeds when any shard is streamed)
        # (masked and screen_masked, which _screens weighs it with, are the same on every rank: remove_ids, search, __init__)
        masked = keep is not None or self._index.keep_mask is not None
        if plan is None or not self._index._screens(B, k, masked) or (world == 1 and kp == k):
            # no seed exchange on any rank (agreed in the constructor; B, k and masked are the same everywhere): the shard's own
            # search -- the masked exact kernel when a mask is in effect and the index does not screen under one; a short
            # list's padding is ignored by the merge
            if comm_stream is not None:
                self._flush()
            self._index.search(q, kp, out=(sl.send_v, sl.send_i), keep=keep)
            return
        ks, kth = plan

        def union(lst: torch.Tensor) -> torch.Tensor:
            if world == 1:
                return seed_union(lst.unsqueeze(0), 1, kth)
            recv = torch.empty((world,) + tuple(lst.shape), dtype=torch.float32, device=lst.device)
            send_b, recv_b = lst.view(-1).view(torch.uint8), recv.view(-1).view(torch.uint8)
            if comm_stream is None:
                coll.all_gather_blocks(send_b, recv_b)
            else:
                cur = torch.cuda.current_stream(lst.device)
                sl.sampled.record(cur)
                with torch.cuda.stream(comm_stream):
                    comm_stream.wait_event(sl.sampled)
                    lst.record_stream(comm_stream)
                    recv.record_stream(comm_stream)
                    coll.all_gather_blocks(send_b, recv_b)
                    sl.seeded.record(comm_stream)
                self._flush()                # the PREVIOUS step's list exchange + merge: behind this step's seed gather
                cur.wait_event(sl.seeded)    # (the event, not the stream: the screen does not wait for that exchange)
            return seed_union(recv, world, kth)

        # (under a mask the seed lists hold kept documents' maxima only: distinct kept documents of disjoint shards, so the
        #  union seed bounds the masked global k-th score as it is)
        self._index.search(q, kp, out=(sl.send_v, sl.send_i), _seed_union=union, _k_seed=k, _k_list=ks, keep=keep)

    @property
    def collective(self) -> str:
        """Which transport the exchange uses (reported by bench.py)."""
        return self._coll.via

    @classmethod
    def from_global(cls, docs: torch.Tensor, group=None, **kw) -> "ShardedIndex":
        lo, hi = _my_shard(docs.shape[0], group)
        return cls(docs[lo:hi], lo, group=group, **kw)

    @classmethod
    def from_host_bf16(cls, host_docs: torch.Tensor, group=None, resident: bool = False, **kw) -> "ShardedIndex":
        """BASELINE configs[4]: `host_docs` is the WHOLE bf16 corpus [N,d] in host memory (an np.memmap-backed tensor will do:
        only this rank's rows are touched); rank r pins and streams rows [r*N/W, (r+1)*N/W) only.  resident=True: rank r
        copies those rows to its GPU once, as bf16 (n*d*2 bytes of HBM), and searches them there."""
        lo, hi = _my_shard(host_docs.shape[0], group)
        rows = host_docs[lo:hi]
        if resident:
            dev = kw.pop("device", None)
            rows = rows.to(torch.device(dev) if dev is not None else torch.device("cuda", torch.cuda.current_device()))
        return cls(rows, lo, group=group, **kw)

    @classmethod
    def from_documents(cls, model, tokenizer, documents, device, group=None, **kw) -> "ShardedIndex":
        """Index build across ranks (third row: embarrassingly parallel over documents, no collective): every rank
        holds the same document list (documents.pkl order, backend/main.py:134-136), embeds ONLY its contiguous shard
        [lo, hi) with the document tower and keeps those rows; row i of the global index is documents[i] on every rank."""
        from .evaluators import embed_corpus
        lo, hi = _my_shard(len(documents), group)
        model.eval()
        with torch.no_grad():
            local = embed_corpus(model, tokenizer, documents[lo:hi], device)
        return cls(local, lo, group=group, **kw)

    _MAX_SLOT_SHAPES = 8

    def _slot(self, B: int, kp: int, k: int, which: int) -> _Slot:
        """which: 0 / 1 = the two slots submit() alternates between, 2 = search()'s own (a search() between a submit() and
        its .result() must not overwrite that PendingSearch's outputs), 3 = biased_search()'s own, made on first use (its values
        are biased scores: they share no buffer with a search's).  Slot sets are kept per (B, kp, k) shape; when
        more than _MAX_SLOT_SHAPES shapes have been seen the oldest set is retired, after its queued exchanges have
        completed (its buffers are used on the exchange stream, which the caching allocator does not know about)."""
        key = (B, kp, k, self._coll.world)
        if key not in self._slots:
            while len(self._slots) >= self._MAX_SLOT_SHAPES:
                old = self._slots.pop(next(iter(self._slots)))
                for sl in old:
                    sl.merged.synchronize()
            self._slots[key] = [_Slot(B, kp, k, self._coll.world, self._dev) for _ in range(3)]
        while len(self._slots[key]) <= which:
            self._slots[key].append(_Slot(B, kp, k, self._coll.world, self._dev))
        return self._slots[key][which]

    def _flush(self, only: Optional[_Slot] = None) -> None:
        """Issue the deferred list exchange + merge of the last submit() on the exchange stream (only: just if it is that
        slot's)."""
        d = self._deferred
        if d is None or (only is not None and d[0] is not only):
            return
        self._deferred = None
        sl, B, kp, k = d
        with torch.cuda.stream(self._xs):
            self._xs.wait_event(sl.searched)
            for t in sl.tensors():           # allocated on the caller's stream, used on the exchange stream
                t.record_stream(self._xs)
            self._exchange_merge(sl, B, kp, k)
            sl.merged.record(self._xs)

    def _exchange_merge(self, sl: _Slot, B: int, kp: int, k: int) -> None:
        """all-gather + in-place merge of one slot on the CURRENT stream."""
        self._coll.all_gather_blocks(sl.send, sl.recv)
        with torch.cuda.device(sl.recv.device):
            merge = getattr(_lib.lib(), _merge_fn(k, kp, shards=True))
            _lib.check(merge(sl.recv.data_ptr(), self._coll.world, sl.stride, sl.nv, B, kp, k, sl.out_v.data_ptr(),
                             sl.out_i.data_ptr(), _stream(sl.recv)))

    def search(self, q: torch.Tensor, k: int = 10, keep: Optional[torch.Tensor] = None,
               exclude: Optional[torch.Tensor] = None, candidates: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """One search, everything on the caller's stream; fresh result tensors.
        candidates: per-query candidate lists of GLOBAL ids, int64 [B,C] ([C] with a 1-D q), the same on every rank like q.
        Every rank scores the candidates of its own shard (the others are padding to it) and merges them to its list; the
        exchange and the shard merge are the ordinary search's.  A COLLECTIVE like every search of this class.
        keep: a packed keep-bitmask over THIS RANK'S rows for this call (ANDed with the mask of remove_ids).  It must be given
        on all ranks or on none: a masked search does not enter the seed exchange (with screen_masked=True it does, on every
        rank alike).
        exclude: per-query exclusion lists of GLOBAL ids, int64 [B,E] ([E] with a 1-D q), the same on every rank like q.  The
        local search, the exchange and the merge are those of a search for k + E (per-shard lists of max(k + E, shard_k));
        the filter (tt_topk_exclude_ids) runs once, on the merged rows."""
        if q.dim() == 1:
            return _squeezed(self.search, q, k, keep, _exclude_row(exclude), _ids_row(candidates, "candidates"))
        k_out = k
        if exclude is not None:
            exclude, k = _check_exclude(exclude, q.shape[0], k, self._dev)
        if candidates is not None:
            candidates = _check_ids(candidates, q.shape[0], self._dev, "candidates")
        kp = max(k, self.shard_k)
        return self._exchange_step(2, q.shape[0], kp, k,
                                   lambda sl: self._local_search(q, kp, k, sl, keep=keep, candidates=candidates),
                                   _cloned if exclude is None else lambda v, i: topk_exclude(v, i, exclude, k_out))

    def _exchange_step(self, which: int, B: int, kp: int, k: int, local: Callable, read: Callable):
        """One search of this class on the caller's stream, through slot `which` (_slot) of the shape: local(slot) writes this
        shard's [B,kp] list into the slot's send block (slot.send_v, slot.send_i), the ranks' lists are gathered and merged
        to k, and read(out_v, out_i) takes the result out of the slot -- copies, clones or the exclusion filter: whatever
        read returns is the caller's own.  The rule that orders callers on different streams: `merged` is waited for before
        anything writes the slot and recorded AFTER THE LAST READ of it, so the next caller, on whatever stream, never
        overwrites rows that are still being copied out."""
        sl = self._slot(B, kp, k, which)
        cur = torch.cuda.current_stream(sl.send.device)
        cur.wait_event(sl.merged)  # (a call on another stream may still own the slot)
        self._flush()              # (a submitted step's exchange goes out first: one issue order on every rank)
        local(sl)
        self._exchange_merge(sl, B, kp, k)
        res = read(sl.out_v, sl.out_i)
        sl.merged.record(cur)
        return res

    @property
    def tags(self) -> Optional[torch.Tensor]:
        """This rank's tags over its own rows (set_tags), or None."""
        return self._index.tags

    def set_tags(self, local_tags: torch.Tensor) -> None:
        """One 32-bit tag per row of THIS RANK'S shard (BruteForceIndex.set_tags / StreamedIndex.set_tags).  Called on every
        rank, like every call on this class: tagged search is a property of the job."""
        self._index.set_tags(local_tags)

    def tagged_search(self, q: torch.Tensor, k: int = 10, match_mask=0xffffffff, match_value=0,
                      keep: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """search() with a filter per query (BruteForceIndex.tagged_search): q, match_mask and match_value are the same on
        every rank, the tags are each rank's own.  The local tagged search runs for max(k, shard_k) (<= 64: ValueError above),
        then the usual all-gather and merge on the caller's stream; no seed exchange is involved, so every rank enters the
        same collectives whatever its tags hold.  A COLLECTIVE like every search of this class.  keep: as in search()."""
        if self._index.tags is None:
            raise ValueError("tagged_search: this index has no tags (set_tags)")
        if q.dim() == 1:
            return _squeezed(self.tagged_search, q, k, match_mask, match_value, keep)
        kp = _TAGGED.shard_k(k, self.shard_k)
        return self._exchange_step(2, q.shape[0], kp, k, lambda sl: self._index.tagged_search(
            q, kp, match_mask, match_value, keep=keep, out=(sl.send_v, sl.send_i)), _cloned)

    @property
    def bias(self) -> Optional[torch.Tensor]:
        """This rank's biases over its own rows (set_bias), or None."""
        return self._index.bias

    def set_bias(self, local_bias: Optional[torch.Tensor]) -> None:
        """One float32 bias per row of THIS RANK'S shard (BruteForceIndex.set_bias / StreamedIndex.set_bias; None clears it).
        Called on every rank, like every call on this class: biased search is a property of the job."""
        self._index.set_bias(local_bias)

    def biased_search(self, q: torch.Tensor, k: int = 10, keep: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """search() ranked by q.d + bias[n] (BruteForceIndex.biased_search): q is the same on every rank, the biases are each
        rank's own.  The local biased search runs for max(k, shard_k) (<= 64: ValueError above), then the usual all-gather and
        merge on the caller's stream -- the merges see values that are already biased; no seed exchange is involved.  A
        COLLECTIVE like every search of this class.  keep: as in search()."""
        if self._index.bias is None:
            raise ValueError("biased_search: this index has no bias (set_bias)")
        if q.dim() == 1:
            return _squeezed(self.biased_search, q, k, keep)
        kp = _BIASED.shard_k(k, self.shard_k)
        return self._exchange_step(3, q.shape[0], kp, k, lambda sl: self._index.biased_search(
            q, kp, keep=keep, out=(sl.send_v, sl.send_i)), _cloned)

    def _cursor_device(self) -> torch.device:
        return self._dev

    def _search_after(self, q: torch.Tensor, k: int, av: torch.Tensor, ai: torch.Tensor, keep: Optional[torch.Tensor], out=None):
        """search_after (_CursorSearch) over the job: q and the cursor are the same on every rank -- a global (score, id) cursor
        means the same on every shard, whichever shard its document lives on.  The local cursor search runs for
        max(k, shard_k) (<= 64: ValueError above), then the usual all-gather and merge on the caller's stream; no seed exchange
        is involved.  A COLLECTIVE like every search of this class, and so are pages(), deep_search() and
        mine_hard_negatives over it.  keep: as in search()."""
        kp = _AFTER.shard_k(k, self.shard_k)
        return self._exchange_step(2, q.shape[0], kp, k, lambda sl: self._index._search_after(
            q, kp, av, ai, keep, (sl.send_v, sl.send_i)), _cloned if out is None else lambda v, i: _copied(out, v, i))

    def _all_reduce(self, t: torch.Tensor, op: str) -> torch.Tensor:
        """t reduced elementwise over the ranks, op "SUM" or "MAX": torch.distributed's all_reduce on the index's group, in
        place; with a communicator of the library's own and no torch.distributed, the ranks' blocks gathered and reduced
        here.  One rank: t as it is."""
        if self._coll.world == 1:
            return t
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized():
            dist.all_reduce(t, op=getattr(dist.ReduceOp, op), group=self.group)
            return t
        recv = torch.empty((self._coll.world,) + tuple(t.shape), dtype=t.dtype, device=t.device)
        self._coll.all_gather_blocks(t.reshape(-1).view(torch.uint8), recv.view(-1).view(torch.uint8))
        return recv.sum(0) if op == "SUM" else recv.amax(0)

    def score_ids(self, q: torch.Tensor, ids: torch.Tensor, keep: Optional[torch.Tensor] = None) -> torch.Tensor:
        """float32 [B,C] ([C] for a single query), identical on every rank: the exact dense score of every id of ids int64
        [B,C] (GLOBAL ids, the same on every rank like q), -inf where the id is negative, beyond the corpus, removed or not
        kept (keep: over THIS RANK'S rows, on all ranks or on none).  Each rank scores against its own shard, where the other
        shards' ids are padding (-inf); exactly one rank holds a real value, so the result is the elementwise MAX over the
        ranks: one all_reduce(MAX) of the [B,C] floats on the index's group.  A COLLECTIVE: every rank calls it at the same
        point."""
        return self._all_reduce(self._index.score_ids(q, ids, keep=keep), "MAX")

    def diverse_search(self, q: torch.Tensor, k: int = 10, lambda_: float = 0.5, fetch_k: Optional[int] = None,
                       keep: Optional[torch.Tensor] = None, exclude: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        if q.dim() == 1:
            return _squeezed(self.diverse_search, q, k, lambda_, fetch_k, keep, _exclude_row(exclude))
        fk, lam = _mmr_fetch_k(k, fetch_k), _check_lambda(lambda_)
        v, i = self.search(q, fk, keep=keep, exclude=exclude)
        return mmr_select(v, i, None, k, lam, rows=self._all_reduce(self._index._candidate_rows(i), "SUM"))

    diverse_search.__doc__ = _DIVERSE_DOC + """
        Sharded, a COLLECTIVE like every search of this class: the sharded search for fetch_k, identical on every rank; then
        each rank fills a float32 [B,fetch_k,d] block with the rows of the candidates it owns (zeros elsewhere) and the
        blocks are summed over the ranks -- one all_reduce(SUM) of B * fetch_k * d * 4 bytes on the index's group (13 MB at
        B = 100, fetch_k = 128, d = 256).  Exactly one rank contributes each row and x + 0 is exact, so every rank holds the
        candidates' rows and runs the selection on them (tt_mmr_select_rows_f32): the single-GPU result on every rank."""

    @property
    def groups(self) -> Optional[torch.Tensor]:
        """This rank's group ids over its own rows (set_groups), or None."""
        return self._index.groups

    def set_groups(self, local_groups: Optional[torch.Tensor]) -> None:
        """One int64 group id per row of THIS RANK'S shard (BruteForceIndex.set_groups / StreamedIndex.set_groups; None clears
        it); the ids are global names, a group may span shards.  Called on every rank, like every call on this class."""
        self._index.set_groups(local_groups)

    def _gather_gids(self, ids: torch.Tensor) -> torch.Tensor:
        """The group ids of merged result ids on every rank: each rank fills in the ids it owns (zeros elsewhere), one
        all_reduce(SUM) of the int64 block on the index's group."""
        return self._all_reduce(_owned_gids(self._index.groups, ids, self.row_offset), "SUM")

    def collapsed_search(self, q: torch.Tensor, k: int = 10, max_per_group: int = 1, fetch_k: Optional[int] = None,
                         keep: Optional[torch.Tensor] = None, exclude: Optional[torch.Tensor] = None, exact: bool = True):
        return _collapsed_search(self, q, k, max_per_group, fetch_k, keep, exclude, exact, self._index.groups, self._index.ntotal,
                                 self.row_offset, self._dev, None, self._gather_gids)

    collapsed_search.__doc__ = _COLLAPSED_DOC + """
        Sharded, a COLLECTIVE like every search of this class (q, exclude and the arguments the same on every rank; keep over
        THIS RANK'S rows, on all ranks or on none): the sharded search for fetch_k, identical on every rank; each rank fills
        the group ids of the result ids it owns and zeros elsewhere, one all_reduce(SUM) of the int64 [B,fetch_k] block
        completes them, and every rank runs the filter on the ids (tt_topk_collapse_gids): the single-index result on every
        rank.  In a masked round every rank clears its own rows of the saturated groups -- every rank derives the same set
        from the identical merged result.  The corpus size is not known to a rank, so the default fetch_k is not cut to it."""

    def count(self, q: torch.Tensor, min_score, keep: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The count of the whole corpus, identical on every rank: this rank's count over its shard under its mask (keep: over
        THIS RANK'S rows, on all ranks or on none, as in search()), then one all_reduce(SUM) of the int64 [B] on the index's
        group.  A COLLECTIVE: every rank calls it at the same point."""
        return self._all_reduce(self._index.count(q, min_score, keep=keep), "SUM")

    def range_search(self, q: torch.Tensor, min_score, k: int = 10, keep: Optional[torch.Tensor] = None):
        return _range_search(self, q, min_score, k, keep)

    range_search.__doc__ = _RANGE_DOC + """
        Sharded: counts are count()'s (one all_reduce), the rows the sharded search()'s, cut on every rank alike."""

    @property
    def device(self) -> torch.device:
        return self._dev

    def submit(self, q: torch.Tensor, k: int = 10, keep: Optional[torch.Tensor] = None,
               exclude: Optional[torch.Tensor] = None, candidates: Optional[torch.Tensor] = None) -> PendingSearch:
        """Pipelined search of a [B,d] batch: the local search is enqueued on the caller's stream now; its list exchange and
        merge go out on this index's second stream inside the NEXT submit() (behind that step's seed gather), or when
        .result() / search() asks for them.  Call .result() when the answer is needed.  keep: as in search() (all ranks or
        none).  exclude: as in search(); the step runs for k + E and .result() filters the merged rows.  candidates: as in
        search(): the step's local search is the candidate search.
        Slots: the step writes one of two slots of its shape (B, max(k + E, shard_k), k + E), taken in turn per shape, so
        its result is valid until two more submits of THAT shape, however many other shapes are submitted in between; after
        that its .result() raises RuntimeError.  The collectives issued, and their order, do not depend on the slot."""
        if q.dim() != 2:
            raise ValueError("submit wants a [B,d] batch")
        k_out = k
        if exclude is not None:
            exclude, k = _check_exclude(exclude, q.shape[0], k, self._dev)
        if candidates is not None:
            candidates = _check_ids(candidates, q.shape[0], self._dev, "candidates")
        kp = max(k, self.shard_k)
        B = q.shape[0]
        shape = (B, kp, k, self._coll.world)
        which, generation = self._turns.take(shape)
        sl = self._slot(B, kp, k, which)
        dev = sl.send.device
        if self._xs is None:
            self._xs = torch.cuda.Stream(device=dev)
        cur = torch.cuda.current_stream(dev)
        self._flush(sl)                      # (the slot's own previous step, if nobody collected it: issue before reuse)
        cur.wait_event(sl.merged)            # the slot's previous exchange has read its send block
        self._local_search(q, kp, k, sl, comm_stream=self._xs, keep=keep, candidates=candidates)
        self._flush()                        # (a local search without a seed exchange has not issued the previous step's yet)
        sl.searched.record(cur)
        self._deferred = (sl, B, kp, k)
        return PendingSearch(sl, self, exclude, k_out, shape, generation)


class StreamedIndex(_CursorSearch):
    """BASELINE configs[4]: a corpus kept as bf16 rows in (pinned) host DRAM and streamed through the GPU.

    search() walks the corpus in blocks: a copy stream moves block i+1 host -> device (hipMemcpyAsync from
    pinned memory) while the compute stream widens block i to fp32 (+ fp16 shadow), searches it with the
    resident-corpus kernels (idx_offset = block start) and folds the block's top-k into the running top-k
    with the merge kernel.  Two staging buffers; events order the two streams.  The result is the exact
    top-k over the bf16 corpus (bf16 -> fp32 is exact), with the usual (score desc, index asc) order.
    PCIe-bound by design: ~55-60 GB/s on Gen5 x16, i.e. ~110 ms per pass over a 6.4 GB shard.

    Callers, streams and threads: RE-ENTRANT.  Any interleaving of the searches of one object from any streams and from
    several host threads returns what each call returns alone.  The staging buffers, the widened blocks, the copy stream and
    the pinned gather buffers are the object's, so passes over them are ORDERED, not concurrent: a host lock covers the part
    of a call that enqueues a pass (a walk, or score_ids' gather), and an event recorded on the caller's stream at the end of
    each pass is waited for by the next pass's stream and by the copy stream -- passes run on the device one after another in
    the order they were issued, whatever streams they came from (a pass is PCIe-bound: two at once would share the link).
    No memory is added per caller.  A walk stays asynchronous to the host; score_ids, search(candidates=) and
    diverse_search synchronise with the host as their docstrings say, and a thread that issues a pass meanwhile waits for
    that call's lock.  remove_ids / set_tags / set_bias / set_groups are the one mutating caller's: not while searches are
    being issued.  collapse_rounds describes the most recent call.
    """

    def __init__(self, host_docs: torch.Tensor, block_docs: int = 1 << 20, device=None, idx_offset: int = 0,
                 screen: bool = True, screen_masked: bool = False):
        if host_docs.is_cuda or host_docs.dtype != torch.bfloat16 or host_docs.dim() != 2:
            raise ValueError("StreamedIndex wants a CPU bfloat16 [N,d] tensor (pinned for full PCIe speed)")
        self.host = host_docs if (host_docs.shape[0] == 0 or host_docs.is_pinned()) else host_docs.pin_memory()
        self.N, self.d = self.host.shape
        self.block = int(min(block_docs, max(self.N, 1)))
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.idx_offset = int(idx_offset)
        self.screen_masked = bool(screen_masked)  # the per-block views screen masked searches too (BruteForceIndex)
        dev = self.device
        self._stage = [torch.empty((self.block, self.d), dtype=torch.bfloat16, device=dev) for _ in range(2)]
        self._d32 = [torch.empty((self.block, self.d), dtype=torch.float32, device=dev) for _ in range(2)]
        self._d16 = [torch.empty((self.block, self.d), dtype=torch.float16, device=dev) for _ in range(2)] \
            if (screen and self.d == 256) else [None, None]
        self._copy = torch.cuda.Stream(device=dev)
        self._ready = [torch.cuda.Event() for _ in range(2)]
        self._free = [torch.cuda.Event() for _ in range(2)]
        self._lock = threading.Lock()    # held while a pass over the staging buffers is being enqueued (_ordered)
        self._done = torch.cuda.Event()  # caller's stream: the most recent pass has read the last of the shared buffers
        # one streaming pass at build time: the corpus-wide largest row norm bounds the screen's error term
        stats = torch.zeros(2, dtype=torch.float32, device=dev)
        self._walk(lambda s, lo, n: None, stats=stats)
        dmax, amax = (float(x) for x in stats.tolist())
        self.dmax_norm = dmax
        if not _fp16_range_ok(dmax, amax):
            self._d16 = [None, None]
        self._keep: Optional[torch.Tensor] = None  # persistent keep-bitmask (remove_ids): N/8 bytes, on the device
        self._gather = None  # two pinned [block,d] host buffers of the candidate gather (_score_ids), allocated on first use
        self._tags: Optional[torch.Tensor] = None  # one 32-bit tag per row, resident on the device (set_tags): 4 bytes per row
        self._bias: Optional[torch.Tensor] = None  # one float per row, resident on the device (set_bias): 4 bytes per row
        self._groups: Optional[torch.Tensor] = None  # one int64 group id per row, resident on the device (set_groups)
        self.collapse_rounds = (0, 0)  # (batched, masked) rounds of the most recent collapsed_search

    @contextlib.contextmanager
    def _ordered(self):
        """One pass over the shared buffers (staging, widened blocks, pinned gather) at a time, in issue order: yields the
        caller's stream once it and the copy stream are behind the previous pass -- whichever stream that ran on --, under
        the object's lock; on the way out the pass's end is recorded on that stream for the next one.  Nothing here waits on
        the host."""
        with self._lock:
            cur = torch.cuda.current_stream(self.device)
            cur.wait_event(self._done)         # the previous pass's kernels have read _d32 / _d16 / _stage
            self._copy.wait_event(self._done)  # ... before this pass's first copy lands in _stage
            try:
                yield cur
            finally:
                self._done.record(cur)

    def _staged(self, s: int, rows: torch.Tensor, cur, consume: Callable) -> None:
        """The staging handshake, for both kinds of pass: `rows` (pinned host memory) -> staging buffer s on the copy stream
        once that buffer has been consumed (_free[s]); the caller's stream `cur` waits for the copy (_ready[s]);
        consume(staged rows, s) enqueues on `cur` what reads the buffer; then _free[s] is recorded on `cur`.  (A plain call,
        not a context manager: it runs once per block of every walk.)"""
        staged = self._stage[s][:rows.shape[0]]
        with torch.cuda.stream(self._copy):
            self._copy.wait_event(self._free[s])
            staged.copy_(rows, non_blocking=True)
            self._ready[s].record(self._copy)
        cur.wait_event(self._ready[s])
        consume(staged, s)
        self._free[s].record(cur)

    def _walk(self, visit, stats=None):
        L = _lib.lib()
        nblk = (self.N + self.block - 1) // self.block

        def widen(staged, s):  # bf16 block -> fp32 rows (+ fp16 shadow, + the build pass's statistics)
            with torch.cuda.device(self.device):
                _lib.check(L.tt_index_build_from_bf16(
                    self._stage[s].data_ptr(), staged.shape[0], self.d, self._d32[s].data_ptr(),
                    self._d16[s].data_ptr() if self._d16[s] is not None else None,
                    stats.data_ptr() if stats is not None else None, 0, cur.cuda_stream))

        with self._ordered() as cur:
            for s in range(2):
                self._free[s].record(cur)
            for i in range(nblk):
                s = i % 2
                lo = i * self.block
                n = min(self.block, self.N - lo)
                self._staged(s, self.host[lo:lo + n], cur, widen)
                visit(s, lo, n)

    def resident(self, dtype: torch.dtype = torch.float32) -> "BruteForceIndex":
        """The same corpus widened once into HBM (N*d*4 bytes fp32 + N*d*2 bytes fp16 shadow): configs[4]'s shard
        of 12.5M passages is 19.2 GB of a 288 GB GPU, after which it is searched at the resident rates.
        dtype=torch.bfloat16: the rows are copied to HBM as they are (N*d*2 bytes, 6.4 GB for that shard) and searched by
        the exact bf16 kernel (same results).
        The new index starts from this index's state: it is handed COPIES of the keep-bitmask of remove_ids and of the tags,
        biases and group ids (set_tags / set_bias / set_groups), so what was removed stays removed and every flavour of search
        answers as it does here.  From then on the two are independent: a later remove_ids or set_* on one does not show on
        the other."""
        if dtype == torch.bfloat16:
            return self._hand_state(BruteForceIndex(self.host.to(self.device), idx_offset=self.idx_offset,
                                                    screen_masked=self.screen_masked))
        if dtype != torch.float32:
            raise ValueError(f"resident() keeps float32 or bfloat16 rows, not {dtype}")
        d32 = torch.empty((self.N, self.d), dtype=torch.float32, device=self.device)
        d16 = torch.empty((self.N, self.d), dtype=torch.float16, device=self.device) if self._d16[0] is not None else None

        def visit(s, lo, n):
            d32[lo:lo + n].copy_(self._d32[s][:n])
            if d16 is not None:
                d16[lo:lo + n].copy_(self._d16[s][:n])

        self._walk(visit)
        return self._hand_state(BruteForceIndex._from_buffers(d32, d16, self.dmax_norm, self.idx_offset, self.screen_masked))

    def _hand_state(self, index: "BruteForceIndex") -> "BruteForceIndex":
        """resident(): copies of the keep-bitmask, tags, biases and group ids, in the layouts the two classes share."""
        for name in ("_keep", "_tags", "_bias", "_groups"):
            t = getattr(self, name)
            setattr(index, name, None if t is None else t.clone())
        return index

    @property
    def ntotal(self) -> int:
        return self.N

    @property
    def keep_mask(self) -> Optional[torch.Tensor]:
        """The persistent keep-bitmask over the whole corpus (int32 [ceil(N/32)], on the device), or None."""
        return self._keep

    def remove_ids(self, ids) -> None:
        """Withdraw documents by global id (with idx_offset); other ids are ignored.  The mask stays on the device."""
        self._keep = _clear_ids(self._keep, self.N, self.device, ids, self.idx_offset)

    def _check_q(self, q: torch.Tensor) -> None:
        """The queries [B,d] of every pass of this index: on its device, of the rows' width."""
        if q.device != self.device:
            raise ValueError(f"queries on {q.device} but the index streams through {self.device}")
        if q.shape[1] != self.d:
            raise ValueError(f"shape mismatch: q {tuple(q.shape)} vs docs {(self.N, self.d)}")

    def _mask(self, keep: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
        """The mask a call runs under, over the whole corpus: the persistent one ANDed with the call's checked `keep`, or None."""
        return _and_keep(self._keep, keep, self.N, self.device)

    def _need_word_blocks(self, what: str, needed: bool = True) -> None:
        """A pass that hands every block its slice of per-row words (keep-bitmask, tags) needs blocks that start on
        32-row boundaries, unless there is one block only."""
        if needed and self.block % 32 and self.N > self.block:
            raise ValueError(f"a {what} needs block_docs to be a multiple of 32, got {self.block}")

    def _walk_topk(self, q: torch.Tensor, k: int, out, keep: Optional[torch.Tensor], block_topk: Callable):
        """The one top-k walk: block_topk(s, lo, n, keep_slice) -> (vals [B,k], idx [B,k]) is the search of the n widened rows
        from lo in buffer s under the block's words of the ANDed mask `keep`; the blocks' lists are folded into a running
        top-k with the merge kernel, an empty corpus gives padding only, and the result goes into `out` when given."""
        run = []  # the running top-k: (values, indices)

        def visit(s, lo, n):
            v, i = block_topk(s, lo, n, _keep_slice(keep, lo, n))
            run[:] = (v, i) if not run else topk_merge(torch.cat([run[0], v], 1), torch.cat([run[1], i], 1), k)

        self._walk(visit)
        if not run:
            run = _pad_pair(*_out_pair(q.shape[0], k, q.device))
        return _copied(out, run[0], run[1])

    def _score_ids(self, q: torch.Tensor, ids: torch.Tensor, keep: Optional[torch.Tensor], what: str = "ids"):
        """(scores f32 [B,C], global ids int64 [B,C], -1 where the entry yields nothing) of checked q [B,d] under the ANDed
        mask `keep` or None.  The rows are in host memory, so the gather happens there: the distinct present ids of the
        batch (one synchronising copy to the host), their rows through the staging buffers in pieces of at most block_docs
        rows, each piece scored by tt_score_ids_bf16 with the candidates' POSITIONS among the gathered rows as ids."""
        ids = _check_ids(ids, q.shape[0], self.device, what)
        dev, N = self.device, self.N
        vals = torch.full(ids.shape, float("-inf"), dtype=torch.float32, device=dev)
        if N == 0 or ids.numel() == 0:
            return vals, torch.full_like(ids, -1)
        n = ids - self.idx_offset
        ok = (ids >= 0) & (ids >= self.idx_offset) & (n >= 0) & (n < N)
        if keep is not None:  # removed or unkept ids are neutralised on the device: a bit test against the keep words
            nc = n.clamp(0, N - 1)
            ok &= ((keep[nc >> 5] >> (nc & 31).to(torch.int32)) & 1).bool()
        uniq, inv = torch.unique(torch.where(ok, n, torch.full_like(n, -1)), return_inverse=True)
        rows = uniq.cpu()  # (the one synchronisation: which rows to fetch)
        pad = int(rows.numel() > 0 and int(rows[0]) < 0)  # padding sorts first
        rows = rows[pad:]
        pos = (inv - pad).contiguous()  # the candidate's position among the gathered rows, -1 = nothing
        U = rows.numel()
        need = min(self.block, U)  # rows per pinned buffer: grown on demand, never beyond a staging buffer
        bufs = 1 if U <= self.block else 2
        with self._ordered() as cur:  # (the pinned buffers are the object's too: the lock is held until their copies are out)
            if self._gather is None or self._gather[0].shape[0] < need or len(self._gather) < bufs:
                self._gather = [torch.empty((need, self.d), dtype=torch.bfloat16).pin_memory() for _ in range(bufs)]
            for s in range(2):
                self._free[s].record(cur)
            for j, p0 in enumerate(range(0, U, self.block)):
                s = j % 2
                m = min(self.block, U - p0)
                if j >= 2:
                    self._ready[s].synchronize()  # the copy out of this pinned buffer two pieces ago has finished
                torch.index_select(self.host, 0, rows[p0:p0 + m], out=self._gather[s][:m])
                piece = vals if U <= self.block else torch.empty_like(vals)  # (a single piece writes the result itself)
                self._staged(s, self._gather[s][:m], cur,  # (positions outside the piece: padding)
                             lambda staged, _: _score_ids_into(q, staged, pos, p0, None, piece, None))
                if piece is not vals:
                    vals = torch.maximum(vals, piece)
            if U:
                self._ready[(U - 1) // self.block % 2].synchronize()  # (the pinned buffers are reusable when this returns)
        return vals, torch.where(ok, ids, torch.full_like(ids, -1))

    def score_ids(self, q: torch.Tensor, ids: torch.Tensor, keep: Optional[torch.Tensor] = None) -> torch.Tensor:
        """float32 [B,C] ([C] for a single query): the exact dense score of every id of ids int64 [B,C] on the device (global
        ids, with idx_offset), -inf where the id is negative, outside the corpus, removed or not kept by `keep` (a mask over
        the whole corpus): the resident bf16 index's values.  Traffic is at most B*C rows instead of the N-row walk.
        SYNCHRONISES with the host once: the distinct ids of the batch are copied to the host, where their rows are
        gathered (index_select from the pinned corpus) and sent through the staging buffers in pieces of block_docs rows."""
        _need_cuda(q)
        if q.dim() == 1:
            return self.score_ids(q.unsqueeze(0), _ids_row(ids), keep)[0]
        self._check_q(q)
        return self._score_ids(_f32c(q), ids, self._mask(keep))[0]

    def search(self, q: torch.Tensor, k: int = 10, out=None, keep: Optional[torch.Tensor] = None,
               exclude: Optional[torch.Tensor] = None, candidates: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """out: optional (vals f32 [B,k], idx int64 [B,k]) device tensors to write the result into (ShardedIndex's send block).
        candidates: optional per-query candidate lists of global ids, int64 [B,C] on the device ([C] with a 1-D q): no walk --
        the candidates' rows are gathered on the host and scored (score_ids: it synchronises with the host once), then
        merged: the exact top-k of the distinct, present candidates.
        exclude: optional per-query exclusion lists of global ids, int64 [B,E] on the device ([E] with a 1-D q): the blocks are
        searched and merged for k + E (<= 1024) and the running list is filtered once at the end (tt_topk_exclude_ids).
        keep: optional packed keep-bitmask over the whole corpus (on the device), ANDed with the mask of remove_ids.  Block i of
        a masked search gets the word slice at lo / 32 and runs the masked exact kernel (the masked screen where the block
        screens and screen_masked is set), so the blocks must start on word boundaries: block_docs % 32 != 0 (with more than
        one block) raises ValueError."""
        _need_cuda(q)
        if q.dim() == 1:
            return _squeezed(self.search, q, k, None, keep, _exclude_row(exclude), _ids_row(candidates, "candidates"))
        self._check_q(q)
        if exclude is not None:
            exclude, kk = _check_exclude(exclude, q.shape[0], k, self.device)
            v, i = self.search(q, kk, None, keep, None, candidates)
            return topk_exclude(v, i, exclude, k, out)
        q = _f32c(q)
        keep = self._mask(keep)
        if candidates is not None:
            return _merge_candidates(*self._score_ids(q, candidates, keep, "candidates"), k, out)
        self._need_word_blocks("masked StreamedIndex search", keep is not None)

        def block_topk(s, lo, n, keep_words):  # the block as a resident index of its own: it screens where it can
            blk = BruteForceIndex._from_buffers(self._d32[s][:n], self._d16[s][:n] if self._d16[s] is not None else None,
                                                self.dmax_norm, self.idx_offset + lo, self.screen_masked)
            return blk.search(q, k, keep=keep_words)

        return self._walk_topk(q, k, out, keep, block_topk)

    @property
    def tags(self) -> Optional[torch.Tensor]:
        """The tags of the whole corpus, on the device (int32 [32*ceil(N/32)], zero padding beyond N), or None: not set."""
        return self._tags

    def set_tags(self, tags: torch.Tensor) -> None:
        """One 32-bit tag per row of the whole corpus (int32 [N] or padded to [32*ceil(N/32)]), on the index's DEVICE: the rows
        stream from the host, the tags stay resident at 4 bytes per row (N/8 bytes for a keep-bitmask, next to 2 N d of rows
        that do not fit)."""
        self._tags = _check_tags(tags, self.N, self.device)

    def tagged_search(self, q: torch.Tensor, k: int = 10, match_mask=0xffffffff, match_value=0,
                      keep: Optional[torch.Tensor] = None, out=None) -> Tuple[torch.Tensor, torch.Tensor]:
        """search() with a filter per query (BruteForceIndex.tagged_search; k <= 64): every streamed block runs the tagged
        exact kernel under its slice of the tags (and of the ANDed keep-bitmask, if any), and the blocks' lists are merged as
        in search().  A tile of 32 tags belongs to one block, so the blocks must start on multiples of 32 rows:
        block_docs % 32 != 0 (with more than one block) raises ValueError."""
        if self._tags is None:
            raise ValueError("tagged_search: this index has no tags (set_tags)")
        if q.dim() == 1:
            return _squeezed(self.tagged_search, q, k, match_mask, match_value, keep)
        _need_cuda(q)
        self._check_q(q)
        _TAGGED.check_k(k)
        q = _f32c(q)
        B = q.shape[0]
        mm = _match_words(match_mask, B, self.device, "match_mask")
        mv = _match_words(match_value, B, self.device, "match_value")
        keep = self._mask(keep)
        self._need_word_blocks("tagged StreamedIndex search")

        def block_topk(s, lo, n, keep_words):
            if lo % 32:
                raise ValueError(f"block at row {lo}: the tags of a 32-document tile belong to one block")
            return _mode_into(_TAGGED, q, self._d32[s][:n], (self._tags[lo:lo + _tag_words(n)], mm, mv), keep_words, k,
                              self.idx_offset + lo)

        return self._walk_topk(q, k, out, keep, block_topk)

    @property
    def bias(self) -> Optional[torch.Tensor]:
        """The biases of the whole corpus, on the device (float32 [32*ceil(N/32)], zero padding beyond N), or None: not set."""
        return self._bias

    def set_bias(self, bias: Optional[torch.Tensor]) -> None:
        """One float32 bias per row of the whole corpus (float32 [N] or padded to [32*ceil(N/32)]), on the index's DEVICE: the
        rows stream from the host, the biases stay resident at 4 bytes per row.  Checked for NaN and infinities once, here
        (ValueError; a host synchronisation).  None clears it."""
        self._bias = _set_bias(bias, self.N, self.device)

    def biased_search(self, q: torch.Tensor, k: int = 10, keep: Optional[torch.Tensor] = None,
                      out=None) -> Tuple[torch.Tensor, torch.Tensor]:
        """search() ranked by q.d + bias[n] (BruteForceIndex.biased_search; k <= 64): every streamed block runs the biased exact
        kernel under its slice of the biases (and of the ANDed keep-bitmask, if any), and the blocks' lists -- biased values --
        are merged as in search().  A block that starts on a multiple of 32 rows reads its slice in place; with a block_docs
        that is no multiple of 32 every block takes a padded copy of its slice (4 bytes per row of the block).  A keep-bitmask
        still needs whole words per block: keep with block_docs % 32 != 0 (and more than one block) raises ValueError."""
        if self._bias is None:
            raise ValueError("biased_search: this index has no bias (set_bias)")
        if q.dim() == 1:
            return _squeezed(self.biased_search, q, k, keep)
        _need_cuda(q)
        self._check_q(q)
        _BIASED.check_k(k)
        q = _f32c(q)
        keep = self._mask(keep)
        self._need_word_blocks("masked StreamedIndex search", keep is not None)

        def block_topk(s, lo, n, keep_words):
            if lo % 32 == 0:  # whole tiles from a 128-byte aligned start: read in place
                b = self._bias[lo:lo + _tag_words(n)]
            else:
                b = torch.zeros(_tag_words(n), dtype=torch.float32, device=self.device)
                b[:n] = self._bias[lo:lo + n]
            return _mode_into(_BIASED, q, self._d32[s][:n], (b,), keep_words, k, self.idx_offset + lo)

        return self._walk_topk(q, k, out, keep, block_topk)

    def _cursor_device(self) -> torch.device:
        return self.device

    def _search_after(self, q: torch.Tensor, k: int, av: torch.Tensor, ai: torch.Tensor, keep: Optional[torch.Tensor], out=None):
        """search_after (_CursorSearch) over the streamed rows: every block runs the exact kernel in its cursor mode under
        the same global cursor (and its slice of the ANDed keep-bitmask, if any), and the blocks' lists are merged as in
        search().  A keep-bitmask needs whole words per block, as in search()."""
        self._check_q(q)
        _AFTER.check_k(k, hint=False)  # (this class's refusal has always read without the pages() hint: the words stay)
        q = _f32c(q)
        keep = self._mask(keep)
        self._need_word_blocks("masked StreamedIndex search", keep is not None)
        return self._walk_topk(q, k, out, keep, lambda s, lo, n, keep_words: _mode_into(
            _AFTER, q, self._d32[s][:n], (av, ai), keep_words, k, self.idx_offset + lo))

    def _candidate_rows(self, ids: torch.Tensor) -> torch.Tensor:
        """float32 [B,C,d]: the rows of the global ids this index owns (bf16 widened exactly), zeros elsewhere.  The rows are
        in host memory: one synchronising copy of the ids to the host, index_select there into pinned staging, one copy back."""
        n = ids - self.idx_offset
        own = (ids >= 0) & (n >= 0) & (n < self.N)
        if self.N == 0 or ids.numel() == 0:
            return torch.zeros(tuple(ids.shape) + (self.d,), dtype=torch.float32, device=self.device)
        at = torch.where(own, n, torch.zeros_like(n)).reshape(-1).cpu()  # (the one synchronisation: which rows to fetch)
        staged = torch.empty((at.numel(), self.d), dtype=torch.bfloat16).pin_memory()
        torch.index_select(self.host, 0, at, out=staged)
        rows = staged.to(self.device, non_blocking=True).to(torch.float32).view(tuple(ids.shape) + (self.d,))
        return rows.masked_fill_(~own.unsqueeze(-1), 0.0)

    def diverse_search(self, q: torch.Tensor, k: int = 10, lambda_: float = 0.5, fetch_k: Optional[int] = None,
                       keep: Optional[torch.Tensor] = None, exclude: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        if q.dim() == 1:
            return _squeezed(self.diverse_search, q, k, lambda_, fetch_k, keep, _exclude_row(exclude))
        fk, lam = _mmr_fetch_k(k, fetch_k), _check_lambda(lambda_)
        v, i = self.search(q, fk, keep=keep, exclude=exclude)
        return mmr_select(v, i, None, k, lam, rows=self._candidate_rows(i))

    diverse_search.__doc__ = _DIVERSE_DOC + """
        Streamed: the walk for fetch_k, then -- SYNCHRONISING with the host once, like score_ids -- the candidates' ids are
        copied to the host, their rows gathered there (index_select from the pinned corpus into pinned staging), sent to the
        device (B * fetch_k * d * 2 bytes), widened exactly and selected from (tt_mmr_select_rows_f32): the resident bf16
        index's result."""

    @property
    def groups(self) -> Optional[torch.Tensor]:
        """The group ids of the whole corpus, on the device (int64 [N]; negative = ungrouped), or None: not set."""
        return self._groups

    def set_groups(self, groups: Optional[torch.Tensor]) -> None:
        """One int64 group id per row of the whole corpus (int64 [N]), on the index's DEVICE: the rows stream from the host, the
        group table stays resident at 8 bytes per row.  None clears it."""
        self._groups = None if groups is None else _check_groups(groups, self.N, self.device)

    def collapsed_search(self, q: torch.Tensor, k: int = 10, max_per_group: int = 1, fetch_k: Optional[int] = None,
                         keep: Optional[torch.Tensor] = None, exclude: Optional[torch.Tensor] = None, exact: bool = True):
        return _collapsed_search(self, q, k, max_per_group, fetch_k, keep, exclude, exact, self._groups, self.N, self.idx_offset,
                                 self.device, self.N)

    collapsed_search.__doc__ = _COLLAPSED_DOC + """
        Streamed: every round is one walk over the host rows; a masked round needs block_docs to be a multiple of 32 like
        every masked search of this class."""

    def count(self, q: torch.Tensor, min_score, keep: Optional[torch.Tensor] = None) -> torch.Tensor:
        """int64 [B] (0-d for a single query): the documents of the whole corpus (not removed, kept by `keep`: a mask over the
        whole corpus, on the device) scoring at least min_score.  The walk counts every block with the counting pass, adding
        into one tensor (accumulate) under the block's slice of the mask; masked, block_docs must be a multiple of 32 as in
        search().  The blocks are the widened fp32 rows (bf16 -> fp32 is exact): the count of the resident index."""
        _need_cuda(q)
        if q.dim() == 1:
            return self.count(q.unsqueeze(0), min_score, keep)[0]
        self._check_q(q)
        q = _f32c(q)
        thr = _min_score(min_score, q.shape[0], self.device)
        keep = self._mask(keep)
        self._need_word_blocks("masked StreamedIndex count", keep is not None)
        counts = torch.zeros(q.shape[0], dtype=torch.int64, device=self.device)
        self._walk(lambda s, lo, n: _count_into(q, self._d32[s][:n], thr, _keep_slice(keep, lo, n), counts, True))
        return counts

    def range_search(self, q: torch.Tensor, min_score, k: int = 10, keep: Optional[torch.Tensor] = None):
        return _range_search(self, q, min_score, k, keep)

    range_search.__doc__ = _RANGE_DOC + """
        Streamed: two walks over the host rows, one for the rows and one for the counts."""
