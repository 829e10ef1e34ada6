"""Hard-negative mining against an index: the k best documents that score at most a ceiling derived from the query's own
positives, and are not positives themselves (positive-aware mining: a document that outscores the positive by more than the
rule allows is more likely an unlabelled positive than a useful negative).

One score_ids call for the positives' scores, one cursor search (search_after with the cursor (ceiling, -1) and the positives
as its exclusion list) for the negatives: one pass over the rows, no [B,N] matrix.  Everything runs through libtt.so."""
from __future__ import annotations

from typing import Optional, Tuple

import torch

__all__ = ["mine_hard_negatives", "negatives_ceiling"]


def negatives_ceiling(pos_scores: torch.Tensor, pos_ids: torch.Tensor, margin: float = 0.0, ratio: Optional[float] = None) -> torch.Tensor:
    """float32 [B]: the score ceiling of each query's negatives.  pos_scores float32 [B,P] are the scores of pos_ids int64
    [B,P]; an entry is a valid positive when its id is not negative (padding) and the index gave it a score (-inf: not in the
    index, removed or not kept).  ceiling[b] = (the smallest score of b's valid positives) - margin, or, with `ratio`, that
    smallest score times ratio -- one rule or the other, in float32.  A query without a valid positive gets +inf: no ceiling."""
    if ratio is not None and margin != 0.0:
        raise ValueError("mine_hard_negatives: margin and ratio are two rules for one ceiling, give one of them")
    if ratio is not None and not ratio > 0.0:
        raise ValueError(f"mine_hard_negatives: ratio must be positive, got {ratio}")
    if pos_scores.shape != pos_ids.shape or pos_scores.dim() != 2:
        raise ValueError(f"pos_ids must be [B,P], got {tuple(pos_ids.shape)} with scores {tuple(pos_scores.shape)}")
    inf = torch.full_like(pos_scores, float("inf"))
    valid = (pos_ids >= 0) & (pos_scores > float("-inf"))
    if pos_scores.shape[1] == 0:
        return inf.new_full((pos_scores.shape[0],), float("inf"))
    smallest = torch.where(valid, pos_scores, inf).amin(dim=1)
    return smallest * ratio if ratio is not None else smallest - margin


def mine_hard_negatives(index, q: torch.Tensor, pos_ids: torch.Tensor, k: int, margin: float = 0.0, ratio: Optional[float] = None,
                        keep: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """(vals [B,k], ids [B,k]): for each query the k best documents of `index` (a BruteForceIndex, StreamedIndex or
    ShardedIndex) that score at most its ceiling and are none of its positives, (score desc, index asc), tail (-inf, -1).
    q [B,d] (or [d] with pos_ids [P]); pos_ids int64 [B,P] GLOBAL ids on the index's device, negative entries are padding.
    The positives' scores come from index.score_ids; ceiling = min over the valid positives - margin, or min * ratio
    (negatives_ceiling; e.g. ratio = 0.95 keeps negatives below 95 % of the positive's score).  A query without a valid
    positive gets the plain top-k.  k + P <= 64.  keep: as in search().  On a ShardedIndex a COLLECTIVE: every rank calls it
    with the same q and pos_ids and gets the same result.  The ids go back to the trainer as the `n` of a triplet step or as
    rows of a negatives pool (trainer.py)."""
    if q.dim() == 1:
        if pos_ids.dim() != 1:
            raise ValueError(f"a single query takes pos_ids [P], got {tuple(pos_ids.shape)}")
        v, i = mine_hard_negatives(index, q.unsqueeze(0), pos_ids.unsqueeze(0), k, margin, ratio, keep)
        return v[0], i[0]
    if pos_ids.dtype != torch.int64 or pos_ids.dim() != 2 or pos_ids.shape[0] != q.shape[0]:
        raise ValueError(f"pos_ids must be int64 [B,P] = [{q.shape[0]},P], got {pos_ids.dtype} {tuple(pos_ids.shape)}")
    if ratio is not None and margin != 0.0:  # (before any launch or collective)
        raise ValueError("mine_hard_negatives: margin and ratio are two rules for one ceiling, give one of them")
    if pos_ids.shape[1] == 0:
        return index.search_after(q, k, None, keep=keep)
    ceiling = negatives_ceiling(index.score_ids(q, pos_ids, keep=keep), pos_ids, margin, ratio)
    return index.search_after(q, k, after=(ceiling, -1), keep=keep, exclude=pos_ids)
