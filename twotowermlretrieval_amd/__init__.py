"""MI355X-native (gfx950) implementation of the two-tower retrieval hot path of
jpe17/TwoTowerMLRetrieval: fused brute-force scoring + top-k, GRU encoder towers,
triplet-loss training.  Python host over a C-ABI HIP library (libtt.so, include/tt.h)."""
from . import collective, evaluators, hybrid, lexical, mining, model, query_inferencer, tokenizer, trainer
from .index import (BruteForceIndex, GraphedSearch, PendingSearch, ShardedIndex, StreamedIndex, l2_bias, l2_distances, mmr_select, pack_keep_mask, score_all, score_count, score_ids, score_rank, score_topk,
                    score_topk_after, score_topk_biased, score_topk_tagged, shard_bounds, topk_collapse, topk_cut_below, topk_exclude, topk_merge)
from .mining import mine_hard_negatives
from .lexical import LexicalIndex, lexical_score_all, lexical_score_topk
from .hybrid import HybridSearcher, SimpleHybridRetriever
from . import fusion
from .fusion import HybridIndex, fuse_topk, fused_search, rrf_weights
from .model import (LogitScale, RNNEncoder, TwoTowerModel, contrastive_softmax_loss, distillation_targets, in_batch_softmax_loss, multi_positive_targets,
                    soft_contrastive_loss, symmetric_contrastive_losses, triplet_loss_cosine)
from .query_inferencer import QueryInferencer
from .tokenizer import PretrainedTokenizer
from .trainer import DataParallelTrainer, FusedClipAdam, GraphedTrainStep, train_step

__all__ = ["BruteForceIndex", "GraphedSearch", "ShardedIndex", "PendingSearch", "StreamedIndex", "score_topk", "topk_merge", "topk_exclude", "topk_collapse", "score_rank", "score_all", "score_ids", "mmr_select", "shard_bounds", "pack_keep_mask", "score_count", "topk_cut_below", "score_topk_tagged", "score_topk_biased", "l2_bias", "l2_distances", "score_topk_after", "mine_hard_negatives", "mining",
           "LexicalIndex", "lexical_score_topk", "lexical_score_all", "lexical",
           "HybridIndex", "fuse_topk", "fused_search", "rrf_weights", "fusion",
           "RNNEncoder", "TwoTowerModel", "triplet_loss_cosine", "in_batch_softmax_loss", "contrastive_softmax_loss", "soft_contrastive_loss", "symmetric_contrastive_losses", "LogitScale", "distillation_targets", "multi_positive_targets", "QueryInferencer", "PretrainedTokenizer", "HybridSearcher", "SimpleHybridRetriever",
           "FusedClipAdam", "DataParallelTrainer", "train_step", "GraphedTrainStep", "model", "trainer", "tokenizer", "query_inferencer",
           "evaluators", "hybrid", "collective"]
__version__ = "0.1.0"
