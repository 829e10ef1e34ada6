"""Drop-in mirror of the reference's backend/model.py public surface, computed by libtt.so.

    RNNEncoder(vocab_size, embed_dim, hidden_dim, pretrained_embeddings=None, rnn_type='GRU',
               num_layers=1, dropout=0.0, bidirectional=False, normalize_output=True)   model.py:11-46
    RNNEncoder.forward(LongTensor[B,T]) -> FloatTensor[B,H]                              model.py:48-75
    TwoTowerModel(config, pretrained_embeddings).encode_query / encode_document / forward model.py:78-106
    triplet_loss_cosine((q, p, n), margin=0.2) -> 0-d tensor                             model.py:109-114
    in_batch_softmax_loss((q, p, n), temperature=0.05) -> 0-d tensor                     (not in the reference: in-batch negatives)
    contrastive_softmax_loss(q, docs, pos_offset=0, temperature=0.05) -> 0-d tensor      (the same over any pool of documents)
    ... both with group labels (groups=, neg_groups= / q_groups=, doc_groups=): a passage that carries a query's label, other
    than its own positive, is no negative of it
    ... and with symmetric=alpha in (0, 1]: the bidirectional (CLIP-style) loss, each positive also classified among the queries;
    symmetric_contrastive_losses(q, docs, ...) -> (L_qd, L_dq) reports the two directions
    soft_contrastive_loss(q, docs, targets, temperature=0.05) -> 0-d tensor              (the same softmax against a weight per pair:
    distillation_targets(teacher_scores, ...), multi_positive_targets(q_groups, doc_groups, pos_offset) make the weights)
    LogitScale(temperature=0.05, min_temperature=0.01, max_temperature=1.0, learnable=True)  a temperature on the device, for
    every `temperature=` above: learned (the kernels return its gradient) or a word a schedule rewrites

Same constructor arguments, attribute names (`query_encoder.embedding.embedding_dim` is read by
backend/main.py:104) and state_dict keys ({query,doc}_encoder.{embedding.weight,
rnn.weight_ih_l0[_reverse], ..., projection.weight/bias}), so a model.pth written by either side
loads in the other.  The nn.Module objects here only OWN the parameters; every forward/backward
runs in hand-written HIP kernels (csrc/encoder*.hip, gru16.hip, train.hip, in_batch_loss.hip).  There is no PyTorch fallback:
CPU tensors raise.  RNN_TYPE GRU, LSTM and RNN (tanh) are the three the reference's getattr(nn, ...) accepts.
"""
from __future__ import annotations

import ctypes as C
import math
import threading
from typing import Dict, Optional, Tuple

import numpy as np
import torch
import torch.nn as nn

from . import _lib

__all__ = ["RNNEncoder", "TwoTowerModel", "triplet_loss_cosine", "in_batch_softmax_loss", "contrastive_softmax_loss", "soft_contrastive_loss",
           "symmetric_contrastive_losses", "LogitScale",
           "distillation_targets", "multi_positive_targets", "SplitRecurrenceTimeout"]


class SplitRecurrenceTimeout(RuntimeError):
    """Status bit 2: a column-split GRU recurrence (csrc/gru16x4.hip) gave up waiting for a partner workgroup -- a transient
    condition of the device (CUs held by other work), not of the data.  The call's outputs are invalid; the same call with
    `one_workgroup` recurrences (TT_ENC_ONE_WORKGROUP) cannot time out and returns the same bits.  RNNEncoder's inference
    forward and trainer.train_step redo the call that way themselves; this exception reaches the caller of a hand-written
    autograd loop only."""


def _stream(dev) -> int:
    return torch.cuda.current_stream(dev).cuda_stream


_PREP_LOCK = threading.Lock()  # module level: nn.Module instances must stay deep-copyable / picklable

_CELLS = {"GRU": (0, 3), "LSTM": (1, 4), "RNN": (2, 1)}  # RNN_TYPE -> (C-ABI rnn_type, gate rows / H)


class _GRUParams(nn.Module):
    """Parameter container with torch.nn.GRU's / nn.LSTM's / nn.RNN's names, shapes (gates * H rows) and default init
    (U(-1/sqrt(H), 1/sqrt(H)))."""

    def __init__(self, input_size: int, hidden_size: int, num_layers: int, bidirectional: bool, gates: int = 3):
        super().__init__()
        self.input_size, self.hidden_size = input_size, hidden_size
        self.num_layers, self.bidirectional = num_layers, bidirectional
        k = 1.0 / math.sqrt(hidden_size)
        ndir = 2 if bidirectional else 1
        for layer in range(num_layers):
            I = input_size if layer == 0 else ndir * hidden_size
            for d in range(ndir):
                sfx = f"_l{layer}" + ("_reverse" if d else "")
                for name, shape in (("weight_ih", (gates * hidden_size, I)), ("weight_hh", (gates * hidden_size, hidden_size)),
                                    ("bias_ih", (gates * hidden_size,)), ("bias_hh", (gates * hidden_size,))):
                    self.register_parameter(name + sfx, nn.Parameter(torch.empty(shape).uniform_(-k, k)))

    def quads(self):
        """[(W_ih, W_hh, b_ih, b_hh)] ordered (layer, dir): the order of the C ABI's `weights` array."""
        out = []
        for layer in range(self.num_layers):
            for d in range(2 if self.bidirectional else 1):
                sfx = f"_l{layer}" + ("_reverse" if d else "")
                out.append(tuple(getattr(self, n + sfx) for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")))
        return out


class _LinearParams(nn.Module):
    """Parameter container with nn.Linear's names and default init."""

    def __init__(self, in_features: int, out_features: int):
        super().__init__()
        k = 1.0 / math.sqrt(in_features)
        self.in_features, self.out_features = in_features, out_features
        self.weight = nn.Parameter(torch.empty(out_features, in_features).uniform_(-k, k))
        self.bias = nn.Parameter(torch.empty(out_features).uniform_(-k, k))


def _ptr_array(tensors):
    arr = (C.c_void_p * len(tensors))()
    for i, t in enumerate(tensors):
        arr[i] = t.data_ptr()
    return arr


class deferred_input_checks:
    """Context manager: the encoders' per-call status reads (one D2H sync each) are collected instead and checked
    ONCE on exit, so independent tower calls can be enqueued back to back on several streams.  The same exceptions
    are raised, only later: after all the towers of a step have been launched, before anything consumes them."""

    def __init__(self, *encoders: "RNNEncoder"):
        self.encoders = encoders

    def __enter__(self):
        self._box = []
        for e in self.encoders:
            e._deferred_status = self._box
        return self

    def __exit__(self, exc_type, exc, tb):
        for e in self.encoders:
            e._deferred_status = None
        if exc_type is None and self._box:
            _raise_status(_or_all(self._box))
        return False


def _or_all(status_tensors) -> int:
    acc = 0
    for v in torch.cat([s.reshape(1) for s in status_tensors]).tolist():  # one D2H copy for all of them
        acc |= int(v)
    return acc


def _raise_status(status: int) -> None:
    """Data errors first (they are properties of the batch: the reference's exceptions), the transient time-out last."""
    if status & 2:
        raise IndexError("index out of range in self")  # nn.Embedding's message (tests/golden/g10_errors.json)
    if status & 1:
        raise RuntimeError("Length of all samples has to be greater than 0, but found an element in 'lengths' "
                           "that is <= 0")  # pack_padded_sequence's message (model.py:55-57)
    if status & 4:
        raise SplitRecurrenceTimeout("libtt: a column-split GRU recurrence gave up waiting for a partner workgroup (bounded "
                                     "hand-off sweep, csrc/gru16x4.hip); the call's outputs are invalid.  Set "
                                     "encoder.one_workgroup = True (TT_ENC_ONE_WORKGROUP) and call again: same bits, no hand-off")


class _EncoderFn(torch.autograd.Function):
    """forward = tt_encoder_forward_f32 (train=1), backward = tt_encoder_backward_f32."""

    @staticmethod
    def forward(ctx, enc: "RNNEncoder", ids: torch.Tensor, *params: torch.Tensor):
        p = enc.dropout if enc.training else 0.0
        # the mask stream is seeded from torch's default CPU generator (torch.manual_seed reproduces it)
        seed = int(torch.randint(0, 2 ** 62, (1,)).item()) if p > 0.0 else 0
        # a status word handed to a watching optimizer is read in its step(), behind the backward; one that was checked here (or
        # at the end of a deferred_input_checks block) is re-read behind the backward for the backward's time-out bit
        ctx.handed_over = enc.check_inputs and enc._deferred_status is None and enc._status_sink is not None
        out, ws, status = enc._run_forward(ids, train=True, dropout_p=p, dropout_seed=seed)
        ctx.enc, ctx.ids, ctx.ws, ctx.status = enc, ids, ws, status
        ctx.dropout = (p, seed)
        ctx.opts = enc._opts_bwd()
        ctx.n_params = len(params)
        return out

    @staticmethod
    def backward(ctx, d_out: torch.Tensor):
        enc = ctx.enc
        grads = enc._run_backward(ctx.ids, ctx.ws, d_out.contiguous(), *ctx.dropout, status=ctx.status, opts=ctx.opts)
        ctx.ws = None
        if enc.check_inputs and not ctx.handed_over and enc._backward_may_time_out(ctx.ids.shape[0], ctx.opts):
            # the backward ORs bit 2 into the forward's word (include/tt.h); nobody else reads it on this path
            _raise_status(int(ctx.status.item()) & 4)
        return (None, None, *grads)


class RNNEncoder(nn.Module):
    """Text encoder: embedding gather -> (stacked / bidirectional) GRU | LSTM | RNN -> final hidden -> L2-normalise."""

    def __init__(self, vocab_size: int, embed_dim: int, hidden_dim: int,
                 pretrained_embeddings: Optional[np.ndarray] = None, rnn_type: str = "GRU", num_layers: int = 1,
                 dropout: float = 0.0, bidirectional: bool = False, normalize_output: bool = True, arith: str = "split16"):
        """The reference's signature (backend/model.py:11-22) plus `arith`: "split16" (default: GRU towers with H = 128 / 256
        take every product as three f16 MFMAs on fp16 hi/lo splits, fp32-grade) or "f32" (every product on the fp32-MFMA
        kernels: nn.GRU's own fp32 arithmetic, include/tt.h TT_ENC_F32; also settable later as `encoder.arith`)."""
        super().__init__()
        if arith not in ("split16", "f32"):
            raise ValueError(f"arith={arith!r} (supported: 'split16', 'f32')")
        self.arith = arith
        self.embedding = nn.Embedding(vocab_size, embed_dim, padding_idx=0)  # parameter owner only
        if pretrained_embeddings is not None:
            # every row is copied, row 0 included (it is the GloVe word "the"), and the table is frozen
            self.embedding.weight.data.copy_(torch.from_numpy(np.asarray(pretrained_embeddings)))
            self.embedding.weight.requires_grad = False
        self.rnn_type = rnn_type.upper()
        if self.rnn_type not in _CELLS:  # the reference's getattr(nn, rnn_type.upper()) accepts exactly these three
            raise AttributeError(f"module 'torch.nn' has no attribute {self.rnn_type!r} usable as RNN_TYPE "
                                 "(supported: GRU, LSTM, RNN)")
        self._cell, gates = _CELLS[self.rnn_type]
        self.bidirectional = bidirectional
        self.num_layers = num_layers
        self.hidden_dim = hidden_dim
        self.dropout = float(dropout) if num_layers > 1 else 0.0
        self.rnn = _GRUParams(embed_dim, hidden_dim, num_layers, bidirectional, gates)
        self.normalize_output = normalize_output
        self.projection = _LinearParams(hidden_dim * 2, hidden_dim) if bidirectional else None
        self.check_inputs = True  # read the device status word after each call (one 4-byte D2H sync)
        # inference keeps the weights in kernel form (tt_encoder_prepare_f32) until they change: see _prepared_weights
        self.cache_prepared = True
        self._prep: dict = {}
        # inference, layer 0: the input projection of EVERY vocabulary row, computed once per weight version (the projected
        # table, include/tt.h: tt_encoder_project_table_f32) and gathered by the recurrence kernels, instead of a GEMM over the
        # batch's tokens in every call.  None = when it pays and is safe by construction: the table is frozen (GloVe loaded,
        # backend/model.py:25-27), the configuration has one (GRU, H = 128 / 256) and it fits PROJECTED_MAX_BYTES
        # (V x 3H x 4 bytes per direction: 1.23 GB for the north-star tower).  True / False force it on (any table: its version
        # counter is part of the cache key) / off.  Results are bit-identical either way.
        self.projected_table: Optional[bool] = None
        self._proj: dict = {}
        self._deferred_status = None  # a list while a caller (trainer.train_step) batches the status reads
        # a list owned by an optimizer that watches this encoder (FusedClipAdam.watch): TRAINING calls hand their status words
        # over instead of raising here, and optimizer.step() decides -- together with the other ranks -- whether the step happens
        self._status_sink = None
        # keep every recurrence of this encoder's calls on the one-workgroup kernels (TT_ENC_ONE_WORKGROUP, include/tt.h)
        self.one_workgroup = False
        self.one_workgroup_bwd = None  # None: as one_workgroup; True / False: the reverse-time recurrence alone (any mix is valid)

    # ---- plumbing ---------------------------------------------------------------
    def __getstate__(self):
        """copy.deepcopy / pickling of the module leave the per-device caches behind (kernel-form weights, the 1.2 GB projected
        table): the copy derives its own on first use."""
        state = self.__dict__.copy()
        state["_prep"], state["_proj"] = {}, {}
        return state

    def _flat_params(self):
        ps = [w for quad in self.rnn.quads() for w in quad]
        if self.projection is not None:
            ps += [self.projection.weight, self.projection.bias]
        return ps

    def _arith_bit(self) -> int:
        return _lib.TT_ENC_F32 if self.arith == "f32" else 0

    def _opts(self) -> int:
        return (_lib.TT_ENC_ONE_WORKGROUP if self.one_workgroup else 0) | self._arith_bit()

    def _opts_bwd(self) -> int:
        one = self.one_workgroup if self.one_workgroup_bwd is None else self.one_workgroup_bwd
        return (_lib.TT_ENC_ONE_WORKGROUP if one else 0) | self._arith_bit()

    def split_workgroups(self, B: int) -> int:
        """CUs the column-split recurrence of a B-row call of this encoder occupies (0: it runs the one-workgroup kernels)."""
        if self.arith == "f32":
            return 0
        return _lib.lib().tt_encoder_split_workgroups(int(B), self.hidden_dim, int(self.bidirectional), self._cell)

    def _backward_may_time_out(self, B: int, opts: int) -> bool:
        if opts & (_lib.TT_ENC_ONE_WORKGROUP | _lib.TT_ENC_F32):
            return False
        return _lib.lib().tt_encoder_split_workgroups(B, self.hidden_dim, int(self.bidirectional), self._cell) > 0

    def _check_device(self, x: torch.Tensor):
        if not x.is_cuda:
            raise RuntimeError("twotowermlretrieval_amd.RNNEncoder runs only on an AMD GPU via libtt.so "
                               f"(got ids on {x.device}; there is no CPU fallback)")
        for p in self.parameters():
            if p.device != x.device:
                raise RuntimeError(f"parameter on {p.device} but ids on {x.device}: call model.to(device) first")
            if p.dtype != torch.float32:
                raise TypeError("parameters must be float32")

    def invalidate_prepared(self) -> None:
        """Drop the cached kernel-form weights.  The cache is keyed on every weight's (address, tensor version counter), so
        in-place torch ops ON THE PARAMETER (`w.mul_()`, `w.copy_()` under no_grad), load_state_dict, .to() and
        FusedClipAdam.step / DataParallelTrainer.broadcast_parameters are noticed by themselves.  NOT noticed -- call this
        afterwards: writes through `w.data` (`w.data.copy_(...)` leaves the counter alone), through another view of the same
        storage (an optimizer's flat buffer: FusedClipAdam.mark_params_changed does the bump for its own), or through raw
        pointers."""
        self._prep = {}
        self._proj = {}

    PROJECTED_MAX_BYTES = 8 << 30

    def _projected_table(self, device: torch.device, quads, wptr, prepared: torch.Tensor) -> Optional[torch.Tensor]:
        """P[V, 3H] per direction = table W_ih^T + b_ih of layer 0, keyed on the table's and every weight's (address, version)."""
        if self.projected_table is False or (self.projected_table is None and self.embedding.weight.requires_grad):
            return None
        table = self.embedding.weight
        key = (table.data_ptr(), table._version) + tuple((w.data_ptr(), w._version) for w in quads)
        ent = self._proj.get(device)
        if ent is not None and ent[0] == key:
            return ent[1]
        if torch.cuda.is_current_stream_capturing():
            return None
        L = _lib.lib()
        V, E = table.shape
        need = L.tt_encoder_projected_bytes(V, E, self.hidden_dim, int(self.bidirectional), self._cell)
        if need == 0 or (self.projected_table is None and need > self.PROJECTED_MAX_BYTES):
            return None
        with _PREP_LOCK:
            ent = self._proj.get(device)
            if ent is not None and ent[0] == key:
                return ent[1]
            # (the table this one replaces is dropped here: every call records its stream on the table it reads -- _run_forward --
            #  so the caching allocator hands the 1.2 GB out again only when the calls queued on it have finished)
            self._proj.pop(device, None)
            del ent
            blob = torch.empty(need, dtype=torch.uint8, device=device)
            with torch.cuda.device(device):
                _lib.check(L.tt_encoder_project_table_f32(table.detach().data_ptr(), V, E, self.hidden_dim, self.num_layers,
                                                          int(self.bidirectional), self._cell, wptr, prepared.data_ptr(),
                                                          blob.data_ptr(), blob.numel(), _stream(device)))
                torch.cuda.current_stream(device).synchronize()  # once per weight version: any stream may read it now
            self._proj[device] = (key, blob)
        return blob

    def _prepared_weights(self, device: torch.device, quads, wptr) -> Optional[torch.Tensor]:
        """The weights converted once into what the forward kernels read (W_ih fp16 hi/lo fragment stream, packed W_hh,
        scale words): a serving process (query_inferencer.py:51-75) loads its weights once, and re-deriving them is six
        small launches, a quarter of a query-tower call.  Keyed on every weight's (address, version counter)."""
        key = tuple((w.data_ptr(), w._version) for w in quads)
        ent = self._prep.get(device)
        if ent is not None and ent[0] == key:
            return ent[1]
        if torch.cuda.is_current_stream_capturing():
            return None  # (no synchronisation inside a capture: this call derives them in its workspace)
        with _PREP_LOCK:
            ent = self._prep.get(device)
            if ent is not None and ent[0] == key:
                return ent[1]
            L = _lib.lib()
            E, H = self.embedding.weight.shape[1], self.hidden_dim
            need = L.tt_encoder_prepared_bytes(E, H, self.num_layers, int(self.bidirectional), self._cell)
            blob = torch.empty(max(need, 256), dtype=torch.uint8, device=device)
            with torch.cuda.device(device):
                _lib.check(L.tt_encoder_prepare_f32(E, H, self.num_layers, int(self.bidirectional), self._cell, wptr,
                                                    blob.data_ptr(), blob.numel(), _stream(device)))
                torch.cuda.current_stream(device).synchronize()  # once per weight version: any stream may read it now
            # the buffer it replaces stays referenced until the next replacement: calls queued on other streams may still read it
            self._prep[device] = (key, blob, ent[1] if ent is not None else None)
        return blob

    def _run_forward(self, x: torch.Tensor, train: bool, dropout_p: float = 0.0, dropout_seed: int = 0, opts: Optional[int] = None,
                     sync=None, phase: int = 0, resume=None):
        """sync: an _lib.EncSync (tt_enc_sync_t) that orders this call's recurrences against another stream's (training calls).
        phase: 0 = the whole call; _lib.TT_ENC_PHASE_BEGIN = everything in front of the first recurrence launch (returns the
        (out, ws, status) triple to pass back as `resume`); _lib.TT_ENC_PHASE_FINISH with resume = the rest (train mode only)."""
        L = _lib.lib()
        opts = self._opts() if opts is None else opts
        if isinstance(dropout_seed, torch.Tensor):   # a device int64: the kernels read the seed when they run (captured steps)
            seed_arg, opts = int(dropout_seed.data_ptr()), opts | _lib.TT_ENC_SEED_ON_DEVICE
        else:
            seed_arg = int(dropout_seed)
        ids = x.contiguous()
        if ids.dtype != torch.int64:
            ids = ids.to(torch.int64)
        if ids.dim() != 2:
            raise ValueError(f"expected ids [B,T], got {tuple(ids.shape)}")
        B, T = ids.shape
        V, E = self.embedding.weight.shape
        H = self.hidden_dim
        drop = int(train and dropout_p > 0.0 and self.num_layers > 1)
        # train = 2: the workspace also holds the gradient w.r.t. the gathered vectors (trainable embedding table)
        train_mode = (2 if self.embedding.weight.requires_grad else 1) if train else 0
        quads = [w.detach().contiguous() for quad in self.rnn.quads() for w in quad]
        wptr = _ptr_array(quads)
        prepared = self._prepared_weights(ids.device, quads, wptr) if (
            train_mode == 0 and self.cache_prepared and resume is None and not (opts & _lib.TT_ENC_F32)) else None
        projected = self._projected_table(ids.device, quads, wptr, prepared) if prepared is not None else None
        need = L.tt_encoder_workspace_bytes(B, max(T, 1), E, H, self.num_layers, int(self.bidirectional), self._cell,
                                            train_mode | (_lib.TT_ENC_PROJECTED if projected is not None else 0), drop)
        # One workspace per call, from torch's caching allocator (a cached block: microseconds).  In train mode the
        # autograd node owns it; in eval mode a per-call buffer keeps concurrent callers apart -- the reference serves
        # queries from a thread pool (frontend/main.py:103), and a buffer shared across threads or streams would be
        # overwritten by the next call's kernels while this call's are still queued.
        if resume is not None:
            out, ws, status = resume
        else:
            ws = torch.empty(max(need, 256), dtype=torch.uint8, device=ids.device)
            out = torch.empty((B, H), dtype=torch.float32, device=ids.device)
            # (not zeroed: every call that returns TT_OK WRITES the word on the stream -- include/tt.h, `status` -- and a call that
            #  does not raises below before anyone reads it; the fill was one more ~5 us launch in front of every tower call)
            status = torch.empty(1, dtype=torch.int32, device=ids.device)
        pw = self.projection.weight.detach().contiguous() if self.projection is not None else None
        pb = self.projection.bias.detach().contiguous() if self.projection is not None else None
        table = self.embedding.weight.detach()
        with torch.cuda.device(ids.device):
            if projected is not None:
                projected.record_stream(torch.cuda.current_stream(ids.device))
                _lib.check(L.tt_encoder_forward_projected_f32(
                    ids.data_ptr(), B, T, projected.data_ptr(), V, E, H, self.num_layers, int(self.bidirectional),
                    self._cell, wptr, prepared.data_ptr(), pw.data_ptr() if pw is not None else None,
                    pb.data_ptr() if pb is not None else None, int(self.normalize_output), opts, out.data_ptr(),
                    ws.data_ptr(), ws.numel(), status.data_ptr(), _stream(ids.device)))
            elif prepared is not None:
                _lib.check(L.tt_encoder_forward_prepared_f32(
                    ids.data_ptr(), B, T, table.data_ptr(), V, E, H, self.num_layers, int(self.bidirectional),
                    self._cell, wptr, prepared.data_ptr(), pw.data_ptr() if pw is not None else None,
                    pb.data_ptr() if pb is not None else None, int(self.normalize_output), opts, out.data_ptr(),
                    ws.data_ptr(), ws.numel(), status.data_ptr(), _stream(ids.device)))
            else:
                _lib.check(L.tt_encoder_forward_f32(
                    ids.data_ptr(), B, T, table.data_ptr(), V, E, H, self.num_layers, int(self.bidirectional),
                    self._cell, wptr, pw.data_ptr() if pw is not None else None,
                    pb.data_ptr() if pb is not None else None, int(self.normalize_output), train_mode | opts | phase,
                    float(dropout_p), seed_arg, out.data_ptr(), ws.data_ptr(), ws.numel(), status.data_ptr(),
                    C.byref(sync) if sync is not None else None, _stream(ids.device)))
        if phase == _lib.TT_ENC_PHASE_BEGIN:
            return out, ws, status   # (the status word is handed over / read when the FINISH half has been issued)
        if self.check_inputs:
            if self._deferred_status is not None:
                self._deferred_status.append(status)  # the caller reads them once, after enqueuing its other calls
            elif train and self._status_sink is not None:
                self._status_sink.append(status)  # the watching optimizer reads them, reduced over the ranks, in step()
            else:
                st = int(status.item())
                if (st & 7) == 4 and not train and not (opts & _lib.TT_ENC_ONE_WORKGROUP):
                    # inference: a transient time-out of the column-split recurrence and nothing wrong with the data -- the
                    # same call on the one-workgroup kernels (same bits, nothing to wait for)
                    return self._run_forward(x, train, dropout_p, dropout_seed, opts | _lib.TT_ENC_ONE_WORKGROUP, sync)
                _raise_status(st)
        return out, ws, status

    def _run_backward(self, ids: torch.Tensor, ws: torch.Tensor, d_out: torch.Tensor, dropout_p: float = 0.0,
                      dropout_seed: int = 0, into: Optional[list] = None, status: Optional[torch.Tensor] = None,
                      opts: Optional[int] = None, sync=None):
        """into: contiguous float32 tensors, one per _flat_params() entry, that receive the gradients (the C entry point
        OVERWRITES its gradient buffers): trainer.train_step hands over the optimizer's gradient views.
        status: the forward call's status word; a time-out of the column-split backward recurrence ORs bit 2 into it."""
        L = _lib.lib()
        opts = self._opts_bwd() if opts is None else opts
        if isinstance(dropout_seed, torch.Tensor):
            seed_arg, opts = int(dropout_seed.data_ptr()), opts | _lib.TT_ENC_SEED_ON_DEVICE
        else:
            seed_arg = int(dropout_seed)
        B, T = ids.shape
        V, E = self.embedding.weight.shape
        H = self.hidden_dim
        params = self._flat_params()
        grads = into if into is not None else [torch.empty_like(p, memory_format=torch.contiguous_format) for p in params]
        table = self.embedding.weight
        g_table = torch.empty_like(table, memory_format=torch.contiguous_format) if table.requires_grad else None
        nq = 4 * self.num_layers * (2 if self.bidirectional else 1)
        quads = [p.detach().contiguous() for p in params[:nq]]
        wptr, gptr = _ptr_array(quads), _ptr_array(grads[:nq])
        pw = params[nq].detach().contiguous() if self.projection is not None else None
        pb = params[nq + 1].detach().contiguous() if self.projection is not None else None
        with torch.cuda.device(ids.device):
            _lib.check(L.tt_encoder_backward_f32(
                ids.contiguous().data_ptr(), B, T, self.embedding.weight.detach().data_ptr(), V, E, H,
                self.num_layers, int(self.bidirectional), self._cell, wptr, pw.data_ptr() if pw is not None else None,
                pb.data_ptr() if pb is not None else None, int(self.normalize_output), float(dropout_p),
                seed_arg, d_out.data_ptr(), gptr,
                grads[nq].data_ptr() if pw is not None else None,
                grads[nq + 1].data_ptr() if pb is not None else None,
                g_table.data_ptr() if g_table is not None else None, ws.data_ptr(), ws.numel(), opts,
                status.data_ptr() if status is not None else None, C.byref(sync) if sync is not None else None,
                _stream(ids.device)))
        return grads + ([g_table] if g_table is not None else [])

    # ---- public -----------------------------------------------------------------
    def forward(self, x: torch.Tensor) -> torch.Tensor:
        self._check_device(x)
        params = self._flat_params()
        if self.embedding.weight.requires_grad:
            # no GloVe vectors: the reference trains nn.Embedding(padding_idx=0) (model.py:23-27); the table is the
            # last differentiable input of the autograd node (dense [V,E] gradient, row 0 stays zero)
            params = params + [self.embedding.weight]
        needs_grad = torch.is_grad_enabled() and any(p.requires_grad for p in params)
        if needs_grad:
            return _EncoderFn.apply(self, x, *params)
        out, _, _ = self._run_forward(x, train=False)
        return out


class TwoTowerModel(nn.Module):
    """Two independent RNNEncoder towers (no weight sharing; each owns its embedding table copy)."""

    def __init__(self, config: Dict, pretrained_embeddings: Optional[np.ndarray] = None):
        super().__init__()
        encoder_args = {
            "vocab_size": config["VOCAB_SIZE"],
            "embed_dim": config["EMBED_DIM"],
            "hidden_dim": config["HIDDEN_DIM"],
            "pretrained_embeddings": pretrained_embeddings,
            "rnn_type": config.get("RNN_TYPE", "GRU"),
            "num_layers": config.get("NUM_LAYERS", 1),
            "dropout": config.get("DROPOUT", 0.0),
            "bidirectional": config.get("BIDIRECTIONAL", False),
            "normalize_output": config.get("NORMALIZE_OUTPUT", True),
            "arith": config.get("ARITH", "split16"),   # (not a reference key: "f32" = every product on the fp32-MFMA kernels)
        }
        self.query_encoder = RNNEncoder(**encoder_args)
        self.doc_encoder = RNNEncoder(**encoder_args)

    def encode_query(self, query: torch.Tensor) -> torch.Tensor:
        return self.query_encoder(query)

    def encode_document(self, document: torch.Tensor) -> torch.Tensor:
        return self.doc_encoder(document)

    def forward(self, query: torch.Tensor, document: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        return self.encode_query(query), self.encode_document(document)


class _TripletFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, p, n, margin: float):
        L = _lib.lib()
        q, p, n = q.contiguous(), p.contiguous(), n.contiguous()
        B, H = q.shape
        loss = torch.empty((), dtype=torch.float32, device=q.device)
        dq, dp, dn = torch.empty_like(q), torch.empty_like(p), torch.empty_like(n)
        rows = torch.empty(B, dtype=torch.float32, device=q.device)
        with torch.cuda.device(q.device):
            _lib.check(L.tt_triplet_loss_f32(q.data_ptr(), p.data_ptr(), n.data_ptr(), B, H, float(margin),
                                             loss.data_ptr(), dq.data_ptr(), dp.data_ptr(), dn.data_ptr(),
                                             rows.data_ptr(), _stream(q.device)))
        ctx.save_for_backward(dq, dp, dn)
        return loss

    @staticmethod
    def backward(ctx, g):
        dq, dp, dn = ctx.saved_tensors
        return g * dq, g * dp, g * dn, None


def triplet_loss_cosine(triplet: Tuple[torch.Tensor, torch.Tensor, torch.Tensor], margin: float = 0.2) -> torch.Tensor:
    """mean(clamp(cos(q,n) - cos(q,p) + margin, min=0)), differentiable (fused forward+gradient kernel)."""
    query, pos_doc, neg_doc = triplet
    for t in (query, pos_doc, neg_doc):
        if not t.is_cuda:
            raise RuntimeError("triplet_loss_cosine runs only on an AMD GPU via libtt.so (no CPU fallback)")
        if t.dtype != torch.float32 or t.dim() != 2 or t.shape != query.shape:
            raise ValueError("triplet_loss_cosine wants three float32 [B,H] tensors of one shape")
    return _TripletFn.apply(query, pos_doc, neg_doc, margin)


def in_batch_workspace(B: int, H: int, device) -> torch.Tensor:
    """An uninitialised workspace for tt_in_batch_loss_f32 at [B,H] (the call rewrites all of it that it reads)."""
    need = _lib.lib().tt_in_batch_loss_workspace_bytes(B, H)
    if need == 0:
        raise ValueError(f"in_batch_softmax_loss: B={B} H={H} (B >= 1, 1 <= H <= 512)")
    return torch.empty(need, dtype=torch.uint8, device=device)


class _InBatchFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, p, n, temperature: float):
        L = _lib.lib()
        q, p, n = q.contiguous(), p.contiguous(), n.contiguous()
        B, H = q.shape
        loss = torch.empty((), dtype=torch.float32, device=q.device)
        dq, dp, dn = torch.empty_like(q), torch.empty_like(p), torch.empty_like(n)
        ws = in_batch_workspace(B, H, q.device)
        with torch.cuda.device(q.device):
            _lib.check(L.tt_in_batch_loss_f32(q.data_ptr(), p.data_ptr(), n.data_ptr(), B, H, float(temperature),
                                              loss.data_ptr(), dq.data_ptr(), dp.data_ptr(), dn.data_ptr(),
                                              ws.data_ptr(), ws.numel(), _stream(q.device)))
        ctx.save_for_backward(dq, dp, dn)
        return loss

    @staticmethod
    def backward(ctx, g):
        dq, dp, dn = ctx.saved_tensors
        return g * dq, g * dp, g * dn, None


def in_batch_softmax_loss(triplet: Tuple[torch.Tensor, torch.Tensor, torch.Tensor], temperature: float = 0.05,
                          groups: Optional[torch.Tensor] = None, neg_groups: Optional[torch.Tensor] = None,
                          symmetric: float = 0.0) -> torch.Tensor:
    """In-batch negatives: mean_i(logsumexp_j s_ij - s_ii), s_ij = cos(q_i, D_j) / temperature over D = [p; n] -- every query
    is scored against all 2B passages of the batch (its own positive, the other queries' positives, all explicit negatives)
    instead of one hinge against one negative.  Cosine with eps 1e-8 per norm, as triplet_loss_cosine.  Differentiable (fused
    forward + gradient kernels on the f32 matrix pipe, deterministic).
    The pool is the triplet's own 2B passages; contrastive_softmax_loss takes any pool (the trainers gather the passages of all
    ranks into one with gather_negatives=True).
    groups [B] (int64 on the device): grouped negatives -- query i and its positive carry groups[i], the negatives carry
    neg_groups [B] (None: -1, no group); a passage with query i's label >= 0, other than its own positive, is left out of its
    softmax (contrastive_softmax_loss).  Rows of one query that the batch holds several times share a label.
    symmetric in (0, 1]: the weight of the document-to-query direction (contrastive_softmax_loss, on the pool [p; n]: each
    positive is classified among the B queries; the explicit negatives have no query of their own).
    temperature: a float, or a LogitScale (the pool form on [p; n] at the module's word: contrastive_softmax_loss)."""
    query, pos_doc, neg_doc = triplet
    symmetric = _symmetric_weight("in_batch_softmax_loss", symmetric)
    if groups is None and neg_groups is not None:
        raise ValueError("in_batch_softmax_loss: neg_groups needs groups")
    for t in (query, pos_doc, neg_doc):
        if not t.is_cuda:
            raise RuntimeError("in_batch_softmax_loss runs only on an AMD GPU via libtt.so (no CPU fallback)")
        if t.dtype != torch.float32 or t.dim() != 2 or t.shape != query.shape:
            raise ValueError("in_batch_softmax_loss wants three float32 [B,H] tensors of one shape")
    if groups is None and (symmetric > 0.0 or isinstance(temperature, LogitScale)):
        return contrastive_softmax_loss(query, torch.cat((pos_doc, neg_doc)), 0, temperature, symmetric=symmetric)
    if groups is None:
        return _InBatchFn.apply(query, pos_doc, neg_doc, temperature)
    B = query.shape[0]
    groups = _group_labels("in_batch_softmax_loss", "groups", groups, B, query.device)
    if neg_groups is None:
        neg_groups = torch.full_like(groups, -1)
    else:
        neg_groups = _group_labels("in_batch_softmax_loss", "neg_groups", neg_groups, B, query.device)
    # (the pool entry on [p; n]: the in-batch entry's bits)
    return contrastive_softmax_loss(query, torch.cat((pos_doc, neg_doc)), 0, temperature, groups, torch.cat((groups, neg_groups)),
                                    symmetric=symmetric)


def contrastive_workspace(B: int, M: int, H: int, device) -> torch.Tensor:
    """An uninitialised workspace for tt_contrastive_loss_f32 at q [B,H], docs [M,H] (the call rewrites all of it that it reads)."""
    need = _lib.lib().tt_contrastive_loss_workspace_bytes(B, M, H)
    if need == 0:
        raise ValueError(f"contrastive_softmax_loss: B={B} M={M} H={H} (1 <= B <= M <= 2^25, B <= 2^24, 1 <= H <= 512)")
    return torch.empty(need, dtype=torch.uint8, device=device)


class _ContrastiveFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, docs, pos_offset: int, temperature: float, q_groups=None, doc_groups=None):
        L = _lib.lib()
        q, docs = q.contiguous(), docs.contiguous()
        (B, H), M = q.shape, docs.shape[0]
        loss = torch.empty((), dtype=torch.float32, device=q.device)
        dq, ddocs = torch.empty_like(q), torch.empty_like(docs)
        ws = contrastive_workspace(B, M, H, q.device)
        with torch.cuda.device(q.device):
            if q_groups is None:
                _lib.check(L.tt_contrastive_loss_f32(q.data_ptr(), B, docs.data_ptr(), M, H, int(pos_offset), float(temperature),
                                                     loss.data_ptr(), dq.data_ptr(), ddocs.data_ptr(), ws.data_ptr(), ws.numel(),
                                                     _stream(q.device)))
            else:
                q_groups, doc_groups = q_groups.contiguous(), doc_groups.contiguous()
                _lib.check(L.tt_contrastive_loss_grouped_f32(q.data_ptr(), B, docs.data_ptr(), M, H, int(pos_offset),
                                                             q_groups.data_ptr(), doc_groups.data_ptr(), float(temperature),
                                                             loss.data_ptr(), dq.data_ptr(), ddocs.data_ptr(), ws.data_ptr(),
                                                             ws.numel(), _stream(q.device)))
        ctx.save_for_backward(dq, ddocs)
        return loss

    @staticmethod
    def backward(ctx, g):
        dq, ddocs = ctx.saved_tensors
        return g * dq, g * ddocs, None, None, None, None


def symmetric_workspace(B: int, M: int, H: int, device) -> torch.Tensor:
    """An uninitialised workspace for tt_contrastive_loss_sym_f32 at q [B,H], docs [M,H] (the call rewrites all of it that it reads)."""
    need = _lib.lib().tt_contrastive_loss_sym_workspace_bytes(B, M, H)
    if need == 0:
        raise ValueError(f"contrastive_softmax_loss: B={B} M={M} H={H} (1 <= B <= M <= 2^25, B <= 2^24, 1 <= H <= 512)")
    return torch.empty(need, dtype=torch.uint8, device=device)


def _symmetric_call(q, docs, pos_offset, temperature, alpha, q_groups, doc_groups, loss, dirs, dq, ddocs):
    """tt_contrastive_loss_sym_f32 on contiguous tensors; dirs [2] and the gradients may be None."""
    L = _lib.lib()
    (B, H), M = q.shape, docs.shape[0]
    ws = symmetric_workspace(B, M, H, q.device)
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    with torch.cuda.device(q.device):
        _lib.check(L.tt_contrastive_loss_sym_f32(q.data_ptr(), B, docs.data_ptr(), M, H, int(pos_offset), ptr(q_groups),
                                                 ptr(doc_groups), float(temperature), float(alpha), loss.data_ptr(), ptr(dirs),
                                                 ptr(dq), ptr(ddocs), ws.data_ptr(), ws.numel(), _stream(q.device)))


class _SymmetricFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, docs, pos_offset: int, temperature: float, alpha: float, q_groups=None, doc_groups=None):
        q, docs = q.contiguous(), docs.contiguous()
        if q_groups is not None:
            q_groups, doc_groups = q_groups.contiguous(), doc_groups.contiguous()
        loss = torch.empty((), dtype=torch.float32, device=q.device)
        dq, ddocs = torch.empty_like(q), torch.empty_like(docs)
        _symmetric_call(q, docs, pos_offset, temperature, alpha, q_groups, doc_groups, loss, None, dq, ddocs)
        ctx.save_for_backward(dq, ddocs)
        return loss

    @staticmethod
    def backward(ctx, g):
        dq, ddocs = ctx.saved_tensors
        return g * dq, g * ddocs, None, None, None, None, None


class LogitScale(nn.Module):
    """A temperature that lives on the device: log_scale [1] f32 = log(1 / temperature) (CLIP's logit_scale), clamped into
    [log(1 / max_temperature), log(1 / min_temperature)] inside the loss kernels.  Pass it as `temperature=` to
    in_batch_softmax_loss, contrastive_softmax_loss, soft_contrastive_loss, symmetric_contrastive_losses and the trainers.
    learnable=True: a trained parameter -- the kernels return d loss / d log_scale beside dq and ddocs (torch.clamp's
    derivative: 0 outside the clamp); give `parameters()` to the optimizer along with the model's.
    learnable=False: a fixed word that a schedule may rewrite (`log_scale.fill_(...)` under torch.no_grad()).
    Either way the kernels read the word when they run, so a captured step (GraphedTrainStep) sees the current value at every
    replay with no recapture."""

    def __init__(self, temperature: float = 0.05, min_temperature: float = 0.01, max_temperature: float = 1.0,
                 learnable: bool = True):
        super().__init__()
        t, lo, hi = float(temperature), float(min_temperature), float(max_temperature)
        if not 0.0 < lo <= t <= hi < float("inf"):  # (NaN fails a comparison)
            raise ValueError(f"LogitScale: want 0 < min_temperature <= temperature <= max_temperature < inf, got "
                             f"{min_temperature!r}, {temperature!r}, {max_temperature!r}")
        self.min_log_scale, self.max_log_scale = -math.log(hi), -math.log(lo)
        if self.min_log_scale < -80.0 or self.max_log_scale > 80.0:
            raise ValueError("LogitScale: temperatures outside [exp(-80), exp(80)]")
        self.log_scale = nn.Parameter(torch.tensor([-math.log(t)], dtype=torch.float32), requires_grad=bool(learnable))

    @property
    def temperature(self) -> float:
        """The temperature the kernels would form now (reads the device word: a host sync, for logging)."""
        return math.exp(-min(max(float(self.log_scale.detach()[0]), self.min_log_scale), self.max_log_scale))

    def extra_repr(self) -> str:
        return (f"min_temperature={math.exp(-self.max_log_scale):g}, max_temperature={math.exp(-self.min_log_scale):g}, "
                f"learnable={self.log_scale.requires_grad}")


def _temperature_arg(who: str, temperature, device=None):
    """`temperature` as a float, or the LogitScale itself (its word on `device`), or the ValueError, before any launch."""
    if isinstance(temperature, LogitScale):
        w = temperature.log_scale
        if device is not None and (w.device != device or w.dtype != torch.float32 or tuple(w.shape) != (1,)):
            raise ValueError(f"{who}: the LogitScale's log_scale must be a float32 [1] on {device}, got {w.dtype} "
                             f"{tuple(w.shape)} on {w.device}")
        return temperature
    if isinstance(temperature, nn.Module) or not 0.0 < float(temperature) < float("inf"):  # (NaN fails both comparisons)
        raise ValueError(f"{who}: temperature={temperature!r} must be finite and > 0, or a LogitScale")
    return float(temperature)


def scaled_workspace(B: int, M: int, H: int, device, soft: bool = False, symmetric: bool = False) -> torch.Tensor:
    """An uninitialised workspace for tt_contrastive_loss_ls_f32 (soft: with targets) or tt_contrastive_loss_sym_ls_f32."""
    L = _lib.lib()
    need = L.tt_contrastive_loss_sym_ls_workspace_bytes(B, M, H) if symmetric else \
        L.tt_contrastive_loss_ls_workspace_bytes(B, M, H, int(soft))
    if need == 0:
        raise ValueError(f"contrastive loss: B={B} M={M} H={H} (1 <= B <= M <= 2^25, B <= 2^24, 1 <= H <= 512)")
    return torch.empty(need, dtype=torch.uint8, device=device)


def _scaled_call(q, docs, pos_offset, scale: LogitScale, alpha, q_groups, doc_groups, targets, loss, dirs, d_log_scale, dq,
                 ddocs, stream=None, ws=None):
    """tt_contrastive_loss_ls_f32 (alpha None) or tt_contrastive_loss_sym_ls_f32 on contiguous tensors; the kernels read
    scale.log_scale where it lies.  dirs, d_log_scale and the gradients may be None."""
    L = _lib.lib()
    (B, H), M = q.shape, docs.shape[0]
    if ws is None:
        ws = scaled_workspace(B, M, H, q.device, soft=targets is not None, symmetric=alpha is not None)
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    word, lo, hi = scale.log_scale.data_ptr(), scale.min_log_scale, scale.max_log_scale
    with torch.cuda.device(q.device):
        st = _stream(q.device) if stream is None else stream
        if alpha is None:
            _lib.check(L.tt_contrastive_loss_ls_f32(q.data_ptr(), B, docs.data_ptr(), M, H, int(pos_offset), ptr(q_groups),
                                                    ptr(doc_groups), ptr(targets), word, lo, hi, loss.data_ptr(), None,
                                                    ptr(d_log_scale), ptr(dq), ptr(ddocs), ws.data_ptr(), ws.numel(), st))
        else:
            _lib.check(L.tt_contrastive_loss_sym_ls_f32(q.data_ptr(), B, docs.data_ptr(), M, H, int(pos_offset), ptr(q_groups),
                                                        ptr(doc_groups), word, lo, hi, float(alpha), loss.data_ptr(), ptr(dirs),
                                                        None, ptr(d_log_scale), ptr(dq), ptr(ddocs), ws.data_ptr(), ws.numel(),
                                                        st))


class _ScaledFn(torch.autograd.Function):
    """The four losses at a LogitScale: the gradient of log_scale beside dq and ddocs, all scaled by the incoming g."""

    @staticmethod
    def forward(ctx, q, docs, log_scale, scale: LogitScale, pos_offset: int, alpha, q_groups=None, doc_groups=None, targets=None):
        q, docs = q.contiguous(), docs.contiguous()
        q_groups, doc_groups, targets = (None if t is None else t.contiguous() for t in (q_groups, doc_groups, targets))
        loss = torch.empty((), dtype=torch.float32, device=q.device)
        dq, ddocs = torch.empty_like(q), torch.empty_like(docs)
        dl = torch.empty(1, dtype=torch.float32, device=q.device) if ctx.needs_input_grad[2] else None
        _scaled_call(q, docs, pos_offset, scale, alpha, q_groups, doc_groups, targets, loss, None, dl, dq, ddocs)
        ctx.save_for_backward(dq, ddocs, *(() if dl is None else (dl,)))
        return loss

    @staticmethod
    def backward(ctx, g):
        dq, ddocs, *dl = ctx.saved_tensors
        return g * dq, g * ddocs, (g * dl[0] if dl else None), None, None, None, None, None, None


def _symmetric_weight(who: str, symmetric) -> float:
    """`symmetric` as a float in [0, 1], or the ValueError (before any launch)."""
    if isinstance(symmetric, bool) or not isinstance(symmetric, (int, float)) or not 0.0 <= float(symmetric) <= 1.0:  # (NaN fails)
        raise ValueError(f"{who}: symmetric={symmetric!r} must be a number in [0, 1]")
    return float(symmetric)


def _group_labels(who: str, name: str, t, rows: int, device) -> torch.Tensor:
    """`t` as the labels of `rows` rows, or the ValueError that names the argument."""
    if not isinstance(t, torch.Tensor) or t.dtype != torch.int64 or tuple(t.shape) != (rows,) or t.device != device:
        got = f"{t.dtype} {tuple(t.shape)} on {t.device}" if isinstance(t, torch.Tensor) else type(t).__name__
        raise ValueError(f"{who}: {name} must be an int64 tensor [{rows}] on {device}, got {got}")
    return t


def _contrastive_args(who: str, q, docs, pos_offset, temperature, q_groups, doc_groups):
    """The checks of the pool losses, before any launch -> (B, M, q_groups, doc_groups, temperature as _temperature_arg gives it)."""
    if (q_groups is None) != (doc_groups is None):
        raise ValueError(f"{who}: q_groups and doc_groups must be both given or both None")
    for t in (q, docs):
        if not t.is_cuda:
            raise RuntimeError(f"{who} runs only on an AMD GPU via libtt.so (no CPU fallback)")
        if t.dtype != torch.float32 or t.dim() != 2:
            raise ValueError(f"{who} wants float32 q [B,H] and docs [M,H]")
    (B, H), M = q.shape, docs.shape[0]
    if docs.shape[1] != H:
        raise ValueError(f"{who}: q has H={H}, docs has H={docs.shape[1]}")
    if M < B:
        raise ValueError(f"{who}: M={M} documents for B={B} queries (every query needs its positive: M >= B)")
    if not 0 <= pos_offset <= M - B:
        raise ValueError(f"{who}: pos_offset={pos_offset!r} outside [0, M - B = {M - B}]")
    temperature = _temperature_arg(who, temperature, q.device)
    if q_groups is not None:
        q_groups = _group_labels(who, "q_groups", q_groups, B, q.device)
        doc_groups = _group_labels(who, "doc_groups", doc_groups, M, q.device)
    return B, M, q_groups, doc_groups, temperature


def contrastive_softmax_loss(q: torch.Tensor, docs: torch.Tensor, pos_offset: int = 0, temperature: float = 0.05,
                             q_groups: Optional[torch.Tensor] = None, doc_groups: Optional[torch.Tensor] = None,
                             symmetric: float = 0.0) -> torch.Tensor:
    """The softmax contrastive loss of B queries over a pool of M >= B documents:
    mean_i(logsumexp_j s_ij - s_{i, pos_offset+i}), s_ij = cos(q_i, docs_j) / temperature -- the positive of query i is row
    pos_offset + i of `docs`, every other row is a negative (the passages gathered from all ranks; or several explicit negatives
    per query).  in_batch_softmax_loss((q, p, n)) is contrastive_softmax_loss(q, cat(p, n)), bit for bit.  Cosine with eps 1e-8
    per norm.  Differentiable in q and docs (fused forward + gradient kernels on the f32 matrix pipe, deterministic).
    q_groups [B], doc_groups [M] (int64 on the device, both or neither): grouped negatives.  Row j is left out of query i's
    softmax -- logsumexp and both gradients -- when j != pos_offset + i, q_groups[i] >= 0 and doc_groups[j] == q_groups[i]:
    the other positives of a query that the batch holds several times are no negatives of it.  A negative label is "no group".
    With no match off the positives the result is the ungrouped call's, bit for bit.
    symmetric = alpha in (0, 1]: the SYMMETRIC loss (1 - alpha) L_qd + alpha L_dq -- L_qd the loss above, L_dq =
    mean_i(logsumexp_{i'<B} s_{i', pos_offset+i} - s_{i, pos_offset+i}) classifies each positive document among the B queries
    (the bidirectional InfoNCE; 0.5 is the CLIP loss).  Only the B positive rows of `docs` have a softmax of their own; every
    other row stays a negative of the query-to-document direction alone.  With labels an ignored pair leaves both softmaxes.
    0.0 is the one-directional loss above, on its own kernels; symmetric_contrastive_losses reports the two directions.
    Soft targets (soft_contrastive_loss) do not combine with it.
    temperature: a float (an argument of the launches), or a LogitScale: the kernels read its word on the device when they run,
    and the loss is also differentiable in log_scale (where the module is learnable)."""
    symmetric = _symmetric_weight("contrastive_softmax_loss", symmetric)
    B, M, q_groups, doc_groups, temperature = _contrastive_args("contrastive_softmax_loss", q, docs, pos_offset, temperature,
                                                                q_groups, doc_groups)
    if isinstance(temperature, LogitScale):
        return _ScaledFn.apply(q, docs, temperature.log_scale, temperature, int(pos_offset), symmetric if symmetric > 0.0 else None,
                               q_groups, doc_groups)
    if symmetric > 0.0:
        return _SymmetricFn.apply(q, docs, int(pos_offset), temperature, symmetric, q_groups, doc_groups)
    if q_groups is None:
        return _ContrastiveFn.apply(q, docs, int(pos_offset), temperature)
    return _ContrastiveFn.apply(q, docs, int(pos_offset), temperature, q_groups, doc_groups)


def symmetric_contrastive_losses(q: torch.Tensor, docs: torch.Tensor, pos_offset: int = 0, temperature: float = 0.05,
                                 q_groups: Optional[torch.Tensor] = None,
                                 doc_groups: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """(L_qd, L_dq): the two directions of the symmetric contrastive_softmax_loss as 0-d tensors, for logging (one loss-only
    call; not differentiable).  Whatever weight a step trains with, its loss is (1 - symmetric) L_qd + symmetric L_dq."""
    _, _, q_groups, doc_groups, temperature = _contrastive_args("symmetric_contrastive_losses", q, docs, pos_offset, temperature,
                                                                q_groups, doc_groups)
    q, docs = q.detach().contiguous(), docs.detach().contiguous()
    if q_groups is not None:
        q_groups, doc_groups = q_groups.contiguous(), doc_groups.contiguous()
    loss = torch.empty((), dtype=torch.float32, device=q.device)
    dirs = torch.empty(2, dtype=torch.float32, device=q.device)
    if isinstance(temperature, LogitScale):
        _scaled_call(q, docs, pos_offset, temperature, 0.0, q_groups, doc_groups, None, loss, dirs, None, None, None)
    else:
        _symmetric_call(q, docs, pos_offset, temperature, 0.0, q_groups, doc_groups, loss, dirs, None, None)
    return dirs[0], dirs[1]


def soft_contrastive_workspace(B: int, M: int, H: int, device) -> torch.Tensor:
    """An uninitialised workspace for tt_contrastive_loss_soft_f32 at q [B,H], docs [M,H] (the call rewrites all of it that it reads)."""
    need = _lib.lib().tt_contrastive_loss_soft_workspace_bytes(B, M, H)
    if need == 0:
        raise ValueError(f"soft_contrastive_loss: B={B} M={M} H={H} (1 <= B <= M <= 2^25, B <= 2^24, 1 <= H <= 512)")
    return torch.empty(need, dtype=torch.uint8, device=device)


class _SoftContrastiveFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, docs, targets, temperature: float):
        L = _lib.lib()
        q, docs, targets = q.contiguous(), docs.contiguous(), targets.contiguous()
        (B, H), M = q.shape, docs.shape[0]
        loss = torch.empty((), dtype=torch.float32, device=q.device)
        dq, ddocs = torch.empty_like(q), torch.empty_like(docs)
        ws = soft_contrastive_workspace(B, M, H, q.device)
        with torch.cuda.device(q.device):
            _lib.check(L.tt_contrastive_loss_soft_f32(q.data_ptr(), B, docs.data_ptr(), M, H, targets.data_ptr(), float(temperature),
                                                      loss.data_ptr(), dq.data_ptr(), ddocs.data_ptr(), ws.data_ptr(), ws.numel(),
                                                      _stream(q.device)))
        ctx.save_for_backward(dq, ddocs)
        return loss

    @staticmethod
    def backward(ctx, g):
        dq, ddocs = ctx.saved_tensors
        return g * dq, g * ddocs, None, None


def _soft_targets(who: str, t, B: int, M: int, device) -> torch.Tensor:
    """`t` as the targets of B queries over M documents, or the ValueError that names the argument."""
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or tuple(t.shape) != (B, M) or t.device != device:
        got = f"{t.dtype} {tuple(t.shape)} on {t.device}" if isinstance(t, torch.Tensor) else type(t).__name__
        raise ValueError(f"{who}: targets must be a float32 tensor [{B}, {M}] on {device}, got {got}")
    return t


def soft_contrastive_loss(q: torch.Tensor, docs: torch.Tensor, targets: torch.Tensor, temperature: float = 0.05) -> torch.Tensor:
    """The softmax loss of B queries over a pool of M >= B documents against SOFT TARGETS t [B,M] (float32 on q's device):
    mean_i(w_i logsumexp_j s_ij - sum_j t_ij s_ij), w_i = sum_j t_ij, s_ij = cos(q_i, docs_j) / temperature -- the cross-entropy
    of each query's softmax over the pool against its target row.  distillation_targets makes the rows from a teacher's scores,
    multi_positive_targets from group labels.  Rows need not sum to 1 and weights may be negative (any finite float32).
    For a probability row t_i the row loss is KL(t_i || p_i) + H(t_i): the entropy H(t_i) has no gradient and is not subtracted
    here; subtract it where KL itself is reported.
    One-hot targets (1 at pos_offset + i) give contrastive_softmax_loss(q, docs, pos_offset), bit for bit; an all-zero row
    gives that query no loss and no gradient.  Differentiable in q and docs, not in targets (fused forward + gradient kernels
    on the f32 matrix pipe, deterministic; [B,M] logits never reach memory).
    The symmetric loss (contrastive_softmax_loss(symmetric=)) does not combine with soft targets: they define their own rows
    and there are no column targets.  temperature: a float or a LogitScale (contrastive_softmax_loss)."""
    for t in (q, docs):
        if not t.is_cuda:
            raise RuntimeError("soft_contrastive_loss runs only on an AMD GPU via libtt.so (no CPU fallback)")
        if t.dtype != torch.float32 or t.dim() != 2:
            raise ValueError("soft_contrastive_loss wants float32 q [B,H] and docs [M,H]")
    (B, H), M = q.shape, docs.shape[0]
    if docs.shape[1] != H:
        raise ValueError(f"soft_contrastive_loss: q has H={H}, docs has H={docs.shape[1]}")
    if M < B:
        raise ValueError(f"soft_contrastive_loss: M={M} documents for B={B} queries (the pool entries want M >= B)")
    temperature = _temperature_arg("soft_contrastive_loss", temperature, q.device)
    targets = _soft_targets("soft_contrastive_loss", targets, B, M, q.device)
    if isinstance(temperature, LogitScale):
        return _ScaledFn.apply(q, docs, temperature.log_scale, temperature, 0, None, None, None, targets.detach())
    return _SoftContrastiveFn.apply(q, docs, targets.detach(), temperature)


def distillation_targets(teacher_scores: torch.Tensor, teacher_temperature: float = 1.0,
                         valid: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Targets for soft_contrastive_loss from a teacher's scores [B,M] (cross-encoder, BM25 / TF-IDF, an earlier checkpoint):
    softmax(teacher_scores / teacher_temperature) over the pairs where `valid` (bool [B,M], default all) holds, 0 elsewhere; a
    row with no valid pair is all zeros (that query then has no loss and no gradient).  float32 [B,M] on the scores' device;
    stock torch ops, any device."""
    if not isinstance(teacher_scores, torch.Tensor) or teacher_scores.dim() != 2 or not teacher_scores.is_floating_point():
        got = f"{teacher_scores.dtype} {tuple(teacher_scores.shape)}" if isinstance(teacher_scores, torch.Tensor) else type(teacher_scores).__name__
        raise ValueError(f"distillation_targets: teacher_scores must be a floating-point tensor [B,M], got {got}")
    if not 0.0 < float(teacher_temperature) < float("inf"):
        raise ValueError(f"distillation_targets: teacher_temperature={teacher_temperature!r} must be finite and > 0")
    z = teacher_scores.detach().to(torch.float32) / float(teacher_temperature)
    if valid is None:
        return torch.softmax(z, dim=1)
    if (not isinstance(valid, torch.Tensor) or valid.dtype != torch.bool or valid.shape != teacher_scores.shape
            or valid.device != teacher_scores.device):
        got = f"{valid.dtype} {tuple(valid.shape)} on {valid.device}" if isinstance(valid, torch.Tensor) else type(valid).__name__
        raise ValueError(f"distillation_targets: valid must be a bool tensor {tuple(teacher_scores.shape)} on "
                         f"{teacher_scores.device}, got {got}")
    some = valid.any(dim=1, keepdim=True)
    # (a row without a valid pair: softmax of all -inf would be NaN; it is scored as it lies and zeroed)
    t = torch.softmax(z.masked_fill(~valid & some, float("-inf")), dim=1)
    return torch.where(valid, t, torch.zeros_like(t))


def multi_positive_targets(q_groups: torch.Tensor, doc_groups: torch.Tensor, pos_offset: int = 0) -> torch.Tensor:
    """Targets for soft_contrastive_loss that pull a query towards ALL its positives in the pool (the SupCon / multi-label form):
    1/|P_i| on each j in P_i = {j : q_groups[i] >= 0 and doc_groups[j] == q_groups[i]} + {pos_offset + i}, 0 elsewhere.  Labels
    as contrastive_softmax_loss takes them: int64 q_groups [B], doc_groups [M] on one device, a negative label is "no group".
    P_i is the own positive plus exactly the rows that grouped negatives would leave out.  float32 [B,M]; stock torch ops."""
    if not isinstance(q_groups, torch.Tensor) or q_groups.dim() != 1:
        raise ValueError(f"multi_positive_targets: q_groups must be an int64 tensor [B], got {type(q_groups).__name__}")
    B = q_groups.shape[0]
    q_groups = _group_labels("multi_positive_targets", "q_groups", q_groups, B, q_groups.device)
    if not isinstance(doc_groups, torch.Tensor) or doc_groups.dim() != 1:
        raise ValueError(f"multi_positive_targets: doc_groups must be an int64 tensor [M], got {type(doc_groups).__name__}")
    M = doc_groups.shape[0]
    doc_groups = _group_labels("multi_positive_targets", "doc_groups", doc_groups, M, q_groups.device)
    if M < B or not 0 <= pos_offset <= M - B:
        raise ValueError(f"multi_positive_targets: pos_offset={pos_offset!r} outside [0, M - B = {M - B}]")
    member = (q_groups[:, None] >= 0) & (doc_groups[None, :] == q_groups[:, None])
    i = torch.arange(B, device=q_groups.device)
    member[i, pos_offset + i] = True
    return member.to(torch.float32) / member.sum(dim=1, keepdim=True).to(torch.float32)
