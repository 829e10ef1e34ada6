"""Triplet-loss training step, data-parallel over RCCL.

Mirrors the live train step of the reference (backend/main.py:244-259):

    optimizer.zero_grad()
    q, p, n = model.encode_query(queries), model.encode_document(pos), model.encode_document(neg)
    loss = triplet_loss_cosine((q, p, n), margin)          # model.py:109-114
    loss.backward()
    torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm=1.0)
    optimizer.step()                                       # Adam(lr), main.py:222

`FusedClipAdam` replaces the last two lines with ONE kernel pair over a single flat fp32 buffer
(tt_clip_adam_step_f32) and, when a process group is given, ONE summing all-reduce of that buffer
(RCCL over xGMI for the nccl backend) followed by the 1/world scale inside the kernel -- so every rank
clips the SAME averaged gradient, exactly as the reference would on the global batch.
The reference's own pair of torch calls also keeps working on this package's model (its gradients
are ordinary tensors); the fused optimizer is the MI355X-native path.
"""
from __future__ import annotations

import ctypes as C
from typing import Callable, Iterable, NamedTuple, Optional, Tuple

import torch

from . import _lib
from .collective import Collective
from .model import (LogitScale, RNNEncoder, SplitRecurrenceTimeout, TwoTowerModel, _group_labels, _raise_status, _scaled_call,
                    _soft_targets, contrastive_softmax_loss, contrastive_workspace, deferred_input_checks,
                    in_batch_softmax_loss, in_batch_workspace, scaled_workspace, soft_contrastive_loss, soft_contrastive_workspace,
                    symmetric_workspace, triplet_loss_cosine)

__all__ = ["FusedClipAdam", "train_step", "DataParallelTrainer", "GraphedTrainStep"]


def _hip_clip_adam(flat_p, flat_g, m, v, step, lr, betas, eps, max_norm, grad_scale, total_norm, scratch):
    L = _lib.lib()
    with torch.cuda.device(flat_p.device):
        _lib.check(L.tt_clip_adam_step_f32(flat_p.data_ptr(), flat_g.data_ptr(), m.data_ptr(), v.data_ptr(),
                                           flat_p.numel(), step, lr, betas[0], betas[1], eps, max_norm, grad_scale,
                                           total_norm.data_ptr(), scratch.data_ptr(),
                                           torch.cuda.current_stream(flat_p.device).cuda_stream))


def _hip_clip_adam_gated(flat_p, flat_g, m, v, step_dev, lr, betas, eps, max_norm, grad_scale, total_norm, gate, scratch):
    L = _lib.lib()
    with torch.cuda.device(flat_p.device):
        _lib.check(L.tt_clip_adam_step_gated_f32(flat_p.data_ptr(), flat_g.data_ptr(), m.data_ptr(), v.data_ptr(),
                                                 flat_p.numel(), step_dev.data_ptr(), lr, betas[0], betas[1], eps, max_norm,
                                                 grad_scale, total_norm.data_ptr(),
                                                 gate.data_ptr() if gate is not None else None, scratch.data_ptr(),
                                                 torch.cuda.current_stream(flat_p.device).cuda_stream))


def _hip_step_gate(status_words, gate):
    """gate[b] = how many of the status words have bit b set (one launch, no host read)."""
    cur = torch.cuda.current_stream(gate.device)
    arr = (C.c_void_p * len(status_words))()
    for i, st in enumerate(status_words):
        st.record_stream(cur)  # (written on a tower's stream, read here)
        arr[i] = st.data_ptr()
    with torch.cuda.device(gate.device):
        _lib.check(_lib.lib().tt_step_gate_f32(arr, len(status_words), gate.data_ptr(), cur.cuda_stream))


def _torch_step_gate(status_words, gate):
    """The same on ordinary tensors (the CPU rehearsals of the host logic)."""
    bits = torch.stack([st.reshape(()).to(torch.int64) for st in status_words])
    for b in range(3):
        gate[b] = float(((bits >> b) & 1).sum())
    gate[3] = 0.0


class _FlatClipAdam:
    """Host logic of the fused optimizer on ordinary tensors: all trainable parameters are re-pointed at views of one
    contiguous fp32 buffer (`flat_params`) and their .grad at views of `flat_grads`, so the optimizer and the
    data-parallel all-reduce touch two pointers; step() = summing all-reduce -> step_fn(..., grad_scale = 1/world).

    A FAILED STEP IS A COLLECTIVE DECISION.  The gradient bucket has TT_STEP_GATE_WORDS extra floats behind the gradients (the
    `gate`): before the all-reduce they hold, per status bit, how many of this rank's encoder calls raised it (zero-length row,
    id out of range, column-split recurrence timed out: the status words the watched encoders handed over -- `watch`); the ONE
    all-reduce sums them with the gradients, so afterwards every rank holds the same counts, the device applies the step on
    all ranks or on none, and every rank raises the same exception.  The reference's step is single-process (a bad batch
    raises and the run stops, backend/main.py:244-259); a rank-local raise in front of the all-reduce would leave the peers
    waiting in it forever.

    Private: the CPU tests drive it over gloo with the oracle's step; the product class is FusedClipAdam."""

    GATE = _lib.TT_STEP_GATE_WORDS

    def __init__(self, params: Iterable[torch.nn.Parameter], step_fn: Callable, all_reduce: Callable, world: int,
                 lr: float, betas: Tuple[float, float], eps: float, max_norm: float, scratch_bytes: int,
                 gate_fn: Callable = _torch_step_gate, gated_step_fn: Optional[Callable] = None):
        self.params = [p for p in params if p.requires_grad]
        if not self.params:
            raise ValueError("no trainable parameters")
        dev = self.params[0].device
        self.lr, self.betas, self.eps, self.max_norm = float(lr), (float(betas[0]), float(betas[1])), float(eps), float(max_norm)
        self._step_fn, self._all_reduce, self.world = step_fn, all_reduce, int(world)
        self._gate_fn, self._gated_step_fn = gate_fn, gated_step_fn
        n = sum(p.numel() for p in self.params)
        self.flat_params = torch.empty(n, dtype=torch.float32, device=dev)
        self._bucket = torch.zeros(n + self.GATE, dtype=torch.float32, device=dev)  # what the all-reduce sees
        self.flat_grads = self._bucket[:n]
        self.gate = self._bucket[n:]
        self.exp_avg = torch.zeros(n, dtype=torch.float32, device=dev)
        self.exp_avg_sq = torch.zeros(n, dtype=torch.float32, device=dev)
        self.total_norm = torch.zeros(1, dtype=torch.float32, device=dev)
        self._scratch = torch.empty(scratch_bytes, dtype=torch.uint8, device=dev)
        self._step_dev = torch.zeros(1, dtype=torch.int64, device=dev)  # steps applied (the gated kernel counts on the device)
        self._step_host = 0
        self._pending_status: list = []  # status words of the watched encoders' training calls since the last step()
        self._gate_host, self._gate_ev, self._gate_n, self._deferred = None, None, 0, None   # (snapshot_gate / settle)
        self._reduced_upto = 0           # gradients [0, _reduced_upto) of this step have been all-reduced already (reduce_prefix)
        self.reduce_timing: Optional[list] = None   # a list: every all-reduce appends (event before, event after, bytes) -- bench.py
        self.check = True                # step() reads the reduced gate (one host synchronisation) and raises
        self._views = []
        off = 0
        with torch.no_grad():
            for p in self.params:
                k = p.numel()
                self.flat_params[off:off + k].copy_(p.detach().reshape(-1))
                p.data = self.flat_params[off:off + k].view_as(p)
                gv = self.flat_grads[off:off + k].view_as(p)
                p.grad = gv
                self._views.append(gv)
                off += k

    # ---- step number -----------------------------------------------------------
    @property
    def step_count(self) -> int:
        """Steps applied so far (reads the device counter of the gated kernel: a host synchronisation)."""
        return int(self._step_dev.item()) if self._gated_step_fn is not None else self._step_host

    @step_count.setter
    def step_count(self, value: int) -> None:
        self._step_host = int(value)
        self._step_dev.fill_(int(value))

    # ---- status words of the encoders -------------------------------------------
    def watch(self, *modules) -> None:
        """The RNNEncoders inside `modules` hand the status words of their TRAINING calls to this optimizer instead of raising
        at the call: step() reduces them over the ranks with the gradients and raises -- on every rank -- what the reference
        would have raised.  DataParallelTrainer and train_step do this for their model; a hand-written loop around
        FusedClipAdam(group=...) must, or a bad batch on one rank leaves the others waiting in the all-reduce.
        What a watched encoder hands over is EVERY grad-enabled forward since the last step(): all of them (any number:
        gradient accumulation) decide the next step() together.  Forwards that belong to no step -- validation -- must run under
        torch.no_grad() (as the reference's evaluators do, backend/evaluators.py:31), or their bad batch vetoes the next training
        step instead of raising where it happened; unwatch() ends the hand-over."""
        for mod in modules:
            for enc in mod.modules():
                if isinstance(enc, RNNEncoder):
                    enc._status_sink = self._pending_status

    def unwatch(self, *modules) -> None:
        for mod in modules:
            for enc in mod.modules():
                if isinstance(enc, RNNEncoder) and enc._status_sink is self._pending_status:
                    enc._status_sink = None

    def zero_grad(self) -> None:
        self.flat_grads.zero_()
        for p, gv in zip(self.params, self._views):
            p.grad = gv

    def _collect(self) -> None:
        """Tolerate callers that reset .grad to None / fresh tensors (model.zero_grad(set_to_none=True))."""
        for p, gv in zip(self.params, self._views):
            if p.grad is None:
                gv.zero_()
            elif p.grad.data_ptr() != gv.data_ptr():
                gv.copy_(p.grad)
            p.grad = gv

    def step(self, check: Optional[bool] = None) -> torch.Tensor:
        """Returns the pre-clip global gradient norm (device tensor).  With status words pending or a process group, the step
        is gated (class docstring) and -- unless check is False -- the reduced gate is read back (the step's one host
        synchronisation): IndexError / RuntimeError as the reference raises them, model.SplitRecurrenceTimeout for a time-out,
        on every rank alike; parameters, moments and step number are then untouched."""
        self._collect()
        return self._reduce_apply(self._fold_status(), check)

    def _fold_status(self) -> bool:
        """The pending status words -> the gate words behind the gradients (one launch, no host read).  Returns whether the step
        is gated (status words were pending, or there is a process group)."""
        status = list(self._pending_status)
        self._pending_status.clear()  # (in place: the watched encoders hold this list)
        gated = bool(status) or self.world > 1
        if status:
            self._gate_fn(status, self.gate)
        elif gated:
            self.gate.zero_()
        return gated

    def reduce_prefix(self, upto: int) -> None:
        """Data-parallel only: all-reduce the bucket's first `upto` gradients NOW, on the current stream -- the part of the
        bucket whose gradients are already complete (the query tower's, while the document tower's weight-gradient kernels still
        run: the exchange of half the bucket hides under them).  _reduce_apply then reduces the rest, gate words included: the
        failure decision still rides in the LAST all-reduce of the step.  Every rank must make the same calls in the same order
        (a function of the model's structure only)."""
        if self.world > 1 and 0 < upto <= self.flat_grads.numel() and self._reduced_upto == 0:
            self._timed_all_reduce(self._bucket[:upto])
            self._reduced_upto = int(upto)

    def _timed_all_reduce(self, part: torch.Tensor) -> None:
        """The all-reduce of one part of the bucket on the current stream; with `reduce_timing` set, bracketed by two timing
        events on that stream (what the collective costs THIS rank, its wait for the slowest peer included)."""
        if self.reduce_timing is None or not part.is_cuda:
            self._all_reduce(part)
            return
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        self._all_reduce(part)
        e1.record()
        self.reduce_timing.append((e0, e1, part.numel() * 4))

    def _reduce_apply(self, gated: bool, check: Optional[bool] = None) -> torch.Tensor:
        if self.world > 1:
            # the bucket: 3.4 MB of gradients + the gate words (minus what reduce_prefix has sent already)
            self._timed_all_reduce(self._bucket[self._reduced_upto:] if self._reduced_upto else self._bucket)
            self._reduced_upto = 0
        args = (self.lr, self.betas, self.eps, self.max_norm, 1.0 / self.world, self.total_norm)
        words = None
        if self._gated_step_fn is not None:
            self._gated_step_fn(self.flat_params, self.flat_grads, self.exp_avg, self.exp_avg_sq, self._step_dev, *args,
                                self.gate if gated else None, self._scratch)
        else:  # ordinary tensors: the gate is looked at on the host
            words = self.gate.tolist() if gated else None
            if not words or not any(words):
                self._step_host += 1
                self._step_fn(self.flat_params, self.flat_grads, self.exp_avg, self.exp_avg_sq, self._step_host, *args,
                              self._scratch)
        self.mark_params_changed()
        if gated and (self.check if check is None else check):
            self.raise_for_gate(self.gate.tolist() if words is None else words)
        return self.total_norm

    @staticmethod
    def raise_for_gate(words) -> None:
        _raise_status(sum(1 << b for b in range(3) if words[b] != 0))

    # ---- the gate read, one step late (train_step(defer_check=True), GraphedTrainStep(defer_check=True)) --------------------
    def snapshot_gate(self, redo: Optional[Callable] = None) -> None:
        """Copy the (reduced) gate words of the step just enqueued to pinned host memory, asynchronously on the current stream, and
        make them THE pending check of this optimizer; the previous pending check -- whose step has long finished -- is settled
        afterwards (it raises here, one call late).  redo: called instead of raising when the words say "recurrence time-out".
        Order matters: THIS step's copy is enqueued and registered first, so neither an exception out of the previous check nor
        its redo (which runs a whole step: new gate words in the same device buffer) can lose it -- the copy is already in the
        stream in front of anything the redo enqueues, and it stays pending for the next call's settle().  A redone step is
        applied BEHIND the step enqueued in this call (it was skipped on the device when its turn came; the weights it now starts
        from include this call's update): the order of two updates changes, none is lost."""
        if self._gate_host is None:
            self._gate_host = [torch.zeros(self.GATE, dtype=torch.float32).pin_memory() if self.gate.is_cuda
                               else torch.zeros(self.GATE, dtype=torch.float32) for _ in range(2)]
            self._gate_ev = [torch.cuda.Event() if self.gate.is_cuda else None for _ in range(2)]
        slot = self._gate_n & 1          # (the other slot holds the previous pending check, if there is one)
        self._gate_n += 1
        self._gate_host[slot].copy_(self.gate, non_blocking=True)
        if self._gate_ev[slot] is not None:
            self._gate_ev[slot].record(torch.cuda.current_stream(self.gate.device))
        previous, self._deferred = self._deferred, (slot, redo)
        self._settle_one(previous)

    def settle(self):
        """Look at the pending check, if any: raises what its step would have raised (IndexError / RuntimeError), or returns
        redo()'s result after a recurrence time-out, or None."""
        pending, self._deferred = self._deferred, None
        return self._settle_one(pending)

    def _settle_one(self, pending):
        if pending is None:
            return None
        slot, redo = pending
        if self._gate_ev[slot] is not None:
            self._gate_ev[slot].synchronize()
        try:
            self.raise_for_gate(self._gate_host[slot].tolist())
        except SplitRecurrenceTimeout:
            if redo is None:
                raise
            return redo()
        return None

    def mark_params_changed(self) -> None:
        """Call after ANY write to `flat_params` that did not go through the parameters themselves (this class's own step,
        a broadcast into the flat buffer, a checkpoint copied into it): the parameters are views whose version counters are
        separate from the flat buffer's, and RNNEncoder keys its cache of kernel-form weights on those counters -- without
        the bump an eval forward would keep serving the weights of before the write."""
        torch.autograd.graph.increment_version(self.params)


class FusedClipAdam(_FlatClipAdam):
    """clip_grad_norm_(max_norm) + Adam(lr, betas, eps, weight_decay=0) over one flat buffer in ONE kernel pair
    (tt_clip_adam_step_gated_f32: step number and bias corrections on the device, the step predicated on the reduced gate);
    with a process group, ONE summing all-reduce of the bucket first (tt_allreduce_grads on torch.distributed's RCCL
    communicator; torch.distributed's own call for other backends)."""

    def __init__(self, params: Iterable[torch.nn.Parameter], lr: float = 1e-4, betas: Tuple[float, float] = (0.9, 0.999),
                 eps: float = 1e-8, max_norm: float = 1.0, group=None, comm=None):
        params = [p for p in params if p.requires_grad]
        if params and params[0].device.type != "cuda":
            raise RuntimeError("FusedClipAdam runs only on an AMD GPU via libtt.so (no CPU fallback)")
        self.group = group
        self._coll = Collective(group, params[0].device if params else None, comm=comm)
        super().__init__(params, _hip_clip_adam, self._coll.all_reduce_sum, self._coll.world, lr, betas, eps, max_norm,
                         _lib.lib().tt_clip_adam_scratch_bytes(), gate_fn=_hip_step_gate, gated_step_fn=_hip_clip_adam_gated)


class _StepSpecFields(NamedTuple):
    margin: float
    negatives: str
    temperature: float
    gather_negatives: bool
    concurrent_towers: bool
    direct: bool


class _StepSpec(_StepSpecFields):
    """What one train step is asked to do, apart from its batch (the arguments are train_step's: see there).  Built and checked
    once at the public entries -- train_step, DataParallelTrainer, GraphedTrainStep --; everything below them takes the record.
    The six tuple fields are what the record has always been (callers and tests compare and unpack it as that 6-tuple);
    `symmetric`, the weight of the document-to-query direction of the "in_batch" loss (0.0: the one-directional loss), is the
    seventh constructor argument and a read-only attribute beside them.  Two records are equal when fields and weight are.
    `temperature` is a float or a model.LogitScale: the module itself, compared and hashed by identity -- a record (and a graph
    cache) keys on "the temperature lives in this module", never on the value its word holds."""

    def __new__(cls, margin, negatives, temperature, gather_negatives, concurrent_towers, direct, symmetric=0.0):
        self = super().__new__(cls, margin, negatives, temperature, gather_negatives, concurrent_towers, direct)
        object.__setattr__(self, "symmetric", symmetric)
        return self

    def __setattr__(self, name, value):
        raise AttributeError(f"can't set attribute {name!r}: a step specification is frozen")

    def __eq__(self, other):
        return tuple.__eq__(self, other) and (not isinstance(other, _StepSpec) or self.symmetric == other.symmetric)

    def __ne__(self, other):
        return not self == other

    def __hash__(self):
        return hash((tuple(self), self.symmetric))

    def __repr__(self):
        return super().__repr__()[:-1] + f", symmetric={self.symmetric!r})"

    def _replace(self, **kw):
        symmetric = kw.pop("symmetric", self.symmetric)
        return type(self)(*_StepSpecFields._replace(self, **kw), symmetric)

    def checked(self, graphs: bool) -> "_StepSpec":
        """This record, or the ValueError of a combination no step can run: raised before anything is launched."""
        if self.negatives not in ("paired", "in_batch"):
            raise ValueError(f'negatives must be "paired" or "in_batch", got {self.negatives!r}')
        if self.gather_negatives and self.negatives != "in_batch":
            raise ValueError(f'gather_negatives=True needs negatives="in_batch", got negatives={self.negatives!r}')
        if self.gather_negatives and graphs:
            raise ValueError("gather_negatives=True is not available with graphs=True (the exchange of the passages sits between "
                             "the captured forward and backward)")
        if isinstance(self.temperature, LogitScale) and self.negatives != "in_batch":
            raise ValueError(f'temperature=LogitScale needs negatives="in_batch", got negatives={self.negatives!r} (the triplet '
                             "loss has no temperature)")
        sym = self.symmetric
        if isinstance(sym, bool) or not isinstance(sym, (int, float)) or not 0.0 <= float(sym) <= 1.0:  # (NaN fails)
            raise ValueError(f"symmetric={sym!r} must be a number in [0, 1]")
        if sym > 0 and self.negatives != "in_batch":
            raise ValueError(f'symmetric={sym!r} needs negatives="in_batch", got negatives={self.negatives!r}')
        if sym > 0 and self.gather_negatives:
            raise ValueError("symmetric > 0 is not available with gather_negatives=True: over a gathered pool the softmax of a "
                             "positive's column runs over the queries of ALL ranks, which needs a gather of the queries and a "
                             "reduction of their gradients (a second exchange in the step's collective order)")
        return self


def _batch_labels(who: str, spec: _StepSpec, batch, groups, neg_groups) -> Optional[torch.Tensor]:
    """The batch's group labels as one int64 tensor [2B] = [groups; neg_groups], the labels of the 2B passages [p; n] (its first
    B entries are the queries' too), or None without labels.  They are data of the batch and travel beside it, not in the spec.
    neg_groups None: the negatives carry -1 (no group).  Raises the ValueError of labels no step can use before anything is
    launched: they are for negatives="in_batch" alone."""
    if groups is None and neg_groups is None:
        return None
    if spec.negatives != "in_batch":
        raise ValueError(f'{who}: groups / neg_groups need negatives="in_batch", got negatives={spec.negatives!r}')
    if groups is None:
        raise ValueError(f"{who}: neg_groups needs groups")
    queries, pos_docs, neg_docs = batch
    B = queries.shape[0]
    if not pos_docs.shape[0] == neg_docs.shape[0] == B:
        raise ValueError(f"{who}: groups need as many negatives as positives as queries")
    groups = _group_labels(who, "groups", groups, B, queries.device)
    neg_groups = torch.full_like(groups, -1) if neg_groups is None else _group_labels(who, "neg_groups", neg_groups, B, queries.device)
    return torch.cat((groups, neg_groups))


def _batch_targets(who: str, spec: _StepSpec, optimizer, batch, targets, groups=None, neg_groups=None) -> Optional[torch.Tensor]:
    """The batch's soft targets: float32 [B, 2B] over the passages [p; n] -- gathered, [B, world * 2B] over the pool of all ranks,
    rank r's [p_r; n_r] at column r * 2B -- or None without targets.  Data of the batch like the labels: they travel beside it.
    Raises the ValueError of targets no step can use before anything is launched: they are for negatives="in_batch" alone and
    never come together with group labels."""
    if targets is None:
        return None
    if spec.symmetric > 0:
        raise ValueError(f"{who}: targets and symmetric > 0 exclude each other (soft targets define their own rows and there are "
                         "no column targets)")
    if groups is not None or neg_groups is not None:
        raise ValueError(f"{who}: targets and groups / neg_groups exclude each other (soft targets say what every pair weighs)")
    if spec.negatives != "in_batch":
        raise ValueError(f'{who}: targets need negatives="in_batch", got negatives={spec.negatives!r}')
    queries, pos_docs, neg_docs = batch
    B = queries.shape[0]
    if not pos_docs.shape[0] == neg_docs.shape[0] == B:
        raise ValueError(f"{who}: targets need as many negatives as positives as queries")
    world = getattr(getattr(optimizer, "_coll", None), "world", 1) if spec.gather_negatives else 1
    return _soft_targets(who, targets, B, world * 2 * B, queries.device)


def _scale_grad_view(who: str, spec: _StepSpec, optimizer) -> Optional[torch.Tensor]:
    """Where the step's loss writes d loss / d log_scale: the optimizer's gradient view [1] of a learnable LogitScale's word.
    None: the temperature is a float, or a module that is not learnable (a fixed word, no gradient).  A learnable module whose
    word the optimizer does not own raises ValueError before anything is launched: its gradient would go nowhere."""
    scale = spec.temperature
    if not isinstance(scale, LogitScale) or not scale.log_scale.requires_grad:
        return None
    for p, gv in zip(getattr(optimizer, "params", ()), getattr(optimizer, "_views", ())):
        if p is scale.log_scale:
            return gv
    if isinstance(optimizer, _FlatClipAdam) or not any(p is scale.log_scale for g in getattr(optimizer, "param_groups", ())
                                                       for p in g["params"]):
        raise ValueError(f"{who}: the optimizer does not own the LogitScale's log_scale; build it over "
                         "list(model.parameters()) + list(scale.parameters())")
    return None


_TOWER_STREAMS = {}


def _tower_streams(device):
    key = (device.type, device.index)
    if key not in _TOWER_STREAMS:
        # [0] document tower, [1] query tower, [2] a third tower call of the autograd path.  (A high-priority query stream was
        # tried: its split recurrence still only gets whole CUs when the document tower's input projection ends -- that kernel's
        # workgroups are resident for its whole duration -- 161 us against 148 without, profiles/r04_l_train_timeline.txt.)
        _TOWER_STREAMS[key] = [torch.cuda.Stream(device=device) for _ in range(3)]
    return _TOWER_STREAMS[key]


def _stage_ids(out: torch.Tensor, a: torch.Tensor, b: Optional[torch.Tensor]) -> None:
    """out [Ba + Bb, T] <- rows of a, then rows of b (None: no rows), zero-padded to out's width: ONE launch (tt_concat_ids_i64)
    on the current stream, into an existing buffer (GraphedTrainStep's static inputs)."""
    a = a.contiguous()
    b = b.contiguous() if b is not None else None
    with torch.cuda.device(out.device):
        _lib.check(_lib.lib().tt_concat_ids_i64(a.data_ptr(), a.shape[0], a.shape[1], b.data_ptr() if b is not None else None,
                                                b.shape[0] if b is not None else 0, b.shape[1] if b is not None else 0,
                                                out.data_ptr(), out.shape[1], torch.cuda.current_stream(out.device).cuda_stream))


def _concat_ids(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """[a; b] padded to the longer T with id 0, on the CURRENT stream: one launch (_stage_ids) instead of torch's zero fill + two
    slice copies -- the document tower's whole chain waits for it."""
    out = torch.empty((a.shape[0] + b.shape[0], max(a.shape[1], b.shape[1])), dtype=torch.int64, device=a.device)
    _stage_ids(out, a, b)
    return out


# ---- which tower runs which recurrence ---------------------------------------------------------------------------------------
class _TowerPlan(NamedTuple):
    one_workgroup: tuple        # towers that run the one-workgroup recurrences, forward and backward
    one_workgroup_bwd: tuple    # towers that run the one-workgroup recurrence in the backward alone
    ordered: bool               # the towers' forward recurrence launches are to be ordered by events inside the calls


def _plan_towers(need, rows, cus, stacked, mode) -> _TowerPlan:
    """Which towers leave the column-split recurrences so that what is in flight together fits the device: the smallest towers
    first (fewest rows among equals) until the sum of the others fits.  Arithmetic only: no device, no library call.
    need: {tower: workgroups its split recurrence occupies; 0: it runs the one-workgroup kernels already}; rows: {tower: rows of
    its call}; cus: the device's CU count; stacked: a tower has more than one layer.  mode:
      "ordered"    the direct step, whose calls carry events: the towers stay split in the FORWARD and their recurrences are
                   ordered; the towers picked take the one-workgroup BACKWARD.  Stacked layers: as "no_events" (the ordering
                   event is recorded behind a call's LAST recurrence launch, i.e. behind ALL the layers of the smaller tower -- the
                   document tower's first layer would wait for the whole query tower: 207 us of a 5.5 ms step at the reference's
                   default shape, profiles/r04_z_config1_train_timeline.txt; the smaller tower's few short sequences on one
                   workgroup cost it ~90 us off the critical path)
      "no_events"  calls that cannot carry events (the autograd path, a graph capture): the towers picked take the one-workgroup
                   recurrences in both directions
      "forced"     the redo after a recurrence time-out: every tower of `need`, both directions."""
    if mode == "forced":
        return _TowerPlan(tuple(need), (), False)
    left, picked = dict(need), []
    for t in sorted(left, key=lambda t: (left[t], rows.get(t, 0))):
        if sum(left.values()) <= cus:
            break
        if left[t]:
            picked.append(t)
            left[t] = 0
    if not picked:
        return _TowerPlan((), (), False)
    if mode == "ordered" and not stacked:
        return _TowerPlan((), tuple(picked), True)
    return _TowerPlan(tuple(picked), (), False)


class _towers_in_flight:
    """For the duration of one train step: (1) the model's encoders hand their status words to `optimizer` (watch), so that
    the step's failure is decided in optimizer.step(), by all ranks together; (2) the towers that are in flight at the same time
    never have more column-split workgroups in flight than the device has CUs.  A split launch needs every member of every
    team resident at once (one workgroup per CU), which ONE launch guarantees against the CU count and two launches on two
    streams do not (query tower 128 + document tower 256 on 256 CUs: round 3 rested on in-order dispatch).  Two ways out, both
    co-residency BY CONSTRUCTION (_plan_towers decides; this class gathers its inputs, sets the encoders' flags and puts them back):
      * ordered (the direct step), FORWARD: the towers' recurrence launches are ordered by an event inside the calls
        (tt_enc_sync_t): the query tower's recurrence first, the document tower's behind it, everything else of the two towers
        still overlaps (_forward_sequence).  BACKWARD: the smaller tower runs the one-workgroup recurrence (its workgroups wait
        for nobody).  Ordering the backwards too was measured and dropped: the query
        tower's split recurrence behind the document tower's lands under the document tower's weight-gradient kernels, whose
        one-per-CU workgroups keep it off the CUs until they end (graph replay 1.146 -> 1.207 ms), and in front of it it would
        add its ~100 us to the critical path;
      * one_workgroup (the autograd path, whose calls cannot carry events): the smaller towers run the one-workgroup
        recurrences (TT_ENC_ONE_WORKGROUP: same bits, no hand-off) until the sum fits.  Measured (profiles/
        r04_j_train_timeline.txt): the query tower then holds 32 CUs for 280 + 390 us and 32 of the document tower's split
        workgroups wait for them -- correct (nobody waits for a workgroup that cannot be scheduled), ~60 us per step slower.
    (csrc/gru16x4.hip, include/tt.h)"""

    def __init__(self, model: TwoTowerModel, optimizer, rows: dict, force_one_workgroup: bool = False):
        self.model, self.optimizer, self.rows, self.force = model, optimizer, rows, force_one_workgroup
        self.needs_order = False

    def __enter__(self):
        encs = [self.model.query_encoder, self.model.doc_encoder]
        self._saved = [(e, e.one_workgroup, e.one_workgroup_bwd, e._status_sink) for e in encs]
        if isinstance(self.optimizer, _FlatClipAdam):
            self.optimizer.watch(*encs)
        self._need, self._cus, self._stacked = {}, 0, any(e.num_layers > 1 for e in encs)
        if self.force:
            self._apply(_plan_towers(dict.fromkeys(encs, 0), {}, 0, self._stacked, "forced"))
        elif self.rows and encs[0].embedding.weight.is_cuda:
            self._cus = torch.cuda.get_device_properties(encs[0].embedding.weight.device).multi_processor_count
            self._need = {e: (0 if (e.one_workgroup and e.one_workgroup_bwd is not False) else e.split_workgroups(B))
                          for e, B in self.rows.items()}
            self._apply(_plan_towers(self._need, self.rows, self._cus, self._stacked, "ordered"))
        return self

    def _apply(self, plan: _TowerPlan) -> None:
        for e in plan.one_workgroup:
            e.one_workgroup, e.one_workgroup_bwd = True, None
        for e in plan.one_workgroup_bwd:
            e.one_workgroup_bwd = True
        self.needs_order = plan.ordered

    def use_one_workgroup(self) -> None:
        """The plan for calls that cannot carry events: the smaller towers on the one-workgroup recurrences until the sum fits."""
        if self.needs_order:
            self._apply(_plan_towers(self._need, self.rows, self._cus, self._stacked, "no_events"))

    def __exit__(self, exc_type, exc, tb):
        for e, one, one_bwd, sink in self._saved:
            e.one_workgroup, e.one_workgroup_bwd, e._status_sink = one, one_bwd, sink
        if exc_type is not None and isinstance(self.optimizer, _FlatClipAdam):
            self.optimizer._pending_status.clear()  # (a step that died before optimizer.step(): its words are nobody's)
            self.optimizer._reduced_upto = 0
        return False


# ---- the order of the towers' forward calls ------------------------------------------------------------------------------------
_DOC, _QRY = 0, 1   # the direct step's tuples are (document tower, query tower): the document tower carries the critical path


class _FwdIssue(NamedTuple):
    tower: int              # _DOC / _QRY
    phase: int              # 0 = the whole call; _lib.TT_ENC_PHASE_BEGIN / _FINISH = one half of it
    event: Optional[str]    # "record": behind this call's recurrence; "wait": in front of it; None: the call carries no event
    one_workgroup: bool     # this call on the one-workgroup recurrence, whatever the encoder's flags say


# How the two towers' FORWARD recurrences share the CUs when both column-split would not fit (tools/experiments/fwd_order_ab.py,
# two_phase_check.py).  The call that RECORDS the ordering event must be issued before the WAIT for it (include/tt.h):
#   "query_first"        default: the query tower's recurrence first, the document tower's waits for it; the document tower's call
#                        goes out in two halves around the query tower's -- BEGIN (prep, weight conversion, input projection:
#                        130 us of GPU work), the query tower (records behind its recurrence), FINISH (waits, then recurrence +
#                        head) -- so that the document tower's projection does not wait for the host to issue the query tower
#   "query_first_whole"  the same order of recurrences with whole calls: the query tower's call is issued first
#   "doc_first"          the document tower's first, the query tower's waits (it has slack at the END of the step, none here: the
#                        loss needs its output)
#   "query_one_wg"       no ordering: the query tower on the one-workgroup recurrence beside the document tower's split one
_FWD_ORDER = "query_first"
_FORWARD_SEQUENCES = {
    "query_first": [_FwdIssue(_DOC, _lib.TT_ENC_PHASE_BEGIN, None, False), _FwdIssue(_QRY, 0, "record", False),
                    _FwdIssue(_DOC, _lib.TT_ENC_PHASE_FINISH, "wait", False)],
    "query_first_whole": [_FwdIssue(_QRY, 0, "record", False), _FwdIssue(_DOC, 0, "wait", False)],
    "doc_first": [_FwdIssue(_DOC, 0, "record", False), _FwdIssue(_QRY, 0, "wait", False)],
    "query_one_wg": [_FwdIssue(_DOC, 0, None, False), _FwdIssue(_QRY, 0, None, True)],
}


def _forward_sequence(ordered: bool, order: str) -> list:
    """The tower calls of the direct step's forward in the order they are issued.  Not ordered (both towers' split recurrences fit
    the device, or the plan took one off them): the document tower (2B rows of ~70 tokens: the step's critical path) FIRST, the
    query tower's ~15 small launches then overlap it instead of delaying it by the ~0.1 ms the host needs to issue them."""
    if order not in _FORWARD_SEQUENCES:
        raise ValueError(f"_FWD_ORDER must be one of {sorted(_FORWARD_SEQUENCES)}, got {order!r}")
    return _FORWARD_SEQUENCES[order] if ordered else [_FwdIssue(_DOC, 0, None, False), _FwdIssue(_QRY, 0, None, False)]


_ORDER_EVENTS = {}


def _order_events(device):
    """Two hipEvents per device (tt_event_create: plain HIP events the C calls record / wait on, include/tt.h tt_enc_sync_t)."""
    key = (device.type, device.index)
    if key not in _ORDER_EVENTS:
        evs = []
        with torch.cuda.device(device):
            for _ in range(2):
                e = C.c_void_p()
                _lib.check(_lib.lib().tt_event_create(C.byref(e)))
                evs.append(e.value)
        _ORDER_EVENTS[key] = tuple(evs)
    return _ORDER_EVENTS[key]


# ---- the direct step ---------------------------------------------------------------------------------------------------------
class _Capture(NamedTuple):
    """What only a direct step under stream capture carries (GraphedTrainStep).  Such a step joins the towers' streams on the
    CALLER's stream (loss and optimizer run there) instead of on the document tower's.  Eagerly that would cost two hops per join
    on the critical path (~20 us each); under capture it is free (the hops are graph edges) and it is the only form this ROCm can
    capture: a side stream that waits for ANOTHER side stream and then goes on makes hipStreamEndCapture crash inside the runtime
    (tools/experiments/graph_pattern_probe.py: fork / join through the origin stream is fine, side-to-side joins segfault,
    whatever the kernels).  For the same reason it carries no ordering events (an event edge between the two tower streams is a
    side-to-side edge; with the query tower moved onto the capturing stream it can be captured, but replays slower: 1.19-1.21 ms
    against 1.16 with the smaller tower on the one-workgroup recurrences, profiles/r04_m_graph_probe.log)."""
    phase: str                          # "all" = through optimizer.step(); "fold" = up to the gate words behind the gradients
    #                                     (optimizer._fold_status): the caller reduces and applies -- with a process group the
    #                                     all-reduce stays outside the captured graph
    both: Optional[torch.Tensor]        # the 2B-row document batch [pos_docs; neg_docs], staged outside the graph (None: the batch's)
    seed_words: Optional[dict]          # {id(encoder): device int64[1]}: the towers' dropout seeds as device words the kernels read
    #                                     when they run (TT_ENC_SEED_ON_DEVICE); None: drawn in the step, passed by value


class _TowerForward(NamedTuple):
    """What a tower's forward leaves for its backward."""
    out: torch.Tensor
    ws: torch.Tensor
    status: torch.Tensor
    dropout_p: float
    seed: object
    opts_bwd: int


class _DirectStep:
    """One direct step in flight: what its stages -- forward towers, loss, backward towers, apply or fold -- hand to each other."""

    def __init__(self, model, optimizer, spec, capture, labels=None, targets=None):
        self.model, self.optimizer, self.spec, self.capture = model, optimizer, spec, capture
        self.labels = labels     # the batch's group labels [2B] (_batch_labels), None: none
        self.targets = targets   # the batch's soft targets [B, 2B] or [B, world * 2B] (_batch_targets), None: none
        self.encs = (model.doc_encoder, model.query_encoder)
        self.ordered = False     # the forward recurrences are ordered by events (syncs: what a call of each kind carries)
        self.into = self.ids_of = self.streams = self.cur = self.s_main = self.syncs = None
        self.fw = [None, None]
        self.loss = self.d_out = None

    def join(self):   # s_main waits for both towers
        for t in reversed(self.streams):
            if t is not self.s_main:
                self.s_main.wait_stream(t)

    def fork(self):   # both towers wait for s_main
        for t in reversed(self.streams):
            if t is not self.s_main:
                t.wait_stream(self.s_main)


def _standard_batch(batch) -> bool:
    """Ids on the GPU, as many negatives as positives as queries, the documents int64 already (tt_concat_ids_i64 reads them as
    they are): the batch of the direct step and of a captured one."""
    queries, pos_docs, neg_docs = batch
    return (queries.is_cuda and neg_docs.shape[0] == pos_docs.shape[0] == queries.shape[0]
            and pos_docs.dtype == neg_docs.dtype == torch.int64)


def _frozen_tables(model: TwoTowerModel) -> bool:
    return not any(e.embedding.weight.requires_grad for e in (model.doc_encoder, model.query_encoder))


def _direct_grad_views(model, optimizer, batch, spec, capture):
    """Does the direct step apply -- and if so, into which of the optimizer's gradient views the towers' backwards write: [the
    document tower's, the query tower's], one view per _flat_params() entry.  None: it does not (the step was asked not to, a
    batch of another shape, another optimizer, a trainable embedding table, a tower in eval mode, parameters without the
    optimizer's gradient views or views no call of the step would write, an exchange of passages inside a capture or without a
    Collective): the caller takes the autograd path, which computes the same numbers.  Looks, touches nothing."""
    if not isinstance(optimizer, _FlatClipAdam) or not torch.is_grad_enabled():
        return None
    if capture is None and not (spec.direct and spec.concurrent_towers):
        return None
    if (capture is None or capture.both is None) and not _standard_batch(batch):
        return None
    if spec.gather_negatives and (capture is not None or getattr(optimizer, "_coll", None) is None):
        return None
    encs = (model.doc_encoder, model.query_encoder)
    if not _frozen_tables(model) or not all(enc.training for enc in encs):
        return None
    views = {id(p): gv for p, gv in zip(optimizer.params, optimizer._views)}
    params = [enc._flat_params() for enc in encs]
    # the optimizer's parameters are exactly the towers', but for one: a learnable LogitScale's word, BEHIND them all (the query
    # tower's gradients stay the bucket's prefix: reduce_prefix), which the loss launch writes itself (_direct_loss)
    own = len(optimizer.params)
    scale = spec.temperature
    if isinstance(scale, LogitScale) and scale.log_scale.requires_grad and optimizer.params[-1] is scale.log_scale:
        own -= 1
    if any(id(p) not in views for ps in params for p in ps) or len({id(p) for ps in params for p in ps}) != own:
        return None
    return [[views[id(p)] for p in ps] for ps in params]


def _forward_towers(st: _DirectStep, batch) -> None:
    queries, pos_docs, neg_docs = batch
    s_doc = st.streams[_DOC]
    both = st.capture.both if st.capture is not None else None
    if both is None:
        with torch.cuda.stream(s_doc):  # (on the document tower's own stream: no hop from the caller's)
            pos_docs.record_stream(s_doc)
            neg_docs.record_stream(s_doc)
            both = _concat_ids(pos_docs, neg_docs)
    st.ids_of = (both, queries)
    # dropout seeds from torch's CPU generator in the order the autograd path draws them (query tower, then document tower)
    seeds = st.capture.seed_words if st.capture is not None and st.capture.seed_words is not None else _draw_dropout_seeds(st.model)
    begun = None
    for tower, phase, event, one_workgroup in _forward_sequence(st.ordered, _FWD_ORDER):
        enc, ids, s = st.encs[tower], st.ids_of[tower], st.streams[tower]
        if s is not st.cur and phase != _lib.TT_ENC_PHASE_FINISH:
            s.wait_stream(st.cur)
        with torch.cuda.stream(s):
            ids.record_stream(s)
            p_drop, seed = enc.dropout, seeds[id(enc)]
            # (the encoders are watched -- _towers_in_flight -- so the status word goes to the optimizer instead of a read here)
            res = enc._run_forward(ids, train=True, dropout_p=p_drop, dropout_seed=seed, sync=st.syncs[event], phase=phase,
                                   resume=begun if phase == _lib.TT_ENC_PHASE_FINISH else None,
                                   opts=enc._opts() | _lib.TT_ENC_ONE_WORKGROUP if one_workgroup else None)
            if phase == _lib.TT_ENC_PHASE_BEGIN:
                begun = res
            else:
                st.fw[tower] = _TowerForward(*res, p_drop, seed, enc._opts_bwd())


def _direct_loss(spec: _StepSpec, optimizer, q, pn, s_main, labels=None, targets=None):
    """The fused loss + gradient launch of the step's kind on s_main (the current stream): (loss, dq, dpn) for the towers' outputs
    q [B,H] and pn [2B,H] (positives, then negatives).  The kinds share the buffers; "in_batch" swaps the one launch, nothing else.
    gather_negatives: the loss runs over the passages of ALL ranks: all-gather of pn into the pool G [world * 2B, H] (rank order),
    tt_contrastive_loss_f32(q, G, pos_offset = rank * 2B) -> loss, dq, dG, summing all-reduce of dG, dpn = this rank's 2B rows of
    it.  Both collectives go out whatever the towers' status words say, in front of the query tower's reduce_prefix: every rank
    issues gather, reduce, (prefix,) bucket in that order.
    labels (the batch's group labels [2B], "in_batch" only): the grouped pool entry on pn as it lies (the in-batch entry's bits
    where no label matches); gathered, the ranks' labels travel like the passages, by an all-gather right behind theirs --
    gather, label gather, reduce on every rank.
    targets (the batch's soft targets, "in_batch" only, never with labels): the soft entry on pn as it lies (M = 2B; the in-batch
    entry's bits for one-hot targets); gathered, on the pool with this rank's rows [B, world * 2B] -- the targets are rank-local,
    so no collective is added and their order stays gather, reduce.
    spec.symmetric > 0 ("in_batch" only, never gathered, never with targets): the symmetric entry on pn as it lies (M = 2B,
    pos_offset = 0), with the labels when there are any.
    spec.temperature a LogitScale: every kind above goes to the two *_ls entries instead, on the pool or on pn as it lies (plain
    "in_batch" as the pool form, M = 2B: the two-pointer entry's bits), which read the module's word where it lies -- inside the
    optimizer's flat_params when it is learnable -- and write d loss / d log_scale straight into that parameter's gradient view.
    Gathered, that is this rank's queries' sum; it rides the bucket's all-reduce and 1 / world like every gradient: no collective
    is added."""
    (B, H), dev = q.shape, q.device
    scale = spec.temperature if isinstance(spec.temperature, LogitScale) else None
    d_scale = _scale_grad_view("train step", spec, optimizer)
    loss = torch.empty((), dtype=torch.float32, device=dev)
    dq = torch.empty_like(q)
    pool_labels = labels
    if spec.gather_negatives:
        coll = optimizer._coll
        pool = torch.empty((coll.world * 2 * B, H), dtype=torch.float32, device=dev)
        d_pool = torch.empty_like(pool)
        dpn = d_pool[coll.rank * 2 * B:(coll.rank + 1) * 2 * B]
        if scale is not None:
            rows = scaled_workspace(B, pool.shape[0], H, dev, soft=targets is not None)
        else:
            rows = (soft_contrastive_workspace if targets is not None else contrastive_workspace)(B, pool.shape[0], H, dev)
        if labels is not None:
            pool_labels = torch.empty(coll.world * 2 * B, dtype=torch.int64, device=dev)
    else:
        dpn = torch.empty_like(pn)
        if scale is not None:
            rows = scaled_workspace(B, 2 * B, H, dev, soft=targets is not None, symmetric=spec.symmetric > 0)
        elif targets is not None:
            rows = soft_contrastive_workspace(B, 2 * B, H, dev)
        elif spec.symmetric > 0:
            rows = symmetric_workspace(B, 2 * B, H, dev)
        elif labels is not None:
            rows = contrastive_workspace(B, 2 * B, H, dev)
        else:
            rows = in_batch_workspace(B, H, dev) if spec.negatives == "in_batch" else torch.empty(B, dtype=torch.float32, device=dev)
    for t in (q, pn, loss, dq, dpn, rows) + (() if labels is None else (labels, pool_labels)) + (() if targets is None else (targets,)):
        t.record_stream(s_main)
    L, p, n = _lib.lib(), pn[:B], pn[B:]
    with torch.cuda.device(dev):
        if scale is not None:
            docs, d_docs, pos = (pool, d_pool, coll.rank * 2 * B) if spec.gather_negatives else (pn, dpn, 0)
            if spec.gather_negatives:
                coll.all_gather_blocks(pn, pool)
                if labels is not None:
                    coll.all_gather_blocks(labels, pool_labels)
            # (the queries' labels are the first B of this rank's passages': the positives')
            _scaled_call(q, docs, pos, scale, spec.symmetric if spec.symmetric > 0 else None, labels, pool_labels, targets, loss,
                         None, d_scale, dq, d_docs, stream=s_main.cuda_stream, ws=rows)
            if spec.gather_negatives:
                coll.all_reduce_sum(d_pool.view(-1))
        elif spec.gather_negatives:
            coll.all_gather_blocks(pn, pool)
            if targets is not None:
                _lib.check(L.tt_contrastive_loss_soft_f32(q.data_ptr(), B, pool.data_ptr(), pool.shape[0], H, targets.data_ptr(),
                                                          float(spec.temperature), loss.data_ptr(), dq.data_ptr(), d_pool.data_ptr(),
                                                          rows.data_ptr(), rows.numel(), s_main.cuda_stream))
            elif labels is None:
                _lib.check(L.tt_contrastive_loss_f32(q.data_ptr(), B, pool.data_ptr(), pool.shape[0], H, coll.rank * 2 * B,
                                                     float(spec.temperature), loss.data_ptr(), dq.data_ptr(), d_pool.data_ptr(),
                                                     rows.data_ptr(), rows.numel(), s_main.cuda_stream))
            else:
                coll.all_gather_blocks(labels, pool_labels)
                _lib.check(L.tt_contrastive_loss_grouped_f32(q.data_ptr(), B, pool.data_ptr(), pool.shape[0], H, coll.rank * 2 * B,
                                                             labels.data_ptr(), pool_labels.data_ptr(), float(spec.temperature),
                                                             loss.data_ptr(), dq.data_ptr(), d_pool.data_ptr(), rows.data_ptr(),
                                                             rows.numel(), s_main.cuda_stream))
            # (no scale: a summed row is sum_r d loss_r / d D_j, and the optimizer's 1 / world makes it the mean's)
            coll.all_reduce_sum(d_pool.view(-1))
        elif targets is not None:
            _lib.check(L.tt_contrastive_loss_soft_f32(q.data_ptr(), B, pn.data_ptr(), 2 * B, H, targets.data_ptr(),
                                                      float(spec.temperature), loss.data_ptr(), dq.data_ptr(), dpn.data_ptr(),
                                                      rows.data_ptr(), rows.numel(), s_main.cuda_stream))
        elif spec.symmetric > 0:
            lp = None if labels is None else labels.data_ptr()
            _lib.check(L.tt_contrastive_loss_sym_f32(q.data_ptr(), B, pn.data_ptr(), 2 * B, H, 0, lp, lp, float(spec.temperature),
                                                     float(spec.symmetric), loss.data_ptr(), None, dq.data_ptr(), dpn.data_ptr(),
                                                     rows.data_ptr(), rows.numel(), s_main.cuda_stream))
        elif labels is not None:
            # (the queries' labels are the first B of the passages': the positives')
            _lib.check(L.tt_contrastive_loss_grouped_f32(q.data_ptr(), B, pn.data_ptr(), 2 * B, H, 0, labels.data_ptr(),
                                                         labels.data_ptr(), float(spec.temperature), loss.data_ptr(), dq.data_ptr(),
                                                         dpn.data_ptr(), rows.data_ptr(), rows.numel(), s_main.cuda_stream))
        elif spec.negatives == "in_batch":
            _lib.check(L.tt_in_batch_loss_f32(q.data_ptr(), p.data_ptr(), n.data_ptr(), B, H, float(spec.temperature),
                                              loss.data_ptr(), dq.data_ptr(), dpn[:B].data_ptr(), dpn[B:].data_ptr(),
                                              rows.data_ptr(), rows.numel(), s_main.cuda_stream))
        else:
            _lib.check(L.tt_triplet_loss_f32(q.data_ptr(), p.data_ptr(), n.data_ptr(), B, H, float(spec.margin), loss.data_ptr(),
                                             dq.data_ptr(), dpn[:B].data_ptr(), dpn[B:].data_ptr(), rows.data_ptr(),
                                             s_main.cuda_stream))
    return loss, dq, dpn


def _loss_and_embedding_grads(st: _DirectStep) -> None:
    """On the stream where the towers meet.  Eagerly that is the document tower's: it carries the step's critical path from here
    on -- the loss, the document backward and the optimizer are enqueued on IT (a hop to the caller's stream and back cost ~20 us
    each way on that path: event wait + launch); the query tower's stream joins for the loss and again before the optimizer."""
    st.join()
    with torch.cuda.stream(st.s_main):
        st.loss, dq, dpn = _direct_loss(st.spec, st.optimizer, st.fw[_QRY].out, st.fw[_DOC].out, st.s_main, st.labels,
                                            st.targets)
    st.d_out = (dpn, dq)


def _complete_prefix(optimizer, grads) -> int:
    """How many of the bucket's leading gradients `grads` are, when they are its prefix without a gap (0: they are not)."""
    base = optimizer.flat_grads.data_ptr()
    spans = sorted(((g.data_ptr() - base) // 4, g.numel()) for g in grads)
    if spans[0][0] == 0 and all(a + n == b for (a, n), (b, _) in zip(spans, spans[1:])):
        return spans[-1][0] + spans[-1][1]
    return 0


def _backward_towers(st: _DirectStep) -> None:
    """Each tower's backward on its own stream, written STRAIGHT into the optimizer's gradient views.  No events: the plan gave
    the smaller tower the one-workgroup recurrence (_towers_in_flight)."""
    optimizer = st.optimizer
    st.fork()
    for enc, ids, s, f, d_out, grads in zip(st.encs, st.ids_of, st.streams, st.fw, st.d_out, st.into):
        with torch.cuda.stream(s):
            d_out.record_stream(s)
            # (a time-out of the split backward recurrence ORs bit 2 into the forward's word, which the optimizer reads)
            enc._run_backward(ids.contiguous(), f.ws, d_out, f.dropout_p, f.seed, into=grads, status=f.status, opts=f.opts_bwd)
            if enc is st.model.query_encoder and optimizer.world > 1 and st.capture is None:
                # data-parallel: the query tower's gradients are complete long before the document tower's (its backward is
                # a tenth of the tokens) -- when they are the bucket's prefix their all-reduce goes out HERE, on the query
                # tower's stream, and runs under the document tower's weight-gradient kernels; the rest of the bucket (with
                # the gate words) follows in optimizer.step()
                upto = _complete_prefix(optimizer, grads)
                if upto:
                    optimizer.reduce_prefix(upto)
    st.join()


def _apply_or_fold(st: _DirectStep) -> None:
    optimizer = st.optimizer
    for p_, gv in zip(optimizer.params, optimizer._views):
        p_.grad = gv
    with torch.cuda.stream(st.s_main):
        # The optimizer is enqueued unconditionally: the towers' status words (zero-length rows / ids out of range raise as
        # in the reference; a column-split recurrence that gave up) are folded into the gate behind the gradients, reduced
        # over the ranks with them, and the device applies the step on every rank or on none.  The read of the reduced gate
        # inside step() is the one host synchronisation of the step; for a bad batch the weights stay untouched (the
        # gradient buffer holds garbage, which the next step overwrites).
        for t in (optimizer.flat_params, optimizer._bucket, optimizer.exp_avg, optimizer.exp_avg_sq, optimizer.total_norm,
                  optimizer._scratch, optimizer._step_dev):
            t.record_stream(st.s_main)
        if st.capture is None or st.capture.phase == "all":
            optimizer.step()
        else:
            optimizer._fold_status()


def _train_step_direct(model: TwoTowerModel, optimizer, batch, spec: _StepSpec, plan: Optional[_towers_in_flight],
                       capture: Optional[_Capture], labels: Optional[torch.Tensor] = None,
                       targets: Optional[torch.Tensor] = None):
    """The same step without the autograd engine: tower forwards (train mode), the fused loss + gradient kernel, tower backwards
    written STRAIGHT into the optimizer's flat gradient buffer, optimizer step.  Every parameter receives its gradient exactly
    once (query tower once; positives and negatives as one 2B-row document-tower call), so nothing has to be zeroed or
    accumulated: what the autograd path adds per step -- grad_output plumbing around the loss, four accumulate-adds per
    tower, the 3.4 MB zero fill -- is ~0.1 ms of small launches on the document tower's critical path.  Returns None when the
    shortcut does not apply (_direct_grad_views): the caller then takes the autograd path.
    batch: (queries, pos_docs, neg_docs); plan: the step's _towers_in_flight -- when the two towers' split recurrences do not fit
    the device together their forward recurrence launches are ordered with events; capture: None for the eager step; labels: the
    batch's group labels (_batch_labels), None: none; targets: its soft targets (_batch_targets), None: none."""
    st = _DirectStep(model, optimizer, spec, capture, labels, targets)
    st.into = _direct_grad_views(model, optimizer, batch, spec, capture)
    if st.into is None:
        return None
    dev = batch[0].device
    st.cur = cur = torch.cuda.current_stream(dev)
    st.streams = s_doc, s_qry = _tower_streams(dev)[:2]
    if capture is not None and plan is not None:
        plan.use_one_workgroup()      # (no ordering events in a capture: _Capture)
    st.ordered = plan is not None and plan.needs_order
    st.s_main = cur if capture is not None else s_doc     # where the towers meet: loss, optimizer
    st.syncs = {None: None}
    if st.ordered:
        ev_f, _ = _order_events(dev)
        st.syncs.update(record=_lib.EncSync(None, ev_f), wait=_lib.EncSync(ev_f, None))
    try:
        s_doc.wait_stream(cur)
        _forward_towers(st, batch)
        _loss_and_embedding_grads(st)
        _backward_towers(st)
        _apply_or_fold(st)
    finally:
        # (also when step() raised: the caller's stream joins the towers' streams, nothing of this step is left running
        #  behind the caller's back)
        for t in (s_qry, s_doc):
            if t is not cur:
                cur.wait_stream(t)
    st.loss.record_stream(cur)
    return st.loss


def _draw_dropout_seeds(model: TwoTowerModel) -> dict:
    """{id(encoder): seed} from torch's CPU generator in the order the autograd path draws them (query tower, then document
    tower); 0 for a tower without inter-layer dropout (nothing is drawn for it)."""
    return {id(enc): (int(torch.randint(0, 2 ** 62, (1,)).item()) if enc.dropout > 0.0 else 0)
            for enc in (model.query_encoder, model.doc_encoder)}


# ---- the autograd step and the entries ---------------------------------------------------------------------------------------
class _GatherPoolFn(torch.autograd.Function):
    """This rank's passages pn [2B,H] -> the pool of all ranks [world * 2B, H], rank order (Collective.all_gather_blocks).
    Backward: summing all-reduce of the pool's gradient -- every rank's loss has a gradient for every row -- and this rank's rows."""

    @staticmethod
    def forward(ctx, pn, coll):
        pn = pn.contiguous()
        pool = torch.empty((coll.world * pn.shape[0], pn.shape[1]), dtype=pn.dtype, device=pn.device)
        coll.all_gather_blocks(pn, pool)
        ctx.coll, ctx.rows = coll, pn.shape[0]
        return pool

    @staticmethod
    def backward(ctx, d_pool):
        d_pool = d_pool.contiguous().clone()  # (reduced in place: not the engine's tensor)
        ctx.coll.all_reduce_sum(d_pool.view(-1))
        return d_pool[ctx.coll.rank * ctx.rows:(ctx.coll.rank + 1) * ctx.rows], None


def _autograd_loss(spec: _StepSpec, optimizer, embeddings, pn, labels=None, targets=None):
    """The loss of the step's kind as an autograd graph over the towers' outputs (q, p, n); pn: the 2B passages as one tensor
    when the document tower ran once (None: it did not).  Gathered: the loss of this rank's queries over the passages of all ranks.
    labels: the batch's group labels [2B] (_batch_labels); gathered, the ranks' labels are gathered right behind the passages.
    targets: the batch's soft targets (_batch_targets), over [p; n] or, gathered, over the pool: soft_contrastive_loss."""
    if spec.gather_negatives:
        coll = getattr(optimizer, "_coll", None)
        if coll is None:
            raise ValueError("gather_negatives=True needs a FusedClipAdam (the passages travel through its Collective)")
        if pn is None:
            pn = torch.cat(embeddings[1:])
        pool = _GatherPoolFn.apply(pn, coll)
        if targets is not None:
            return soft_contrastive_loss(embeddings[0], pool, targets, temperature=spec.temperature)
        if labels is None:
            return contrastive_softmax_loss(embeddings[0], pool, pos_offset=coll.rank * pn.shape[0], temperature=spec.temperature)
        pool_labels = torch.empty(coll.world * labels.shape[0], dtype=torch.int64, device=labels.device)
        coll.all_gather_blocks(labels, pool_labels)
        return contrastive_softmax_loss(embeddings[0], pool, pos_offset=coll.rank * pn.shape[0], temperature=spec.temperature,
                                        q_groups=labels[:embeddings[0].shape[0]], doc_groups=pool_labels)
    if spec.negatives == "in_batch":
        if targets is not None:
            return soft_contrastive_loss(embeddings[0], pn if pn is not None else torch.cat(embeddings[1:]), targets,
                                         temperature=spec.temperature)
        if labels is not None:
            B = embeddings[0].shape[0]
            return in_batch_softmax_loss(embeddings, temperature=spec.temperature, groups=labels[:B], neg_groups=labels[B:],
                                         symmetric=spec.symmetric)
        return in_batch_softmax_loss(embeddings, temperature=spec.temperature, symmetric=spec.symmetric)
    return triplet_loss_cosine(embeddings, margin=spec.margin)


def _train_step_once(model, optimizer, batch, spec: _StepSpec, plan: _towers_in_flight, labels=None, targets=None):
    loss = _train_step_direct(model, optimizer, batch, spec, plan, None, labels, targets)
    if loss is not None:
        return loss
    plan.use_one_workgroup()   # (autograd calls cannot carry the ordering events)
    queries, pos_docs, neg_docs = batch
    optimizer.zero_grad()
    pn = None   # (the 2B passages as one tensor, when the document tower ran once)
    if spec.concurrent_towers and queries.is_cuda:
        cur = torch.cuda.current_stream(queries.device)
        B = pos_docs.shape[0]
        if neg_docs.shape[0] == B:
            # positives and negatives go through the SAME tower: one call over 2B rows (rows are independent),
            # so the recurrence kernels fill twice the CUs and the weight-gradient GEMMs run once
            both = _concat_ids(pos_docs.long(), neg_docs.long())
            calls = ((model.encode_query, queries), (model.encode_document, both))
        else:
            calls = ((model.encode_query, queries), (model.encode_document, pos_docs), (model.encode_document, neg_docs))
        outs = []

        def launch():
            for s, (fn, ids) in zip(_tower_streams(queries.device), calls):
                s.wait_stream(cur)
                with torch.cuda.stream(s):
                    ids.record_stream(s)
                    outs.append(fn(ids))
            for s, o in zip(_tower_streams(queries.device), outs):
                cur.wait_stream(s)
                o.record_stream(cur)
        if isinstance(optimizer, _FlatClipAdam):
            launch()  # (the status words go to the optimizer, which reads them -- reduced over the ranks -- in step())
        else:
            # another optimizer: input checking stays on (zero-length rows / out-of-range ids raise as in the reference), but the
            # status words of the towers are read ONCE, after all of them have been enqueued: a per-call read would make the
            # host wait for the query tower before it could launch the document tower
            with deferred_input_checks(model.query_encoder, model.doc_encoder):
                launch()
        if len(outs) == 2:
            q, p, n = outs[0], outs[1][:B], outs[1][B:]
            pn = outs[1]
        else:
            q, p, n = outs
    else:
        q = model.encode_query(queries)
        p = model.encode_document(pos_docs)
        n = model.encode_document(neg_docs)
    loss = _autograd_loss(spec, optimizer, (q, p, n), pn, labels, targets)
    loss.backward()
    optimizer.step()
    return loss.detach()


def _eager_step(model, optimizer, batch, spec: _StepSpec, labels=None, targets=None):
    """One step with the read of the gate wherever optimizer.check puts it; a time-out of a column-split recurrence redoes the
    step on the one-workgroup kernels (ordinary relaunch, same bits as the split forward), with the same labels and targets."""
    queries, pos_docs, neg_docs = batch
    encs = (model.query_encoder, model.doc_encoder)
    n_doc = pos_docs.shape[0] + neg_docs.shape[0] if (spec.concurrent_towers and neg_docs.shape[0] == pos_docs.shape[0]) else max(
        pos_docs.shape[0], neg_docs.shape[0])
    rows = {model.query_encoder: queries.shape[0], model.doc_encoder: n_doc} if spec.concurrent_towers else {}
    rng = torch.get_rng_state() if any(e.dropout > 0.0 and e.training for e in encs) else None
    try:
        with _towers_in_flight(model, optimizer, rows if queries.is_cuda else {}) as plan:
            return _train_step_once(model, optimizer, batch, spec, plan, labels, targets)
    except SplitRecurrenceTimeout:
        if rng is not None:
            torch.set_rng_state(rng)  # (the redone step draws the dropout seeds the failed attempt drew)
        with _towers_in_flight(model, optimizer, {}, force_one_workgroup=True) as plan:
            return _train_step_once(model, optimizer, batch, spec, plan, labels, targets)


def _step(model, optimizer, batch, spec: _StepSpec, defer_check: bool, labels=None, targets=None):
    """train_step behind its argument list (DataParallelTrainer.step enters here with its own record).  labels: _batch_labels;
    targets: _batch_targets."""
    queries, pos_docs, neg_docs = batch
    if spec.gather_negatives and not queries.shape[0] == pos_docs.shape[0] == neg_docs.shape[0]:
        raise ValueError("gather_negatives=True needs as many negatives as positives as queries")
    if not (defer_check and isinstance(optimizer, _FlatClipAdam) and queries.is_cuda):
        return _eager_step(model, optimizer, batch, spec, labels, targets)
    keep, optimizer.check = optimizer.check, False
    try:
        loss = _eager_step(model, optimizer, batch, spec, labels, targets)
    finally:
        optimizer.check = keep
    if keep:
        optimizer.snapshot_gate(redo=lambda: _eager_step(model, optimizer, batch, spec, labels, targets))
    return loss


def train_step(model: TwoTowerModel, optimizer: FusedClipAdam, queries: torch.Tensor, pos_docs: torch.Tensor,
               neg_docs: torch.Tensor, margin: float = 0.2, concurrent_towers: bool = True, direct: bool = True,
               defer_check: bool = False, negatives: str = "paired", temperature: float = 0.05,
               gather_negatives: bool = False, groups: Optional[torch.Tensor] = None,
               neg_groups: Optional[torch.Tensor] = None, targets: Optional[torch.Tensor] = None,
               symmetric: float = 0.0) -> torch.Tensor:
    """One step of backend/main.py:244-259 on this rank's (equal-sized) share of the global batch.
    Returns the local loss as a 0-d device tensor (no .item(): the reference's per-step sync is dropped).

    concurrent_towers: the encoder calls are independent, so the query tower and the document tower (positives and negatives in
    one 2B-row call) are issued on separate HIP streams (autograd replays each call's backward on the stream its forward ran on).
    direct: skip the autograd engine when the step has the standard shape (_train_step_direct: same kernels, same numbers).

    Failure is collective (FusedClipAdam): a zero-length row or an id out of range on ANY rank raises the reference's
    exception on EVERY rank, inside this call, with parameters, moments and step number untouched everywhere.  A time-out of a
    column-split recurrence (transient: CUs held by other work) does not raise: all ranks see it in the same reduced gate and
    redo the step on the one-workgroup kernels (ordinary relaunch, same bits as the split forward).

    defer_check (FusedClipAdam only): the step's one host synchronisation -- the read of the reduced gate words -- moves one call
    back: the words are copied to pinned memory behind the step and looked at inside the NEXT call (or optimizer.settle()), after
    that step has been enqueued, so the host runs ahead of the GPU and the ~0.1 ms the GPU idles per step while the host
    enqueues the next 40 launches is gone.  A bad batch's exception then comes out one call late; its step was not applied
    (the device decided that), the step behind it is an ordinary step on the same weights.

    negatives: "paired" (default) = the reference's triplet loss, one hinge per row against its own negative.  "in_batch" = the
    softmax contrastive loss over all 2B passages of the batch (model.in_batch_softmax_loss) at `temperature`; `margin` is
    ignored; needs as many negatives as positives as queries.  The negatives are rank-local (each rank's softmax runs over its
    own 2B passages, the gradients are averaged over the ranks as always) unless gather_negatives=True.

    gather_negatives (negatives="in_batch" only): every query is scored against the passages of ALL ranks -- world * 2B - 1
    negatives instead of 2B - 1.  Two collectives of the optimizer's Collective per step, between the towers' forwards and
    backwards: an all-gather of the rank's 2B passage embeddings into a pool [world * 2B, H], and a summing all-reduce of the
    pool's gradient (every rank's loss has a gradient for every passage), of which the rank keeps its own 2B rows.  With the
    optimizer's 1/world the update is the gradient of the mean of the ranks' losses, which is the loss of the global batch.
    Every rank must bring the same B.  Returns the rank's own loss: the mean over its B queries against the global pool.
    Both collectives are issued whatever the batch holds, so failure stays collective (above); a redo after a recurrence
    time-out repeats them on all ranks.  One process without a group: the same bits as without the flag.

    groups / neg_groups (negatives="in_batch" only; int64 [B] on the batch's device): grouped negatives.  Row i's query and
    positive carry groups[i], its negative neg_groups[i] (None: -1, no group).  A passage that carries a query's label >= 0, other
    than the query's own positive, is left out of that query's softmax (model.contrastive_softmax_loss): a batch that holds one
    query several times, each with another of its positives, gives the copies one label, and they stop pushing each other's
    positives away.  Derive the label from the loader's query index.  With gather_negatives=True the ranks'
    labels are all-gathered right behind the passages (one more collective, in front of the summing all-reduce), so labels must
    be global (the same query has the same label on every rank) and EVERY rank must pass labels, or none -- like "every rank
    must bring the same B".  The direct and the autograd path give the same bits; a redo keeps the labels.

    targets (negatives="in_batch" only, never with groups / neg_groups; float32 [B, 2B] on the batch's device): soft targets, a
    weight per (query, passage of [p; n]) in place of the one positive per query -- model.soft_contrastive_loss: distillation
    from a teacher (model.distillation_targets) or several positives per query, each pulled (model.multi_positive_targets).
    One-hot targets (1 at column i) give the bits of the plain "in_batch" step.  With gather_negatives=True the targets are
    [B, world * 2B] with the columns in pool order (rank r's [p_r; n_r] at column r * 2B); they are this rank's own rows, so no
    collective is added.  Not differentiated.  The direct and the autograd path give the same bits; a redo keeps the targets.

    symmetric (negatives="in_batch" only; a number in [0, 1]): the weight alpha of the document-to-query direction.  The loss
    becomes (1 - alpha) L_qd + alpha L_dq (model.contrastive_softmax_loss): each positive passage is also classified among the
    batch's B queries; the explicit negatives have no query of their own and stay negatives of the queries alone.  0.5 is the
    CLIP loss; 0.0 (default) is the one-directional step, launch for launch.  Combines with groups / neg_groups (an ignored
    pair leaves both softmaxes), not with targets (soft targets define their own rows; there are no column targets) and not
    with gather_negatives=True (the column softmax would run over the queries of all ranks: a gather of the queries and a
    reduction of their gradients, a second exchange in the step's collective order).  The negatives are rank-local.

    temperature (negatives="in_batch" only when it is a module): a float, or a model.LogitScale -- a temperature that lives on
    the device.  Learnable, the optimizer must own its word (ValueError otherwise): FusedClipAdam(list(model.parameters()) +
    list(scale.parameters())), the scale's behind the model's; the loss kernels return d loss / d log_scale (every kind: plain,
    grouped, soft, symmetric, gathered) and Adam updates the word with the weights.  Its gradient lies in the optimizer's flat
    buffer, so it is part of the global clip norm.  Multi-rank it is averaged over the ranks like every gradient.  Not learnable
    (LogitScale(learnable=False)), the word is a fixed temperature that a schedule may rewrite between steps."""
    spec = _StepSpec(margin, negatives, temperature, gather_negatives, concurrent_towers, direct, symmetric).checked(graphs=False)
    _scale_grad_view("train_step", spec, optimizer)
    batch = (queries, pos_docs, neg_docs)
    targets = _batch_targets("train_step", spec, optimizer, batch, targets, groups, neg_groups)
    return _step(model, optimizer, batch, spec, defer_check, _batch_labels("train_step", spec, batch, groups, neg_groups), targets)


class DataParallelTrainer:
    """Replicated model, per-rank batch shard, gradient all-reduce (with the step's failure gate) inside FusedClipAdam.step().

    graphs=True: steps are replayed from HIP graphs (GraphedTrainStep), one per (batch, query width, document width) bucket --
    widths rounded up to `width_step` columns, the `max_graphs` most recently used buckets kept (a graph owns its workspaces:
    ~0.3 GB at 512 triplets x 128 columns).  A batch that does not fit the rules of GraphedTrainStep (unchecked inputs,
    non-int64 ids, a trainable table) takes the eager train_step; results are the eager step's on ids padded to the bucket's widths.
    defer_check: see GraphedTrainStep (exceptions one call late; call flush() after the last step).
    negatives / temperature / gather_negatives: see train_step.  "in_batch" negatives are rank-local (each rank's softmax over
    its own 2B passages, gradients averaged over the ranks as for the triplet loss) unless gather_negatives=True: then the
    passages of all ranks are gathered and every query sees world * 2B - 1 negatives (every rank must bring the same B; two
    more collectives per step, same order on every rank).  Not with graphs=True.
    symmetric: see train_step (the symmetric "in_batch" loss on each rank's own batch: rank-local negatives, the gradients
    averaged over the ranks as always; not with gather_negatives=True, not with targets).
    temperature: a float or a model.LogitScale (train_step).  The trainer's optimizer takes a learnable module's word behind the
    model's parameters (part of the clip norm, broadcast with them by broadcast_parameters, its gradient -- each rank's own
    queries' sum -- averaged by the bucket's all-reduce; gathered or not, no collective is added); graphs key on the module, not
    on its value."""

    def __init__(self, model: TwoTowerModel, lr: float = 1e-4, margin: float = 0.2, max_norm: float = 1.0, group=None,
                 graphs: bool = False, width_step: int = 32, max_graphs: int = 4, defer_check: bool = False,
                 negatives: str = "paired", temperature: float = 0.05, gather_negatives: bool = False, symmetric: float = 0.0):
        self.graphs, self.width_step, self.max_graphs, self.defer_check = bool(graphs), int(width_step), int(max_graphs), bool(defer_check)
        self.margin = margin
        self.negatives, self.gather_negatives = negatives, bool(gather_negatives)
        self.temperature = temperature if isinstance(temperature, LogitScale) else float(temperature)
        self.symmetric = symmetric
        self._spec()
        self.model = model
        scale_params = list(self.temperature.parameters()) if isinstance(self.temperature, LogitScale) else []
        self.optimizer = FusedClipAdam(list(model.parameters()) + scale_params, lr=lr, max_norm=max_norm, group=group)
        self.optimizer.watch(model)  # (a hand-written loop over self.model / self.optimizer fails collectively too)
        self._graphs: "dict" = {}

    def _spec(self) -> _StepSpec:
        """What a step does now (the attributes may be changed between steps)."""
        return _StepSpec(self.margin, self.negatives, self.temperature, self.gather_negatives, True, True,
                         self.symmetric).checked(self.graphs)

    def broadcast_parameters(self, src: int = 0) -> None:
        import torch.distributed as dist
        if dist.is_initialized() and dist.get_world_size(self.optimizer.group) > 1:
            dist.broadcast(self.optimizer.flat_params, src=src, group=self.optimizer.group)   # (a learnable scale's word included)
            if isinstance(self.temperature, LogitScale) and not self.temperature.log_scale.requires_grad:
                dist.broadcast(self.temperature.log_scale.data, src=src, group=self.optimizer.group)
        self.optimizer.mark_params_changed()  # (the broadcast wrote the flat buffer, not the parameter tensors)

    def _graph_for(self, batch, spec: _StepSpec, grouped: bool = False, soft: bool = False) -> Optional["GraphedTrainStep"]:
        queries, pos_docs, neg_docs = batch
        if not (_standard_batch(batch) and queries.dtype == torch.int64 and _frozen_tables(self.model)
                and self.model.query_encoder.check_inputs and self.model.doc_encoder.check_inputs):
            return None
        up = lambda x: max(self.width_step, -(-int(x) // self.width_step) * self.width_step)  # noqa: E731
        key = (queries.shape[0], up(queries.shape[1]), up(max(pos_docs.shape[1], neg_docs.shape[1])))
        if grouped:
            key += ("grouped",)   # (a step with labels is another graph: its loss node is the grouped entry's; others keep their key)
        if soft:
            key += ("soft",)      # (and so is a step with soft targets: the soft entry's)
        if spec.symmetric > 0:
            key += (("symmetric", float(spec.symmetric)),)   # (the weight is an argument of the captured symmetric entry)
        if isinstance(spec.temperature, LogitScale):
            key += (("scale", id(spec.temperature)),)        # (the module, not its value: the captured launches read its word)
        g = self._graphs.pop(key, None)
        if g is None:
            while len(self._graphs) >= self.max_graphs:           # least recently used first
                self._graphs.pop(next(iter(self._graphs)))
            g = GraphedTrainStep(self.model, self.optimizer, key[0], key[1], key[2], spec.margin, defer_check=self.defer_check,
                                 negatives=spec.negatives, temperature=spec.temperature, grouped=bool(grouped), soft=bool(soft),
                                 symmetric=spec.symmetric)
        self._graphs[key] = g                                      # (re-inserted: most recently used last)
        return g

    def flush(self):
        """defer_check: settle the last step's pending check."""
        return self.optimizer.settle()

    def step(self, queries, pos_docs, neg_docs, groups=None, neg_groups=None, targets=None) -> torch.Tensor:
        """groups / neg_groups: grouped negatives, see train_step (negatives="in_batch" only; with gather_negatives=True every
        rank passes labels or none).  targets: soft targets, see train_step (negatives="in_batch" only, never with labels;
        float32 [B, 2B], with gather_negatives=True [B, world * 2B] in pool order)."""
        self.model.train()
        batch, spec = (queries, pos_docs, neg_docs), self._spec()
        _scale_grad_view("DataParallelTrainer.step", spec, self.optimizer)
        targets = _batch_targets("DataParallelTrainer.step", spec, self.optimizer, batch, targets, groups, neg_groups)
        labels = _batch_labels("DataParallelTrainer.step", spec, batch, groups, neg_groups)
        if self.graphs:
            g = self._graph_for(batch, spec, labels is not None, targets is not None)
            if g is not None:
                return g(queries, pos_docs, neg_docs, groups, neg_groups, targets)
        return _step(self.model, self.optimizer, batch, spec, self.defer_check, labels, targets)


class _SeedRing:
    """The dropout seeds of a captured step: two device words (query tower, document tower) the captured kernels read when they
    run, refilled in front of every replay from one of eight pinned host pairs -- a pair is written again only when the copy
    that read it, eight calls ago, has finished."""

    def __init__(self, device):
        self.words = torch.zeros(2, dtype=torch.int64, device=device)
        self._host = torch.zeros((8, 2), dtype=torch.int64).pin_memory()
        self._events, self._n = [None] * 8, 0

    def put(self, query_seed: int, doc_seed: int) -> None:
        """Enqueue the copy of this call's seeds on the current stream."""
        k = self._n % len(self._events)
        self._n += 1
        if self._events[k] is not None:
            self._events[k].synchronize()   # (this pinned pair was a copy's source eight calls ago: long done)
        self._host[k, 0], self._host[k, 1] = query_seed, doc_seed
        self.words.copy_(self._host[k], non_blocking=True)
        self._events[k] = torch.cuda.Event()
        self._events[k].record()


class GraphedTrainStep:
    """The direct train step of ONE batch shape captured in a HIP graph and replayed: the ~40 launches of a step (two towers on
    two streams, loss, two backwards, gate, clip + Adam) become one graph launch, so the host is out of the step's way -- what
    is left per step is two staging launches (the batch's ids into static buffers, zero-padded), one hipGraphLaunch and the read
    of the gate words (the eager step leaves the GPU idle for ~0.1 ms per step while the host enqueues the next step's launches
    behind its one synchronisation).  Possible because nothing in the captured launches changes from step to step: the step number
    and the bias corrections live on the device (tt_clip_adam_step_gated_f32), the failure decision is a device predicate (the
    gate), and every library call is capture-clean (no allocation, no synchronisation, kernels instead of memsets: include/tt.h).

        step = GraphedTrainStep(model, optimizer, batch=512, q_width=32, doc_width=128, margin=0.5)
        loss = step(queries, pos_docs, neg_docs)      # ids [batch, <= width]

    Padding columns of id 0 change nothing (lengths are counts of non-zero ids, backend/model.py:52): results are bit-identical
    to train_step on ids padded to the same widths (the launch geometry -- slab partitions of the weight-gradient products --
    follows the padded width, so against the UNPADDED eager step the last bits of a gradient sum may differ).
    Failure semantics are train_step's: the reduced gate is read after the replay (the step's one synchronisation) and the
    reference's exceptions are raised, on every rank, with the weights untouched; a recurrence time-out redoes the step eagerly
    on the one-workgroup kernels.  defer_check=True moves that read one step back: step i's gate words are copied to pinned host
    memory behind its replay and looked at inside call i + 1, AFTER step i + 1 has been enqueued -- the GPU never waits for the
    host, and a bad batch's exception comes out of the NEXT call (or of flush()); its step was not applied, the following one
    (already enqueued) is an ordinary step on the same weights.  With a process group the graph ends at the gate words and the
    all-reduce + clip + Adam are issued eagerly behind it (RCCL inside a capture is not rehearsable here).  Needs: the
    optimizer's own parameters on a GPU, GloVe-frozen tables, input checking on (default).  Inter-layer dropout (the reference's
    default model has it) is captured with its seeds as device words (TT_ENC_SEED_ON_DEVICE, include/tt.h): every call draws them
    from torch's CPU generator in the eager step's order and copies them in front of the replay, so a replay computes what the
    eager step would have computed with the generator in the same state.
    grouped=True (negatives="in_batch" only): the captured loss is the grouped entry's; the batch's group labels (train_step:
    groups, neg_groups) are a static int64 input [2B] like the ids, copied in front of the replay.  A call without labels fills
    -1 (no group: the bits of the ungrouped step); neg_groups=None fills -1 for the negatives.
    soft=True (negatives="in_batch" only, not with grouped): the captured loss is the soft entry's; the batch's soft targets
    (train_step: targets) are a static float32 input [B, 2B], refilled in front of every replay.  A call without targets fills
    the one-hot (1 at column i: the bits of the plain "in_batch" step).
    symmetric (negatives="in_batch" only; train_step: symmetric): a captured argument like temperature; > 0 captures the
    symmetric entry as the loss.  Combines with grouped=True; with soft=True it raises ValueError.
    temperature a model.LogitScale (negatives="in_batch" only; train_step: temperature): the captured loss launches read the
    module's word on the device when they run, so nothing about the temperature is frozen into the graph.  Learnable, the word
    lies in the optimizer's flat_params (build the optimizer first: that address is what is captured) and the captured Adam
    updates it: the next replay sees the update with nothing staged.  Not learnable, rewrite the word between calls
    (scale.log_scale.fill_(...) under torch.no_grad()) and replay: a temperature schedule with no recapture."""

    def __init__(self, model: TwoTowerModel, optimizer: FusedClipAdam, batch: int, q_width: int, doc_width: int, margin: float = 0.2,
                 defer_check: bool = False, negatives: str = "paired", temperature: float = 0.05, grouped: bool = False,
                 soft: bool = False, symmetric: float = 0.0):
        # (margin, negatives, a float temperature and symmetric are arguments of the captured loss launches; a LogitScale's word is
        #  read by them on the device)
        temperature = temperature if isinstance(temperature, LogitScale) else float(temperature)
        self._spec = _StepSpec(float(margin), negatives, temperature, False, True, True, symmetric).checked(graphs=True)
        _scale_grad_view("GraphedTrainStep", self._spec, optimizer)
        if grouped and negatives != "in_batch":
            raise ValueError(f'GraphedTrainStep: grouped=True needs negatives="in_batch", got negatives={negatives!r}')
        if soft and negatives != "in_batch":
            raise ValueError(f'GraphedTrainStep: soft=True needs negatives="in_batch", got negatives={negatives!r}')
        if soft and grouped:
            raise ValueError("GraphedTrainStep: soft=True and grouped=True exclude each other")
        if soft and self._spec.symmetric > 0:
            raise ValueError("GraphedTrainStep: soft=True and symmetric > 0 exclude each other (soft targets define their own rows "
                             "and there are no column targets)")
        encs = (model.query_encoder, model.doc_encoder)
        if not isinstance(optimizer, _FlatClipAdam) or optimizer._gated_step_fn is None:
            raise TypeError("GraphedTrainStep needs a FusedClipAdam")
        if not all(e.check_inputs for e in encs):
            raise ValueError("GraphedTrainStep: input checking must be on (the gate is what keeps a bad batch from being applied)")
        self.model, self.optimizer, self.margin = model, optimizer, float(margin)
        self.negatives, self.temperature, self.symmetric = negatives, temperature, float(symmetric)
        self.B, self.q_width, self.doc_width = int(batch), int(q_width), int(doc_width)
        self.defer_check = bool(defer_check)
        dev = optimizer.flat_params.device
        self.q = torch.zeros((self.B, self.q_width), dtype=torch.int64, device=dev)
        self.both = torch.zeros((2 * self.B, self.doc_width), dtype=torch.int64, device=dev)
        self.grouped = bool(grouped)
        self.labels = torch.full((2 * self.B,), -1, dtype=torch.int64, device=dev) if self.grouped else None
        self.soft = bool(soft)
        # (the static targets start as the one-hot that a call without targets refills them with)
        self._one_hot = torch.eye(self.B, 2 * self.B, dtype=torch.float32, device=dev) if self.soft else None
        self.targets = self._one_hot.clone() if self.soft else None
        # inter-layer dropout: the seeds are device words the captured kernels read when they run (TT_ENC_SEED_ON_DEVICE); every
        # call draws them from torch's CPU generator exactly as the eager step does and copies them there in front of the replay
        self._seeds = _SeedRing(dev) if any(e.dropout > 0.0 for e in encs) else None
        words = None if self._seeds is None else {id(model.query_encoder): self._seeds.words[0:1],
                                                  id(model.doc_encoder): self._seeds.words[1:2]}
        self._phase = "all" if optimizer.world == 1 else "fold"
        self._capture = _Capture(self._phase, self.both, words)
        # (the optimizer's hyper-parameters are arguments of the captured launches: changing them means capturing again)
        self._hyper = (optimizer.lr, optimizer.betas, optimizer.eps, optimizer.max_norm)
        model.train()
        keep_check, optimizer.check = optimizer.check, False        # (no host read inside a capture)
        try:
            # the static buffers hold id 0 only: every row is a zero-length row, the gate closes and neither the warm-up run nor
            # anything else before the first real batch touches the weights
            side = torch.cuda.Stream(device=dev)
            side.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(side):
                for _ in range(2):                                   # allocator pools, kernel attributes, lazy handles
                    if self._run() is None:
                        raise ValueError("GraphedTrainStep: the model / optimizer pair does not take the direct step "
                                         "(trainer._direct_grad_views)")
                    if self._phase == "fold":
                        optimizer.gate.zero_()
            torch.cuda.current_stream(dev).wait_stream(side)
            torch.cuda.synchronize(dev)
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph):
                self.loss = self._run()
        finally:
            optimizer.check = keep_check
            optimizer._pending_status.clear()

    def _run(self):
        rows = {self.model.query_encoder: self.B, self.model.doc_encoder: 2 * self.B}
        with _towers_in_flight(self.model, self.optimizer, rows) as plan:
            return _train_step_direct(self.model, self.optimizer, (self.q, None, None), self._spec, plan, self._capture, self.labels,
                                      self.targets)

    def flush(self):
        """defer_check: settle the optimizer's pending check (raises that step's exception, if any)."""
        return self.optimizer.settle()

    def __call__(self, queries: torch.Tensor, pos_docs: torch.Tensor, neg_docs: torch.Tensor,
                 groups: Optional[torch.Tensor] = None, neg_groups: Optional[torch.Tensor] = None,
                 targets: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Returns the step's loss (a static 0-d device tensor, valid until the next call)."""
        if targets is not None and not self.soft:
            raise ValueError("GraphedTrainStep was captured without soft targets (soft=False), got targets")
        if (groups is not None or neg_groups is not None) and not self.grouped:
            raise ValueError("GraphedTrainStep was captured without labels (grouped=False), got groups / neg_groups")
        for src, width, what in ((queries, self.q_width, "queries"), (pos_docs, self.doc_width, "pos_docs"), (neg_docs, self.doc_width, "neg_docs")):
            if src.dim() != 2 or src.shape[0] != self.B or src.shape[1] > width or src.dtype != torch.int64:
                raise ValueError(f"GraphedTrainStep was captured for int64 {what} [{self.B}, <= {width}], got {src.dtype} {tuple(src.shape)}")
        if self.soft:   # (checked like train_step's, before anything is staged)
            targets = _batch_targets("GraphedTrainStep", self._spec, None, (queries, pos_docs, neg_docs), targets, groups, neg_groups)
        opt = self.optimizer
        if self._phase == "all" and (opt.lr, opt.betas, opt.eps, opt.max_norm) != self._hyper:
            raise ValueError("GraphedTrainStep: the optimizer's lr / betas / eps / max_norm changed since the capture (they are "
                             "arguments of the captured launches); build a new GraphedTrainStep")
        _stage_ids(self.q, queries, None)
        _stage_ids(self.both, pos_docs, neg_docs)
        if self.grouped:
            # (checked like train_step's: the eager redo takes the same labels)
            labels = _batch_labels("GraphedTrainStep", self._spec, (queries, pos_docs, neg_docs), groups, neg_groups)
            if labels is None:
                self.labels.fill_(-1)
            else:
                self.labels.copy_(labels)
        else:
            labels = None
        if self.soft:
            # (none: the one-hot, the plain step's bits; the eager redo takes the same targets)
            targets = self._one_hot if targets is None else targets
            self.targets.copy_(targets)
        if self._seeds is not None:
            drawn = _draw_dropout_seeds(self.model)
            self._seeds.put(drawn[id(self.model.query_encoder)], drawn[id(self.model.doc_encoder)])
        self.graph.replay()
        if self._phase == "fold":
            opt._reduce_apply(True, check=False)
        opt.mark_params_changed()
        if not opt.check:
            return self.loss
        # (the eager redo takes the one-workgroup retry itself if it must)
        opt.snapshot_gate(redo=lambda: _eager_step(self.model, opt, (queries, pos_docs, neg_docs), self._spec, labels, targets))
        if not self.defer_check:
            redone = opt.settle()            # the step's one host synchronisation
            if redone is not None:
                return redone
        return self.loss
