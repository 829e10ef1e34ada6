"""A poisoning allocator for tests.

libtt.so allocates nothing: every workspace, output, flag word, status word and seed list comes from the Python host, nearly
always from torch.empty.  In a test process that memory is either fresh (zero) or the block of the previous identical call, so a
kernel that reads a word before anyone wrote it goes unnoticed.  poisoned_empty(word) makes the contents arbitrary on purpose:

    with poisoned_empty(0x3F800000) as p:
        v, i = index.search(q, 10)
    assert p.tensors > 0

While the block runs, every torch.empty(...), torch.empty_like(...) and Tensor.new_empty(...) that returns a CUDA tensor is
filled, bytewise over its whole storage, with the 32-bit pattern `word` (in memory order, i.e. little-endian) before it is
returned; a byte count that is no multiple of 4 gets the pattern's leading bytes in its tail.  (The host takes its workspaces from
torch.empty and its gradient outputs -- the table gradient, whose zeroing launch is load-bearing, among them -- from
torch.empty_like.)  The fill is queued on the current stream, like any kernel that will use the buffer.  Nothing is filled while
the current stream is capturing a graph (a fill would become a node of it), and host tensors are left alone unless host=True,
which exists for the helper's own CPU test.  torch.zeros / torch.full and what ATen allocates inside an operator are not touched."""
from __future__ import annotations

import contextlib
from unittest import mock

import torch

# word          as int32  as fp32    what it catches
PATTERNS = (
    0x00000000,  # 0        0.0        control: what the suite sees on fresh memory
    0xFFFFFFFF,  # -1       NaN        indices, flags, anything compared as float
    0x00000001,  # 1        denormal   counters that start one late: a skipped pool block or tile, no fault
    0x3F800000,  # large    1.0        thresholds or maxima stuck above every cosine of a unit-norm corpus
    0x7F800000,  # large    +inf       thresholds that reject everything; +inf is also the exact kernel's give-up marker
)
CONTROL = PATTERNS[0]


def pattern_id(word: int) -> str:
    return f"{word:08X}"


class PoisonCount:
    """What one poisoned_empty block filled."""

    def __init__(self):
        self.tensors = 0
        self.bytes = 0

    def __repr__(self):
        return f"PoisonCount(tensors={self.tensors}, bytes={self.bytes})"


def fill_bytes(t: torch.Tensor, word: int) -> int:
    """Fill the whole storage of `t` with the 32-bit pattern; returns the number of bytes written."""
    st = t.untyped_storage()
    n = st.nbytes()
    if n == 0:
        return 0
    raw = torch.tensor([], dtype=torch.uint8, device=t.device).set_(st, 0, (n,))
    whole = n & ~3
    if whole:
        raw[:whole].view(torch.int32).fill_(word - (1 << 32) if word & 0x80000000 else word)
    for j, b in enumerate(word.to_bytes(4, "little")[: n - whole]):
        raw[whole + j].fill_(b)
    return n


@contextlib.contextmanager
def poisoned_empty(word: int, *, host: bool = False):
    assert 0 <= word <= 0xFFFFFFFF, word
    count = PoisonCount()

    def poisoning(real):
        def allocate(*args, **kwargs):
            t = real(*args, **kwargs)
            if t.is_cuda:
                if torch.cuda.is_current_stream_capturing():
                    return t
            elif not (host and t.device.type == "cpu"):
                return t
            count.bytes += fill_bytes(t, word)
            count.tensors += 1
            return t
        return allocate

    with mock.patch.object(torch, "empty", poisoning(torch.empty)), \
            mock.patch.object(torch, "empty_like", poisoning(torch.empty_like)), \
            mock.patch.object(torch.Tensor, "new_empty", poisoning(torch.Tensor.new_empty)):
        yield count
