"""tests/poison.py itself: a helper that silently did nothing would let every test of test_uninitialised_buffers_gpu.py pass.
Host tensors stand in for device ones through the helper's test-only host=True switch."""
import numpy as np
import pytest
import torch

import poison
from poison import PATTERNS, poisoned_empty

DTYPES = [torch.uint8, torch.int32, torch.int64, torch.float32, torch.float16, torch.bfloat16]
SIZES = [0, 1, 3, 4, 5, (), (3, 5), (2, 0, 3)]


def raw_bytes(t):
    st = t.untyped_storage()
    return torch.tensor([], dtype=torch.uint8).set_(st, 0, (st.nbytes(),)).numpy().copy()


def expected_bytes(word, n):
    return np.frombuffer((word.to_bytes(4, "little") * (n // 4 + 1))[:n], dtype=np.uint8)


def test_the_patterns_are_the_five_words_and_the_control_comes_first():
    assert PATTERNS == (0x00000000, 0xFFFFFFFF, 0x00000001, 0x3F800000, 0x7F800000)
    assert poison.CONTROL == 0
    as_f32 = np.array(PATTERNS, dtype=np.uint32).view(np.float32)
    assert as_f32[0] == 0.0 and np.isnan(as_f32[1]) and 0 < as_f32[2] < 1e-44 and as_f32[3] == 1.0 and as_f32[4] == np.inf
    assert list(np.array(PATTERNS, dtype=np.uint32).view(np.int32)[:3]) == [0, -1, 1]


@pytest.mark.parametrize("word", PATTERNS + (0x04030201,), ids=poison.pattern_id)
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[-1])
def test_every_dtype_and_size_is_filled_to_the_last_byte(word, dtype):
    for size in SIZES:
        with poisoned_empty(word, host=True) as p:
            t = torch.empty(size, dtype=dtype)
        shape = (size,) if isinstance(size, int) else size
        assert t.dtype == dtype and tuple(t.shape) == shape and t.device.type == "cpu"
        n = t.numel() * t.element_size()
        got = raw_bytes(t)
        assert got.size == n
        assert np.array_equal(got, expected_bytes(word, n)), (size, got[:8])
        assert (p.tensors, p.bytes) == (1, n)


def test_a_tail_that_is_no_whole_word_gets_the_patterns_leading_bytes():
    with poisoned_empty(0x04030201, host=True):
        t = torch.empty(7, dtype=torch.uint8)
        h = torch.empty(3, dtype=torch.float16)
    assert t.tolist() == [1, 2, 3, 4, 1, 2, 3]
    assert raw_bytes(h).tolist() == [1, 2, 3, 4, 1, 2]


def test_typed_values_read_back_as_the_table_says():
    with poisoned_empty(0xFFFFFFFF, host=True):
        assert torch.empty(5, dtype=torch.int32).tolist() == [-1] * 5
        assert torch.empty(3, dtype=torch.int64).tolist() == [-1] * 3
        assert torch.isnan(torch.empty(3)).all() and torch.isnan(torch.empty(())).item()
    with poisoned_empty(0x00000001, host=True):
        assert torch.empty(2, dtype=torch.int32).tolist() == [1, 1]
        assert torch.empty((), dtype=torch.int64).item() == (1 << 32) + 1
    with poisoned_empty(0x3F800000, host=True):
        assert torch.empty(4).tolist() == [1.0] * 4
    with poisoned_empty(0x7F800000, host=True):
        assert torch.isposinf(torch.empty(4)).all()
        assert torch.empty(2, dtype=torch.bfloat16).view(torch.int16).tolist() == [0, 0x7F80]  # (low half, high half: +inf in bf16)


def test_keyword_forms_of_torch_empty_pass_through():
    with poisoned_empty(0x3F800000, host=True) as p:
        a = torch.empty((2, 3), dtype=torch.float32, device="cpu")
        b = torch.empty(2, 3, device=torch.device("cpu"))
        c = torch.empty(size=(6,), dtype=torch.float32)
    assert a.shape == (2, 3) and b.shape == (2, 3) and c.shape == (6,)
    assert all((x == 1.0).all() for x in (a, b, c))
    assert (p.tensors, p.bytes) == (3, 72)


def test_empty_like_and_new_empty_are_poisoned_too():
    """The host's gradient outputs come from torch.empty_like (memory_format= included); Tensor.new_empty for completeness."""
    src = torch.zeros((3, 5), dtype=torch.float32)
    with poisoned_empty(0x04030201, host=True) as p:
        a = torch.empty_like(src)
        b = torch.empty_like(src.t(), memory_format=torch.contiguous_format)
        c = torch.empty_like(src.t())                              # preserve_format: the source's strides
        d = torch.empty_like(src, dtype=torch.float16)
        e = src.new_empty((7,), dtype=torch.uint8)
        f = src.new_empty(2, 2)
        assert (p.tensors, p.bytes) == (6, 60 + 60 + 60 + 30 + 7 + 16)
    assert a.shape == (3, 5) and b.shape == (5, 3) and b.is_contiguous() and c.stride() == src.t().stride() and not src.any()
    assert d.dtype == torch.float16 and e.tolist() == [1, 2, 3, 4, 1, 2, 3] and f.dtype == torch.float32
    for t in (a, b, c, d, e, f):
        n = t.untyped_storage().nbytes()
        assert np.array_equal(raw_bytes(t), expected_bytes(0x04030201, n)), t.shape
    with poisoned_empty(0xFFFFFFFF, host=True):
        assert torch.isnan(torch.empty_like(src)).all() and torch.isnan(torch.empty_like(torch.zeros(()))).item()
        assert torch.empty_like(torch.zeros(0)).numel() == 0


def test_host_tensors_are_left_alone_by_default():
    with poisoned_empty(0xFFFFFFFF) as p:
        t = torch.empty(1 << 16, dtype=torch.int32)
        torch.empty_like(t)
        t.new_empty(5)
    assert (p.tensors, p.bytes) == (0, 0)


def test_the_counters_count():
    with poisoned_empty(1, host=True) as p:
        assert (p.tensors, p.bytes) == (0, 0)
        torch.empty(5, dtype=torch.uint8)
        assert (p.tensors, p.bytes) == (1, 5)
        torch.empty(0)
        assert (p.tensors, p.bytes) == (2, 5)  # an empty tensor is a tensor, of no bytes
        torch.empty((3, 2), dtype=torch.int64)
        torch.zeros(100)  # not torch.empty
        assert (p.tensors, p.bytes) == (3, 53)
    torch.empty(5)
    assert (p.tensors, p.bytes) == (3, 53)
    assert "tensors=3" in repr(p)


def test_torch_empty_is_restored_on_exit_and_after_an_exception():
    def patched():
        return torch.empty, torch.empty_like, torch.Tensor.new_empty
    real = patched()
    with poisoned_empty(0xFFFFFFFF, host=True):
        assert all(now is not was for now, was in zip(patched(), real))
    assert patched() == real
    with pytest.raises(RuntimeError, match="boom"):
        with poisoned_empty(0xFFFFFFFF, host=True):
            assert all(now is not was for now, was in zip(patched(), real))
            raise RuntimeError("boom")
    assert patched() == real
    with pytest.raises(TypeError):  # an error of torch.empty's own leaves the patch intact until exit, and gone after
        with poisoned_empty(0xFFFFFFFF, host=True):
            torch.empty("not a size")
    assert patched() == real


def test_blocks_nest_and_unwind_in_order():
    real = torch.empty
    with poisoned_empty(0x3F800000, host=True) as outer:
        with poisoned_empty(0xFFFFFFFF, host=True) as inner:
            t = torch.empty(2, dtype=torch.int32)
        u = torch.empty(2)
    assert torch.empty is real
    assert t.tolist() == [-1, -1] and u.tolist() == [1.0, 1.0]  # the inner fill is the last one written
    assert inner.tensors == 1 and outer.tensors == 2


def test_a_word_out_of_range_is_refused():
    for bad in (-1, 1 << 32):
        with pytest.raises(AssertionError):
            with poisoned_empty(bad):
                pass
