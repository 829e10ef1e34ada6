"""CPU-side checks of cursor search (tt_score_topk_after_*, score_topk_after, the indexes' search_after / pages / deep_search,
mine_hard_negatives): the numpy reference against a literal walk, the paging identity on the reference, the clamp of the
cursor's id, the mining ceiling, the declarations, the size query and argument validation.  No GPU."""
import ctypes
import re

import numpy as np
import pytest
import torch

import cursor_ref
from conftest import ROOT

NAMES = ("tt_score_topk_after_workspace_bytes", "tt_score_topk_after_f32", "tt_score_topk_after_bf16", "tt_after_local_bound")
I64_MAX, I64_MIN = cursor_ref.I64_MAX, cursor_ref.I64_MIN


@pytest.fixture(scope="module")
def libtt():
    from twotowermlretrieval_amd import build, _lib
    build.build()
    return _lib.lib()


def corpus(kind, N, d=32, seed=0):
    """Rows for the reference's own tests: random, with duplicate rows (runs of ties), or all equal."""
    rs = np.random.RandomState(seed + N)
    D = (rs.standard_normal((N, d)) / np.sqrt(d)).astype(np.float32)
    if kind == "dups":
        D[rs.randint(0, N, size=max(1, N // 2))] = D[0]
        D[rs.randint(0, N, size=max(1, N // 4))] = D[N - 1]
    elif kind == "equal":
        D[:] = D[0]
    Q = (rs.standard_normal((3, d)) / np.sqrt(d)).astype(np.float32)
    Q[0] = D[0]
    return Q, D


@pytest.mark.parametrize("kind", ["random", "dups", "equal"])
@pytest.mark.parametrize("N", [1, 31, 1000])
def test_reference_equals_the_literal_walk(oracle, kind, N):
    Q, D = corpus(kind, N)
    S = oracle.score_all(Q, D)
    rs = np.random.RandomState(N)
    off = 2 ** 33 + 5
    for b in range(Q.shape[0]):
        order = np.argsort(-S[b], kind="stable")
        cursors = [(np.float32(np.inf), -1), (NEG := np.float32(-np.inf), -1), (np.float32(np.nan), 0), (S[b, order[0]], I64_MIN),
                   (S[b, order[0]], I64_MAX), (S[b, order[-1]], off + int(order[-1])), (np.float32(0.0), off + N // 2)]
        cursors += [(S[b, n], off + int(n)) for n in rs.randint(0, N, size=6)]
        cursors += [(S[b, n], off + int(n) - 1) for n in rs.randint(0, N, size=3)]
        for a, i in cursors:
            for k in (1, 7, 64):
                gv, gi = cursor_ref.search_after(S[b:b + 1], [a], [i], k, off)
                wv, wi = cursor_ref.walk(S[b], a, i, k, off)
                assert np.array_equal(gi[0], wi) and np.array_equal(gv[0], wv), (kind, N, b, a, i, k)
        assert (cursor_ref.search_after(S[b:b + 1], [NEG], [-1], 5, off)[1] == -1).all()
        assert (cursor_ref.search_after(S[b:b + 1], [np.nan], [-1], 5, off)[1] == -1).all()


@pytest.mark.parametrize("kind", ["random", "dups", "equal"])
@pytest.mark.parametrize("N", [1, 31, 1000])
@pytest.mark.parametrize("k", [1, 7, 64])
def test_pages_concatenated_are_the_stable_sort(oracle, kind, N, k):
    Q, D = corpus(kind, N, seed=1)
    S = oracle.score_all(Q, D)
    for b in range(Q.shape[0]):
        vals, ids = cursor_ref.pages_until_tail(S[b], k, idx_offset=7)
        order = np.argsort(-S[b], kind="stable")
        real = ids >= 0
        assert ids[real].tolist() == (order + 7).tolist()                       # every document once, in the total order
        assert np.array_equal(vals[real], S[b, order])
        assert not real[len(order):].any() and np.isneginf(vals[~real]).all()   # then nothing but the tail
        assert len(ids) == k * (N // k + 1)                                     # the page that ends in the tail is the last


def test_clamp_of_the_cursor_id(libtt):
    """after_idx - idx_offset as if in exact integers, then clamped to [-1, N]: the int64 extremes on both sides."""
    N = 1000
    offs = (0, 5, -5, 2 ** 33 + 5, I64_MAX, I64_MIN, I64_MAX - N, I64_MIN + 1)
    ids = (0, -1, 1, N - 1, N, N + 1, 2 ** 33 + 5, 2 ** 33 + 4, 2 ** 33 + 5 + N, 2 ** 31, 2 ** 32, -(2 ** 32), I64_MAX, I64_MIN,
           I64_MAX - 1, I64_MIN + 1)
    for off in offs:
        for i in ids:
            want = cursor_ref.local_bound(i, off, N)
            assert -1 <= want <= N
            assert libtt.tt_after_local_bound(i, off, N) == want, (i, off)
    assert cursor_ref.local_bound(I64_MAX, -5, N) == N and cursor_ref.local_bound(I64_MIN, 5, N) == -1   # would wrap in int64
    assert libtt.tt_after_local_bound(I64_MAX, I64_MIN, N) == N and libtt.tt_after_local_bound(I64_MIN, I64_MAX, N) == -1
    assert libtt.tt_after_local_bound(7, 7, 0) == 0 and libtt.tt_after_local_bound(6, 7, 0) == -1
    # the rule on ids and the rule on clamped positions agree: g > i  <=>  n > clamp(i - off, -1, N) for 0 <= n < N
    n = np.arange(N)
    for off in (0, 2 ** 33 + 5, I64_MAX - N):
        for i in ids:
            by_id = np.array([int(x) + off > i for x in n])
            assert np.array_equal(by_id, n > cursor_ref.local_bound(i, off, N)), (i, off)


def test_eligibility_at_the_id_extremes_and_special_scores():
    S = np.array([[0.5, 0.25, 0.25, -0.0, 0.0, 0.25]], dtype=np.float32)
    off = 2 ** 33 + 5
    e = lambda a, i: cursor_ref.eligibility(S, [a], [i], off)[0].tolist()
    assert e(0.25, I64_MAX) == [False, False, False, True, True, False]         # ties excluded
    assert e(0.25, I64_MIN) == [False, True, True, True, True, True]            # ties included
    assert e(0.25, off + 2) == [False, False, False, True, True, True]          # the tie behind the cursor's id only
    assert e(0.25, 2) == [False, True, True, True, True, True]                  # an id below the shard: before every row
    assert e(0.0, off + 3) == [False, False, False, False, True, False]         # -0.0 == +0.0: one run of ties
    assert e(np.nan, -1) == [False] * 6 and e(-np.inf, -1) == [False] * 6
    assert e(np.inf, -1) == [True] * 6


def test_mining_ceiling_against_numpy():
    """negatives_ceiling and the rule around it, the score and search steps stood in by numpy."""
    from twotowermlretrieval_amd.mining import negatives_ceiling
    rs = np.random.RandomState(4)
    B, N, P, k = 9, 300, 3, 10
    S = rs.standard_normal((B, N)).astype(np.float32)
    pos = rs.randint(0, N, size=(B, P)).astype(np.int64)
    pos[1, 2] = -1                                                              # padding
    pos[2] = -1                                                                 # no positive at all
    pos[3, 0] = N + 5                                                           # not in the index: no score
    pos[4] = np.argsort(-S[4])[[0, 40, 41]]                                     # a positive far below the best one
    ok = (pos >= 0) & (pos < N)
    ps = np.where(ok, np.take_along_axis(S, np.clip(pos, 0, N - 1), 1), -np.inf).astype(np.float32)
    for margin, ratio in ((0.0, None), (0.25, None), (0.0, 0.95)):
        got = negatives_ceiling(torch.from_numpy(ps), torch.from_numpy(pos), margin, ratio).numpy()
        want = cursor_ref.ceiling(ps, pos, margin, ratio)
        assert got.dtype == np.float32 and np.array_equal(got, want)
        assert np.isposinf(got[2]) and np.isfinite(np.delete(got, 2)).all()
        assert got[1] == (min(ps[1, 0], ps[1, 1]) * np.float32(ratio) if ratio else min(ps[1, 0], ps[1, 1]) - np.float32(margin))
        (v, i), c = cursor_ref.mine(S, pos, k, margin, ratio)
        assert np.array_equal(c, want)
        for b in range(B):
            real = i[b] >= 0
            assert not np.isin(i[b][real], pos[b]).any() and (v[b][real] <= c[b]).all()
            # the cursor (ceiling, -1) plus the exclusion list says the same
            cv, ci = cursor_ref.search_after(S[b:b + 1], [c[b]], [-1], k + P)
            keep = ~np.isin(ci[0], pos[b][pos[b] >= 0]) & (ci[0] >= 0)
            assert ci[0][keep][:k].tolist() == i[b][real].tolist()
        plain = np.argsort(-S[2], kind="stable")[:k]
        assert i[2].tolist() == plain.tolist()                                  # no positive: the plain top-k
        assert S[4, pos[4, 0]] > c[4] and pos[4, 0] not in i[4]                 # the best positive lies above the ceiling
    with pytest.raises(ValueError, match="one of them"):
        negatives_ceiling(torch.from_numpy(ps), torch.from_numpy(pos), 0.1, 0.9)
    with pytest.raises(ValueError, match="positive"):
        negatives_ceiling(torch.from_numpy(ps), torch.from_numpy(pos), 0.0, 0.0)


def test_header_declares_the_calls_and_the_table_binds_them(libtt):
    from twotowermlretrieval_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "tt.h").read_text(), flags=re.S)
    for name in NAMES:
        assert re.search(rf"\b{name}\s*\(", header), name
        assert name in _lib.SIGNATURES and hasattr(libtt, name), name
    _vp, _i, _i64, _sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_size_t
    assert _lib.SIGNATURES[NAMES[0]] == (_sz, [_i, _i64, _i, _i, _i])
    call = (_i, [_vp, _i, _i, _vp, _i64, _vp, _vp, _vp, _i, _i64, _vp, _vp, _vp, _sz, _vp])
    assert _lib.SIGNATURES[NAMES[1]] == call and _lib.SIGNATURES[NAMES[2]] == call
    assert _lib.SIGNATURES[NAMES[3]] == (_i, [_i64, _i64, _i])


@pytest.mark.parametrize("B,N,d,k,bf16", [(32, 1_000_000, 256, 10, 0), (5, 300_001, 512, 64, 0), (130, 70_000, 128, 1, 1),
                                          (1024, 10_000_000, 256, 10, 1), (3, 0, 64, 7, 0)])
def test_size_query(libtt, B, N, d, k, bf16):
    n = libtt.tt_score_topk_after_workspace_bytes(B, N, d, k, bf16)
    assert n > 0 and n == libtt.tt_score_topk_masked_workspace_bytes(B, N, d, k, bf16)
    assert libtt.tt_score_topk_after_workspace_bytes(0, N, d, k, bf16) == 0
    assert libtt.tt_score_topk_after_workspace_bytes(B, N, d, 65, bf16) == 0


def test_argument_validation_without_gpu(libtt):
    from twotowermlretrieval_amd import _lib
    p = ctypes.c_void_p(16)
    t = ctypes.c_void_p(256)
    f32, bf16 = libtt.tt_score_topk_after_f32, libtt.tt_score_topk_after_bf16
    rc = f32(None, 4, 256, None, 10, t, t, None, 65, 0, p, p, None, 0, None)
    assert rc == _lib.TT_ERR_UNSUPPORTED and b"k=65" in libtt.tt_last_error()
    rc = bf16(None, 4, 256, None, 10, None, None, None, 65, 0, p, p, None, 0, None)        # also as the masked call
    assert rc == _lib.TT_ERR_UNSUPPORTED and b"k=65" in libtt.tt_last_error()
    for av, ai in ((t, None), (None, t)):                                                  # one cursor pointer NULL
        for fn in (f32, bf16):
            rc = fn(None, 4, 256, None, 10, av, ai, None, 5, 0, p, p, None, 0, None)
            assert rc == _lib.TT_ERR_BAD_SHAPE and b"both" in libtt.tt_last_error()
    for addr in (257, 258, 259):                                                           # after_val: 4-byte aligned
        rc = f32(None, 4, 256, None, 10, ctypes.c_void_p(addr), t, None, 5, 0, p, p, None, 0, None)
        assert rc == _lib.TT_ERR_BAD_SHAPE and b"aligned" in libtt.tt_last_error()
    for addr in (257, 258, 260, 262):                                                      # after_idx: 8-byte, not 4
        rc = f32(None, 4, 256, None, 10, t, ctypes.c_void_p(addr), None, 5, 0, p, p, None, 0, None)
        assert rc == _lib.TT_ERR_BAD_SHAPE and b"aligned" in libtt.tt_last_error()
    rc = f32(None, 4, 100, None, 10, t, t, None, 5, 0, p, p, None, 0, None)
    assert rc == _lib.TT_ERR_UNSUPPORTED and b"d=100" in libtt.tt_last_error()
    rc = bf16(None, 4, 96, None, 10, t, t, None, 5, 0, p, p, None, 0, None)                # the exact search's widths per dtype
    assert rc == _lib.TT_ERR_UNSUPPORTED and b"d=96" in libtt.tt_last_error()
    rc = f32(None, 4, 256, None, 10, t, t, ctypes.c_void_p(18), 5, 0, p, p, None, 0, None)
    assert rc == _lib.TT_ERR_BAD_SHAPE and b"keep" in libtt.tt_last_error()
    rc = f32(None, 4, 256, None, -1, t, t, None, 5, 0, p, p, None, 0, None)
    assert rc == _lib.TT_ERR_BAD_SHAPE and b"N=-1" in libtt.tt_last_error()


def test_python_shims_refuse_cpu_tensors_and_wrong_arguments():
    import twotowermlretrieval_amd as tt
    from twotowermlretrieval_amd import index, mining
    assert tt.score_topk_after is index.score_topk_after and tt.mine_hard_negatives is mining.mine_hard_negatives
    assert "score_topk_after" in tt.__all__ and "score_topk_after" in index.__all__ and "mine_hard_negatives" in tt.__all__
    q, D = torch.zeros(2, 256), torch.zeros(100, 256)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tt.score_topk_after(q, D, float("inf"), -1, 5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tt.score_topk_after(q[0], D, 0.5, 7, 5)
    cpu = torch.device("cpu")
    av, ai = index._cursor(None, 3, cpu)                                        # the open cursor
    assert av.dtype == torch.float32 and ai.dtype == torch.int64 and av.tolist() == [float("inf")] * 3 and ai.tolist() == [-1] * 3
    av, ai = index._cursor((0.5, I64_MIN), 2, cpu)
    assert av.tolist() == [0.5, 0.5] and ai.tolist() == [I64_MIN] * 2
    assert index._cursor((0.5, I64_MAX), 1, cpu)[1].tolist() == [I64_MAX]
    tv, ti = torch.tensor([1.0, 2.0]), torch.tensor([3, 4])
    av, ai = index._cursor((tv, ti), 2, cpu)
    assert av.data_ptr() == tv.data_ptr() and ai.data_ptr() == ti.data_ptr()   # read in place: a captured call follows them
    assert index._cursor((torch.tensor(1.0), torch.tensor(3)), 1, cpu)[0].shape == (1,)   # a single query's 0-d cursor
    for bad in ((tv.double(), ti), (tv, ti.int()), ("x", 3), (1.0, 2.5), (1.0, True)):
        with pytest.raises(TypeError):
            index._cursor(bad, 2, cpu)
    for bad in ((tv, ti[:1]), (tv[:1], ti), (tv.reshape(2, 1).expand(2, 2), ti), (1.0, 2 ** 63)):
        with pytest.raises(ValueError):
            index._cursor(bad, 2, cpu)
    with pytest.raises(ValueError, match="live on|runs on"):
        index._cursor((tv, ti), 2, torch.device("cuda", 0))
    for cls in (tt.BruteForceIndex, tt.ShardedIndex, tt.StreamedIndex):
        for name in ("search_after", "pages", "deep_search"):
            assert callable(getattr(cls, name)), (cls, name)
    with pytest.raises(ValueError, match="pos_ids"):
        tt.mine_hard_negatives(None, q, torch.zeros((3, 2), dtype=torch.int64), 5)
    with pytest.raises(ValueError, match="one of them"):
        tt.mine_hard_negatives(None, q, torch.zeros((2, 2), dtype=torch.int64), 5, margin=0.1, ratio=0.9)
