"""Soft targets without a GPU: the float64 helper (tests/soft_loss_ref.py) is pool_loss_ref's on one-hot targets and its closed
form G is autograd's; the target builders against their statements; the new entries are declared, bound and exported; the size
query and every refusal happen before any launch; the trainers refuse targets where they mean nothing."""
import ctypes
import inspect
import re

import numpy as np
import pytest
import torch

import synth
from conftest import ROOT
from grouped_loss_ref import ignored
from pool_loss_ref import pool_loss
from soft_loss_ref import bounds, closed_form_G, scores, soft_loss
from test_abi_cpu import libtt  # noqa: F401  (the fixture builds the library when it is missing)
from test_pool_loss_cpu import BASE, CASES
from twotowermlretrieval_amd._lib import TT_ERR_BAD_SHAPE as BAD_SHAPE

ENTRY, SIZE = "tt_contrastive_loss_soft_f32", "tt_contrastive_loss_soft_workspace_bytes"


def rows(seed, n, H, scale=1.0):
    return (synth.unit_rows(seed, n, H) * np.float32(scale)).astype(np.float32)


def one_hot(B, M, pos):
    t = np.zeros((B, M), dtype=np.float32)
    t[np.arange(B), pos + np.arange(B)] = 1.0
    return t


def dense(seed, B, M):
    z = 3.0 * np.random.RandomState(seed).standard_normal((B, M))
    e = np.exp(z - z.max(axis=1, keepdims=True))
    return (e / e.sum(axis=1, keepdims=True)).astype(np.float32)


def test_on_one_hot_targets_the_helper_is_the_pool_helper():
    q, d = rows(41, 7, 20, 3.0), rows(42, 19, 20, 3.0)
    q[2] = 0.0
    for pos in (0, 5, 12):
        want, got = pool_loss(q, d, pos, 0.05), soft_loss(q, d, one_hot(7, 19, pos), 0.05)
        assert abs(got[0] - want[0]) <= 1e-14 * abs(want[0])
        for g, w in zip(got[1:], want[1:]):
            assert np.abs(g - w).max() <= 1e-13 * np.abs(w).max()


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_closed_form_gradient_is_autograds(dtype):
    """dq = sum_j G_ij d s_ij / d q_i: checked through unit rows scaled by 1, where d s / d qh = Dh / temperature and the
    projection through the norm is the helper's own (autograd of s alone)."""
    B, M, temp = 5, 13, 0.1
    q, d = rows(43, B, 16), rows(44, M, 16, 4.0)
    t = dense(7, B, M)
    t[1] = 0.0
    t[3, 4] = -0.25
    G = torch.from_numpy(closed_form_G(q, d, t, temp, dtype))
    x = [torch.from_numpy(a).to(dtype).requires_grad_(True) for a in (q, d)]
    from in_batch_ref import normalised
    s = (normalised(x[0]) @ normalised(x[1]).T) / temp
    s.backward(G)
    got = soft_loss(q, d, t, temp, dtype)
    eps = 1e-12 if dtype == torch.float64 else 2e-5
    for a, b in zip((x[0].grad.numpy(), x[1].grad.numpy()), got[1:]):
        assert np.abs(a - b).max() <= eps * max(np.abs(b).max(), 1e-30)
    assert not got[1][1].any() and not closed_form_G(q, d, t, temp, dtype)[1].any()     # (an all-zero target row: nothing)


def test_all_zero_rows_cost_nothing_and_the_bound_is_zero_for_all_zero_targets():
    q, d = rows(45, 4, 24), rows(46, 9, 24)
    want, tol = bounds(q, d, np.zeros((4, 9), dtype=np.float32), 0.05)
    assert want[0] == 0.0 and not want[1].any() and not want[2].any() and tol == [0.0, 0.0, 0.0]
    t = dense(8, 4, 9)
    t[[0, 3]] = 0.0
    loss, dq, dd = soft_loss(q, d, t, 0.05)
    alone = [soft_loss(q[i:i + 1], d, t[i:i + 1], 0.05)[0] for i in (1, 2)]
    assert abs(loss - sum(alone) / 4) <= 1e-14 * abs(loss) and not dq[0].any() and not dq[3].any() and dq[1].any()


def test_a_probability_row_costs_kl_plus_entropy():
    q, d = rows(47, 3, 16), rows(48, 11, 16)
    t = dense(9, 3, 11).astype(np.float64)
    t /= t.sum(axis=1, keepdims=True)
    s = scores(q, d, 0.05)
    logp = (s - torch.logsumexp(s, dim=1, keepdim=True)).numpy()
    kl = (t * (np.log(t) - logp)).sum(axis=1)
    ent = -(t * np.log(t)).sum(axis=1)
    assert abs(soft_loss(q, d, t, 0.05)[0] - (kl + ent).mean()) < 1e-12


def test_multi_positive_targets_are_the_ignored_pairs_plus_the_own_positive():
    import twotowermlretrieval_amd as tt
    qg = np.array([5, -1, 5, 7, 9], dtype=np.int64)
    dg = np.array([9, 5, -1, 5, 7, 5, -1, 7, 9, -1], dtype=np.int64)
    for pos in (0, 1, 5):
        member = ignored(qg, dg, pos)
        member[np.arange(5), pos + np.arange(5)] = True
        want = member.astype(np.float32) / member.sum(axis=1, keepdims=True).astype(np.float32)
        got = tt.multi_positive_targets(torch.from_numpy(qg), torch.from_numpy(dg), pos)
        assert got.dtype == torch.float32 and np.array_equal(got.numpy(), want)
        assert np.allclose(got.sum(dim=1).numpy(), 1.0, atol=1e-6) and got.numpy()[1].tolist() == one_hot(5, 10, pos)[1].tolist()
    for bad in (dict(q_groups=torch.from_numpy(qg).int()), dict(doc_groups=torch.from_numpy(dg).float()), dict(pos_offset=6),
                dict(pos_offset=-1), dict(q_groups=[5, -1, 5, 7, 9])):
        kw = dict(dict(q_groups=torch.from_numpy(qg), doc_groups=torch.from_numpy(dg), pos_offset=0), **bad)
        with pytest.raises(ValueError, match="multi_positive_targets"):
            tt.multi_positive_targets(**kw)


def test_distillation_targets_are_the_teachers_softmax_over_the_valid_pairs():
    import twotowermlretrieval_amd as tt
    z = torch.from_numpy(np.random.RandomState(3).standard_normal((4, 9)).astype(np.float32)) * 5.0
    assert torch.equal(tt.distillation_targets(z), torch.softmax(z, dim=1))
    assert torch.equal(tt.distillation_targets(z.double(), 2.0), torch.softmax(z / 2.0, dim=1))
    valid = torch.ones((4, 9), dtype=torch.bool)
    valid[0, [1, 4]] = False
    valid[2] = False                       # (no valid pair: an all-zero row)
    valid[3, 1:] = False                   # (one valid pair: weight 1)
    t = tt.distillation_targets(z, 0.5, valid)
    assert t.dtype == torch.float32 and torch.isfinite(t).all() and not t[~valid].any() and not t[2].any()
    keep = valid[0]
    assert torch.allclose(t[0][keep], torch.softmax(z[0][keep] / 0.5, dim=0), rtol=1e-6, atol=0.0)
    assert torch.equal(t[1], torch.softmax(z[1] / 0.5, dim=0)) and t[3, 0] == 1.0
    assert torch.allclose(t.sum(dim=1), torch.tensor([1.0, 1.0, 0.0, 1.0]), atol=1e-6)
    for bad in (dict(valid=valid.float()), dict(valid=valid[:3]), dict(teacher_temperature=0.0), dict(teacher_temperature=float("nan")),
                dict(teacher_scores=z[0]), dict(teacher_scores=z.long())):
        with pytest.raises(ValueError, match="distillation_targets"):
            tt.distillation_targets(**dict(dict(teacher_scores=z), **bad))


def test_entries_are_declared_bound_and_exported(libtt):  # noqa: F811
    from twotowermlretrieval_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "tt.h").read_text(), flags=re.S)
    for name in (ENTRY, SIZE):
        assert re.search(r"\b%s\s*\(" % name, header)
        assert name in _lib.SIGNATURES and hasattr(libtt, name)
    res, args = _lib.SIGNATURES[ENTRY]
    old = _lib.SIGNATURES["tt_contrastive_loss_f32"]
    assert res is old[0] and args == old[1][:5] + [ctypes.c_void_p] + old[1][6:]      # (targets in the place of pos_offset)
    assert _lib.SIGNATURES[SIZE] == _lib.SIGNATURES["tt_contrastive_loss_workspace_bytes"]
    import twotowermlretrieval_amd as tt
    for fn in (tt.train_step, tt.DataParallelTrainer.step, tt.GraphedTrainStep.__call__):
        assert inspect.signature(fn).parameters["targets"].default is None, fn
    assert inspect.signature(tt.GraphedTrainStep.__init__).parameters["soft"].default is False
    assert list(inspect.signature(tt.soft_contrastive_loss).parameters) == ["q", "docs", "targets", "temperature"]
    assert "H(t_i)" in tt.soft_contrastive_loss.__doc__ and "subtract" in tt.soft_contrastive_loss.__doc__
    for name in ("soft_contrastive_loss", "distillation_targets", "multi_positive_targets"):
        assert name in tt.__all__ and callable(getattr(tt, name))


def ib_slices(walked_rows, owner_rows):
    """(chunks per slice, slices): the rule of csrc/in_batch_loss.hip, restated (as in tests/test_pool_loss_gpu.py)."""
    chunks, tiles = -(-walked_rows // 128), -(-owner_rows // 32)
    want = min(max(256 // tiles, 1), 8, chunks)
    per = -(-chunks // want)
    return per, -(-chunks // per)


# tt_contrastive_loss_workspace_bytes(B, M, H) as the library returned it before the soft entry existed
PLAIN_BYTES = {(1, 1, 1): 70144, (4, 12, 256): 528896, (33, 33, 96): 201216, (17, 130, 256): 924160, (1025, 2060, 32):
               2242048, (512, 1024, 256): 10012672, (512, 8192, 256): 21604352, (65600, 65600, 32): 35983872, (16777216,
               33554432, 512): 206896627712}


def test_size_query_needs_no_gpu_and_leaves_the_plain_queries_alone(libtt):  # noqa: F811
    soft, plain = libtt.tt_contrastive_loss_soft_workspace_bytes, libtt.tt_contrastive_loss_workspace_bytes
    for B, M, H in ((0, 4, 256), (-1, 4, 256), (5, 4, 256), ((1 << 24) + 1, 1 << 25, 32), (4, (1 << 25) + 1, 32), (4, 12, 0),
                    (4, 12, 513)):
        assert soft(B, M, H) == 0, (B, M, H)
    up = lambda n: -(-n // 256) * 256  # noqa: E731
    for (B, M, H), recorded in PLAIN_BYTES.items():
        base = plain(B, M, H)
        assert base == recorded, (B, M, H)
        n, Bq = ib_slices(M, B)[1], -(-B // 128) * 128
        # the plain plan, then per (slice, query) the sums of t and of t s, then w [Bq]: each piece rounded up to 256 bytes
        assert soft(B, M, H) == base + 2 * up(4 * n * Bq) + up(4 * Bq), (B, M, H)
    assert libtt.tt_in_batch_loss_workspace_bytes(512, 256) == PLAIN_BYTES[(512, 1024, 256)]


def _p(addr):
    return ctypes.c_void_p(addr) if addr else None


SOFT_BASE = dict({k: v for k, v in BASE.items() if k != "pos_offset"}, targets=8192)
SOFT_CASES = dict({k: ({a: b for a, b in over.items() if a != "pos_offset"}, msg) for k, (over, msg) in CASES.items()
                   if not k.startswith("pos_offset")}, **{"null targets": (dict(targets=0), "null pointer")})


@pytest.mark.parametrize("over,msg", list(SOFT_CASES.values()), ids=list(SOFT_CASES))
def test_bad_arguments_are_refused_before_any_launch(libtt, over, msg):  # noqa: F811
    """The pointers are never dereferenced: a call that got past its refusals would launch on a machine without a GPU and
    return another status than TT_ERR_BAD_SHAPE."""
    a = dict(SOFT_BASE, **over)
    need = libtt.tt_contrastive_loss_soft_workspace_bytes(BASE["B"], BASE["M"], BASE["H"])
    assert need > 0
    nbytes = a["ws_bytes"] if "ws_bytes" in a else need - a["ws_short"]
    rc = libtt.tt_contrastive_loss_soft_f32(_p(a["q"]), a["B"], _p(a["docs"]), a["M"], a["H"], _p(a["targets"]), a["temperature"],
                                            _p(a["loss"]), _p(a["dq"]), _p(a["ddocs"]), _p(a["ws"]), nbytes, None)
    assert rc == BAD_SHAPE
    err = libtt.tt_last_error().decode()
    assert err.startswith(ENTRY + ": ") and msg in err, err


def test_the_plain_workspace_is_too_small_for_the_soft_entry(libtt):  # noqa: F811
    a = SOFT_BASE
    plain = libtt.tt_contrastive_loss_workspace_bytes(a["B"], a["M"], a["H"])
    rc = libtt.tt_contrastive_loss_soft_f32(_p(a["q"]), a["B"], _p(a["docs"]), a["M"], a["H"], _p(a["targets"]), a["temperature"],
                                            _p(a["loss"]), _p(a["dq"]), _p(a["ddocs"]), _p(a["ws"]), plain, None)
    assert rc == BAD_SHAPE and "workspace" in libtt.tt_last_error().decode()


def test_targets_are_refused_where_they_mean_nothing_without_a_gpu():
    import twotowermlretrieval_amd as tt
    ids = torch.zeros((2, 3), dtype=torch.int64)
    g, t = torch.zeros(2, dtype=torch.int64), torch.zeros((2, 4))
    for step in (lambda **kw: tt.train_step(None, None, ids, ids, ids, **kw),):
        with pytest.raises(ValueError, match='targets need negatives="in_batch"'):
            step(targets=t)                                                                  # (the default: "paired")
        with pytest.raises(ValueError, match='targets need negatives="in_batch"'):
            step(targets=t, negatives="paired")
        for kw in (dict(groups=g), dict(groups=g, neg_groups=g), dict(neg_groups=g)):
            with pytest.raises(ValueError, match="targets and groups / neg_groups exclude each other"):
                step(targets=t, negatives="in_batch", **kw)
        for bad in (t.double(), t.long(), t[:1], t[:, :3], t[None], torch.zeros((2, 8)), [[0.0] * 4] * 2):
            with pytest.raises(ValueError, match=r"targets must be a float32 tensor \[2, 4\]"):
                step(targets=bad, negatives="in_batch")
        with pytest.raises(ValueError, match="as many negatives"):
            tt.train_step(None, None, ids, ids, ids[:1], negatives="in_batch", targets=t)
    with pytest.raises(ValueError, match="soft=True needs"):
        tt.GraphedTrainStep(None, None, batch=2, q_width=16, doc_width=16, soft=True)         # (the default: "paired")
    with pytest.raises(ValueError, match="exclude each other"):
        tt.GraphedTrainStep(None, None, batch=2, q_width=16, doc_width=16, negatives="in_batch", soft=True, grouped=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):                               # (targets do not open a CPU path)
        tt.soft_contrastive_loss(torch.zeros(2, 4), torch.zeros(5, 4), torch.zeros(2, 5))
