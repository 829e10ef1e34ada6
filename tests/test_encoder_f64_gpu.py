"""The encoder kernels (K1 input projection, K2 recurrence, K7 backward, the weight-gradient and table-gradient kernels) against
nn.GRU / nn.LSTM / nn.RNN in float64 (tests/f64_ref.py), one case per dispatch class (tests/encoder_cases.py), through
RNNEncoder alone: no comparison build, no environment switches, no C-ABI calls.  Tolerances are conftest.FWD_ATOL on the
unit-norm outputs and conftest.GRAD_TOL of each gradient's largest element (floor 1e-6); the fp32 oracle measures about an
eighth of either against the same reference (tests/test_encoder_f64_cpu.py).  The reference of a case is computed once and
shared by its three checks."""
import functools

import numpy as np
import pytest
import torch

from conftest import FWD_ATOL, GRAD_TOL, assert_fwd_close, assert_grad_close
from encoder_cases import BY_ID, CASES, IDS, make_inputs
from f64_ref import encoder_f64

pytestmark = pytest.mark.gpu

# the one-workgroup recurrences are an option of the f16 recurrence alone (GRU, H = 256 here; arith="f32" runs neither form)
ONE_WG = [c[0] for c in CASES if c[1] == "GRU" and c[5] == 256 and c[8].get("arith") != "f32"]


@functools.lru_cache(maxsize=None)
def reference(cid):
    """(ids, table, sd, d_out, float64 output, float64 gradients by parameter name, float64 table gradient or None), read-only."""
    cid, cell, B, T, E, H, layers, bi, flags = case = BY_ID[cid]
    ids, table, sd, d_out = make_inputs(case)
    torch.set_num_threads(8)
    out, grads, gt = encoder_f64(cell, ids, table, sd, E, H, layers, bi, d_out, table_grad=bool(flags.get("trainable")))
    for a in [ids, table, d_out, out, *sd.values(), *grads.values()] + ([gt] if gt is not None else []):
        a.setflags(write=False)
    return ids, table, sd, d_out, out, grads, gt


def build(cid, train, one_workgroup=False):
    from twotowermlretrieval_amd.model import RNNEncoder
    cid, cell, B, T, E, H, layers, bi, flags = BY_ID[cid]
    ids, table, sd = reference(cid)[:3]
    enc = RNNEncoder(table.shape[0], E, H, pretrained_embeddings=None if flags.get("trainable") else table.copy(), rnn_type=cell,
                     num_layers=layers, bidirectional=bi, arith=flags.get("arith", "split16"))
    full = {"embedding.weight": torch.from_numpy(table.copy())}
    full.update({k: torch.from_numpy(v.copy()) for k, v in sd.items()})
    enc.load_state_dict(full)  # strict: torch's own key names and shapes
    if one_workgroup:
        enc.one_workgroup = enc.one_workgroup_bwd = True
    return enc.cuda().train(train), torch.from_numpy(ids.copy()).cuda()


def train_step_vs_float64(cid, one_workgroup):
    ids_np, table, sd, d_out, want, wg, wt = reference(cid)
    enc, ids = build(cid, True, one_workgroup)
    trainable = bool(BY_ID[cid][8].get("trainable"))
    assert enc.embedding.weight.requires_grad == trainable
    y = enc(ids)
    assert_fwd_close(y.detach().cpu().numpy(), want, atol=FWD_ATOL)
    y.backward(torch.from_numpy(d_out.copy()).cuda())
    torch.cuda.synchronize()
    checked = set()
    for name, prm in enc.named_parameters():
        if not prm.requires_grad:
            assert name == "embedding.weight" and prm.grad is None
            continue
        got = prm.grad.cpu().numpy()
        if name == "embedding.weight":
            assert_grad_close(got, wt, tol=GRAD_TOL, what=name, floor=1e-6)
            assert not got[0].any()                                      # padding_idx: exactly zero
            continue
        key = name[len("rnn."):] if name.startswith("rnn.") else name
        assert_grad_close(got, wg[key], tol=GRAD_TOL, what=name, floor=1e-6)
        checked.add(key)
    assert checked == set(wg)


@pytest.mark.parametrize("cid", IDS)
def test_eval_forward_vs_float64(cid):
    want = reference(cid)[4]
    enc, ids = build(cid, False)
    with torch.no_grad():
        y = enc(ids)
    torch.cuda.synchronize()
    y = y.cpu().numpy()
    assert_fwd_close(y, want, atol=FWD_ATOL)
    np.testing.assert_allclose(np.linalg.norm(y.astype(np.float64), axis=1), 1.0, rtol=0, atol=1e-6)


@pytest.mark.parametrize("cid", IDS)
def test_train_forward_and_backward_gradients_vs_float64(cid):
    train_step_vs_float64(cid, False)


@pytest.mark.parametrize("cid", ONE_WG)
def test_one_workgroup_recurrences_forward_and_backward_gradients_vs_float64(cid):
    train_step_vs_float64(cid, True)
