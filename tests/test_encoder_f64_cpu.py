"""The fp32 C oracle (oracle/tt_oracle.c) against nn.GRU / nn.LSTM / nn.RNN in float64 (tests/f64_ref.py) at every shape of
tests/encoder_cases.py: the reference that the GPU tests trust, pinned to an independent higher-precision statement of the same
operation at exactly the shapes the kernels are then held to (tests/test_encoder_f64_gpu.py).  Tolerances are the project's
own (conftest.FWD_ATOL, conftest.GRAD_TOL with floor 1e-6): fp32 arithmetic uses about an eighth of them."""
import pytest
import torch

import synth
from conftest import FWD_ATOL, GRAD_TOL, assert_fwd_close, assert_grad_close
from encoder_cases import CASES, IDS, make_inputs
from f64_ref import encoder_f64

torch.set_num_threads(8)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_oracle_forward_and_backward_gradients_vs_float64(oracle, case):
    cid, cell, B, T, E, H, layers, bi, flags = case
    trainable = bool(flags.get("trainable"))
    ids, table, sd, d_out = make_inputs(case)
    want, wg, wt = encoder_f64(cell, ids, table, sd, E, H, layers, bi, d_out, table_grad=trainable)
    quads = synth.weight_quads(sd, layers, bi)
    pw, pb = sd.get("projection.weight"), sd.get("projection.bias")
    got = oracle.encoder_forward(ids, table, quads, H, layers, bi, pw, pb, True, rnn_type=cell)
    assert_fwd_close(got, want, atol=FWD_ATOL)
    res = oracle.encoder_backward(ids, table, quads, H, d_out, layers, bi, pw, pb, True, table_grad=trainable, rnn_type=cell)
    og, gpw, gpb = res[:3]
    names = [f"{n}_l{layer}" + ("_reverse" if d else "") for layer in range(layers) for d in range(2 if bi else 1)
             for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
    flat = [x for quad in og for x in quad]
    assert len(names) == len(flat) and set(names) | ({"projection.weight", "projection.bias"} if bi else set()) == set(wg)
    for name, g in zip(names, flat):
        assert_grad_close(g, wg[name], tol=GRAD_TOL, what=name, floor=1e-6)
    if bi:
        assert_grad_close(gpw, wg["projection.weight"], tol=GRAD_TOL, what="projection.weight", floor=1e-6)
        assert_grad_close(gpb, wg["projection.bias"], tol=GRAD_TOL, what="projection.bias", floor=1e-6)
    if trainable:
        assert_grad_close(res[3], wt, tol=GRAD_TOL, what="embedding.weight", floor=1e-6)
        assert not res[3][0].any() and not wt[0].any()
