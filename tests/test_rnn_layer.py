"""The RNN layer on the CPU (fp32) against the float64 per-step loop of
_rnn_cases.py: forward, finite-difference gradients of every blob and
bottom, blob order, and the CPU emulation of the bf16 kernels held to the
bounds the GPU tests use."""

import pytest
import torch

import _rnn_cases as C
from _bf16_bounds import assert_within

# plain, x_static, exposed nonzero h_0, cont zero in mid-sequence (tuples as
# C.CASES)
SMALL = [(3, 2, 4, 3, 0, False, False, None, "loop"),
         (3, 2, 4, 3, 2, False, False, None, "loop"),
         (3, 2, 4, 3, 0, True, False, None, "loop"),
         (4, 4, 4, 3, 0, False, True, None, "loop")]


def fd_grad(p, name, eps=1e-6):
    """Central differences of the float64 loop's loss in p[name]."""
    def loss():
        o, hs = C.forward64(p)[:2]
        return float(C.loss64(p, o, hs))
    flat = p[name].reshape(-1)
    g = torch.empty_like(flat)
    for i in range(flat.numel()):
        keep = float(flat[i])
        flat[i] = keep + eps
        up = loss()
        flat[i] = keep - eps
        g[i] = (up - loss()) / (2 * eps)
        flat[i] = keep
    return g.reshape(p[name].shape)


@pytest.mark.parametrize("case", SMALL, ids=C.case_id)
def test_forward_and_fd_gradients(case):
    inp = C.inputs(case)
    out, _ = C.run_layer(case, inp)
    p = {k: v.to(C.F64).clone() for k, v in inp.items()}
    o, hs = C.forward64(p)[:2]
    want = {"o": o, "hT": hs[-1]}
    names = dict(dx="x", dxs="xs", dh0="h0")
    for k in set(out) - {"o", "hT", "hs", "hc", "dz", "dpre"}:
        want[k] = fd_grad(p, names.get(k, k))
    # fp32 against float64: 1e-5 of the largest value (FD error ~ eps^2)
    orc = {k: (want[k], 1e-5 * max(1.0, float(want[k].abs().max())))
           for k in want if k in out}
    assert_within({k: out[k] for k in orc}, orc, f"rnn layer {C.case_id(case)}")


@pytest.mark.parametrize("case", C.CASES[:4], ids=C.case_id)
def test_bf16_emulation_within_gpu_bounds(case):
    """fp32 arithmetic with bf16 stores fits the recurrence's bounds, and
    the fp32 layer fits the layer's, at every GPU case."""
    inp = C.inputs(case)
    xg = C.seq_xg(inp)
    emu = C.emulate_seq(xg, inp["W_hh"], inp["cont"], inp.get("h0"),
                        inp["do"], inp.get("dhT"))
    assert_within({k: v for k, v in emu.items() if v is not None},
                  C.seq_oracle(case, inp, xg), f"emu {C.case_id(case)}")
    out, _ = C.run_layer(case, inp)
    assert_within(out, C.layer_oracle(case, inp, out),
                  f"cpu {C.case_id(case)}")
