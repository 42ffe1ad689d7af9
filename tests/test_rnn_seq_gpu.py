"""The RNN recurrence kernels (csrc/rnn_seq.hip) and the layer on the GPU in
bf16, against the float64 loop and the derived bounds of _rnn_cases.py (its
docstring has the derivation).  Each case asserts the route that ran:
"resident" for the batch-tile-resident kernel pair, "loop" for the per-step
GEMM route (a shape outside the gate, or COS_RNN_SEQ=0)."""

import pytest
import torch

import _rnn_cases as C
from _bf16_bounds import E32, INTR, U, assert_within
from caffeonspark_amd import ops

gpu = pytest.mark.gpu


@gpu
@pytest.mark.parametrize("case", C.CASES, ids=C.case_id)
def test_recurrence_and_layer_within_derived_bounds(case, monkeypatch):
    monkeypatch.delenv("COS_RNN_SEQ", raising=False)
    if case[7] is not None:
        monkeypatch.setenv("COS_RNN_SEQ", case[7])
    d = torch.device("cuda:0")
    inp = C.inputs(case)
    xg = C.seq_xg(inp)
    bf = lambda t: None if t is None else t.to(d, torch.bfloat16)  # noqa
    fctx, bctx = {}, {}
    hs, cache = ops.rnn_seq_forward(bf(xg), bf(inp["W_hh"]),
                                    inp["cont"].to(d), bf(inp.get("h0")), fctx)
    dpre, dh0 = ops.rnn_seq_backward(bf(inp["do"]), bf(inp["W_hh"]), cache,
                                     bf(inp.get("dhT")), bctx)
    assert (fctx["route"], bctx["route"]) == (case[8], case[8])
    assert hs.dtype == dpre.dtype == torch.bfloat16
    out = {"hs": hs, "hc": cache[2], "dpre": dpre}
    if dh0 is not None:
        out["dh0"] = dh0
    out = {k: v.float().cpu() for k, v in out.items()}
    assert_within(out, C.seq_oracle(case, inp, xg), f"rnn {C.case_id(case)}")

    out, layer = C.run_layer(case, inp, d, torch.bfloat16)
    assert layer.seq_route == case[8]
    assert_within(out, C.layer_oracle(case, inp, out),
                  f"layer {C.case_id(case)}")


# rows, cols, column window of a wider buffer (None: contiguous): octets;
# cols % 8 != 0; strided rows on octets; strided and misaligned
TANH = [(5, 40, None), (7, 20, None), (6, 64, (8, 96)), (4, 20, (3, 40))]


@gpu
@pytest.mark.parametrize("rows,cols,win", TANH)
def test_tanh_kernels(rows, cols, win):
    """y = bf16(tanhf(z)): (U + INTR)|y|.  dz = bf16(dy (1 - y^2)): y^2 and
    1 - y^2 are exact in fp32 for a bf16 y, so one fp32 and one bf16
    rounding, (U + 4 E32)|dz|.  |z| reaches 4."""
    g = torch.Generator().manual_seed(rows * cols)
    d = torch.device("cuda:0")

    def operand(scale):
        full = (torch.randn(rows, win[1] if win else cols, generator=g)
                * scale).to(torch.bfloat16)
        lo = win[0] if win else 0
        return full, full.to(d)[:, lo:lo + cols], full[:, lo:lo + cols]
    _, z_d, z = operand(1.5)
    _, dy_d, dy = operand(1.0)
    y = ops.gpu_op("tanh_fwd")(z_d)
    dz = ops.gpu_op("tanh_bwd")(y, dy_d)
    y64 = torch.tanh(z.double())
    dz64 = dy.double() * (1 - y.cpu().double() ** 2)
    assert_within({"y": y.float().cpu(), "dz": dz.float().cpu()},
                  {"y": (y64, (U + INTR) * y64.abs()),
                   "dz": (dz64, (U + 4 * E32) * dz64.abs())},
                  f"tanh {rows}x{cols} {win}")
