"""reference.lrn_forward takes keep_scale (the GPU route's saving) and keeps
returning its scale either way."""

import torch

import _bf16_bounds as B
from caffeonspark_amd import ops
from caffeonspark_amd.ops import reference


def test_reference_ignores_keep_scale():
    inp = B.lrn_inputs((8, 5, 1.0, 0.75, 1.0, 1.0), 790)
    x = inp["x"].float()
    y0, s0 = reference.lrn_forward(x, 5, 1.0, 0.75, 1.0)
    y1, s1 = ops.lrn_forward(x, 5, 1.0, 0.75, 1.0, keep_scale=False)
    assert torch.equal(y0, y1) and torch.equal(s0, s1)
    dx0 = reference.lrn_backward(x, y0, s0, inp["dy"].float(), 5, 1.0, 0.75)
    dx1 = ops.lrn_backward(x, y1, s1, inp["dy"].float(), 5, 1.0, 0.75)
    assert torch.equal(dx0, dx1)
