"""The one-pass LRN backward (lrn_bwd_fused_kernel) and the forward without
a stored scale, on the GPU: y and dx inside the float64 bounds of
_bf16_bounds.lrn_oracle, bit-equal to the two-pass route (COS_LRN_FUSED=0),
the grid-stride loop on forced 1, 2 and 3-block grids, the pack contract of
ops.lrn_forward / ops.lrn_backward, and an LRNLayer that keeps no fp32
tensor of its input's size."""

import pytest
import torch

import _bf16_bounds as B

pytestmark = pytest.mark.gpu

from caffeonspark_amd import ops
from caffeonspark_amd.core.blob import Blob
from caffeonspark_amd.core.layers.base import create_layer
from caffeonspark_amd.ops import gpu as G
from caffeonspark_amd.proto import caffe_pb, text_format


def dev():
    return torch.device("cuda:0")


def d(t):
    return t.to(dev())


# (C, local_size, alpha, beta, k, input scale): every window shape of the
# 24-channel register file, each beta mode (0.75 / 0.5 / generic) at more
# than one of them and both at local_size 5 (radius fixed at compile time)
# and at another size (radius read at run time), alpha large enough that
# dx's second term matters
ADDED_CASES = [
    (8, 1, 1.0, 0.75, 1.0, 1.0),      # radius 0
    (8, 3, 2.0, 0.6, 1.0, 1.0),
    (8, 9, 0.5, 0.5, 2.0, 1.0),       # radius 4, both neighbours absent
    (16, 5, 2.0, 0.6, 1.0, 1.0),      # generic beta at the fixed radius 2
    (16, 9, 1.0, 0.75, 1.0, 1.0),     # every window crosses an edge
    (24, 9, 2.0, 0.6, 1.0, 1.0),      # one interior octet at full radius
    (96, 5, 1.0, 0.5, 1.0, 1.0),      # AlexNet norm1's width
    (192, 5, 1e-4, 0.75, 1.0, 60.0),  # GoogLeNet conv2/norm2's width
]
CASES = list(enumerate(B.LRN_CASES + ADDED_CASES))
case_ids = ["C%d-n%d-a%g-b%g" % c[1][:4] for c in CASES]

_runs = {}


def both_routes(case, monkeypatch):
    """Inputs, oracle and the outputs of the fused and the two-pass route
    for one case, computed once."""
    i, params = case
    if i not in _runs:
        inp = B.lrn_inputs(params, 700 + i)
        args = (inp["local_size"], inp["alpha"], inp["beta"])
        x, dy = d(inp["x"]), d(inp["dy"])
        monkeypatch.setenv("COS_LRN_FUSED", "1")
        y_f, pack_f = ops.lrn_forward(x, *args, inp["k"], keep_scale=False)
        dx_f = ops.lrn_backward(x, y_f, pack_f, dy, *args)
        monkeypatch.setenv("COS_LRN_FUSED", "0")
        y_t, pack_t = ops.lrn_forward(x, *args, inp["k"])
        dx_t = ops.lrn_backward(x, y_t, pack_t, dy, *args)
        _runs[i] = dict(inp=inp, orc=B.lrn_oracle(inp), y_f=y_f, dx_f=dx_f,
                        pack_f=pack_f, y_t=y_t, dx_t=dx_t, pack_t=pack_t)
    return _runs[i]


@pytest.mark.parametrize("case", CASES, ids=case_ids)
def test_fused_within_bounds(case, monkeypatch):
    r = both_routes(case, monkeypatch)
    assert r["pack_f"][0] is None
    B.assert_within({"y": r["y_f"], "dx": r["dx_f"]}, r["orc"],
                    f"lrn fused {case[1]}")


@pytest.mark.parametrize("case", CASES, ids=case_ids)
def test_fused_bit_equal_to_two_pass(case, monkeypatch):
    r = both_routes(case, monkeypatch)
    assert r["pack_t"][0] is not None
    assert torch.equal(r["y_f"], r["y_t"])
    nd = int((r["dx_f"] != r["dx_t"]).sum())
    print(f"lrn {case[1]}: {nd}/{r['dx_f'].numel()} dx elements differ")
    assert torch.equal(r["dx_f"], r["dx_t"])


# ----------------------------------------------------------- grid-stride loop

def _pixels_case(n, c, h, w, seed):
    g = B.gen(seed)
    inp = dict(x=B.bf16(torch.randn(n, c, h, w, generator=g)),
               dy=B.bf16(torch.randn(n, c, h, w, generator=g)),
               local_size=5, alpha=1.0, beta=0.75, k=1.0)
    cl = torch.channels_last
    return inp, d(inp["x"]).contiguous(memory_format=cl), \
        d(inp["dy"]).contiguous(memory_format=cl)


# 3x16x5x7 is 210 octets: one partial sweep of a 256-thread block.
# 3x16x13x17 is 1326 octets: 6, 3 and 2 sweeps on 1, 2 and 3 blocks, the
# last one partial on each.
@pytest.mark.parametrize("blocks", [1, 2, 3])
@pytest.mark.parametrize("hw", [(5, 7), (13, 17)], ids=lambda s: "%dx%d" % s)
def test_fused_forced_blocks(hw, blocks):
    n, c = 3, 16
    inp, xl, dyl = _pixels_case(n, c, *hw, 760)
    npix = n * hw[0] * hw[1]
    dx0, dxb = torch.empty_like(xl), torch.empty_like(xl)
    G._ext.lrn_bwd_fused(xl, dyl, dx0, npix, c, 5, 1.0, 0.75, 1.0)
    G._ext.lrn_bwd_fused(xl, dyl, dxb, npix, c, 5, 1.0, 0.75, 1.0,
                         max_blocks=blocks)
    assert torch.equal(dxb, dx0)
    orc = B.lrn_oracle(inp)
    B.assert_within({"dx": dxb}, orc, f"lrn fused {hw} blocks={blocks}")


# ------------------------------------------------------------------- contract

def test_pack_contract(monkeypatch):
    inp = B.lrn_inputs((16, 5, 1.0, 0.75, 1.0, 1.0), 770)
    orc = B.lrn_oracle(inp)
    x, dy = d(inp["x"]), d(inp["dy"])
    monkeypatch.setenv("COS_LRN_FUSED", "1")
    y, pack = ops.lrn_forward(x, 5, 1.0, 0.75, 1.0, keep_scale=False)
    assert pack[0] is None
    dx = ops.lrn_backward(x, y, pack, dy, 5, 1.0, 0.75)
    B.assert_within({"y": y, "dx": dx}, orc, "fused, no scale")
    y, pack = ops.lrn_forward(x, 5, 1.0, 0.75, 1.0)
    assert pack[0].dtype == torch.float32
    dx = ops.lrn_backward(x, y, pack, dy, 5, 1.0, 0.75)
    B.assert_within({"y": y, "dx": dx,
                     "scale": pack[0].permute(0, 3, 1, 2)}, orc,
                    "fused, scale kept")
    monkeypatch.setenv("COS_LRN_FUSED", "0")
    y, pack = ops.lrn_forward(x, 5, 1.0, 0.75, 1.0, keep_scale=False)
    assert pack[0].dtype == torch.float32
    dx = ops.lrn_backward(x, y, pack, dy, 5, 1.0, 0.75)
    B.assert_within({"y": y, "dx": dx,
                     "scale": pack[0].permute(0, 3, 1, 2)}, orc,
                    "two-pass, keep_scale=False")


@pytest.mark.parametrize("fused", ["1", "0"])
def test_fallback_contract(fused, monkeypatch):
    """C % 8 != 0 runs the torch fallback, which keeps its scale."""
    monkeypatch.setenv("COS_LRN_FUSED", fused)
    inp = B.lrn_inputs((12, 5, 1.0, 0.75, 1.0, 1.0), 771)
    orc = B.lrn_oracle(inp)
    x = d(inp["x"])
    y, pack = ops.lrn_forward(x, 5, 1.0, 0.75, 1.0, keep_scale=False)
    assert isinstance(pack, torch.Tensor) and pack.dtype == torch.float32
    dx = ops.lrn_backward(x, y, pack, d(inp["dy"]), 5, 1.0, 0.75)
    # the fallback rounds once, to bf16, from fp32 arithmetic
    B.assert_within({"y": y, "dx": dx}, orc, "lrn fallback C12")


def test_binding_refuses_aliased_dx():
    _, xl, dyl = _pixels_case(2, 16, 3, 3, 772)
    args = (2 * 3 * 3, 16, 5, 1.0, 0.75, 1.0)
    with pytest.raises(RuntimeError, match="alias"):
        G._ext.lrn_bwd_fused(xl, dyl, xl, *args)
    with pytest.raises(RuntimeError, match="alias"):
        G._ext.lrn_bwd_fused(xl, dyl, dyl, *args)
    with pytest.raises(RuntimeError, match="C % 8"):
        G._ext.lrn_bwd_fused(xl, dyl, torch.empty_like(xl), 24, 12, 5, 1.0,
                             0.75, 1.0)


# ---------------------------------------------------------------------- layer

class _Net:
    phase = caffe_pb.Phase.TRAIN
    dtype = torch.bfloat16
    generator = torch.Generator().manual_seed(1)

    def __init__(self):
        self.device = dev()


def test_layer_keeps_no_fp32_scale(monkeypatch):
    monkeypatch.setenv("COS_LRN_FUSED", "1")
    inp = B.lrn_inputs((16, 5, 1.0, 0.75, 2.0, 1.0), 780)
    x, dy = d(inp["x"]), d(inp["dy"])
    lp = text_format.parse(
        """name: "n" type: "LRN" bottom: "x" top: "y"
        lrn_param { local_size: 5 alpha: 1.0 beta: 0.75 k: 2.0 }""",
        caffe_pb.LayerParameter)
    layer = create_layer(lp, _Net())
    bottom, top = Blob(x.shape), Blob([0])
    bottom.data = x
    layer.setup([bottom], [top])
    layer.forward([bottom], [top])
    top.diff = dy
    layer.backward([top], [True], [bottom])
    y, pack = ops.lrn_forward(x, 5, 1.0, 0.75, 2.0, keep_scale=False)
    dx = ops.lrn_backward(x, y, pack, dy, 5, 1.0, 0.75)
    assert torch.equal(top.data, y)
    assert torch.equal(bottom.diff, dx)
    held = [t for t in vars(layer).values() if isinstance(t, torch.Tensor)]
    for v in vars(layer).values():
        if isinstance(v, (tuple, list)):
            held += [t for t in v if isinstance(t, torch.Tensor)]
    assert not [t for t in held
                if t.dtype == torch.float32 and t.numel() >= x.numel()]
