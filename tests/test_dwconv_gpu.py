"""The direct depthwise kernels of dwconv.hip through ops.conv2d_forward /
conv2d_backward against float64 F.conv2d and its gradients, with the bounds
of _gemm_bounds.py: y, dx, dw and db bit-exact on the exact input class,
inside the derived bound on the rounded one.  The route does fp32 sums of
R*S (y, dx) or NPQ (dw) terms with one final rounding, which is what bf_form
and the dw bound are derived for (dx="implicit" selects bf_form with
K = R*S*Kg = R*S).  Each case asserts ctx["dwc"], so a shape cannot fall
back to the per-group GEMM loop unnoticed."""

import pytest
import torch

import _gemm_bounds as GB
from _gemm_bounds import BF, NAN, PADEL

pytestmark = pytest.mark.gpu

from caffeonspark_amd import ops
from caffeonspark_amd.ops import gpu as G

CLASSES = ("exact", "rounded")


def dwcase(n, c, h, w, r, s=None, **kw):
    return GB.ccase(n, c, h, w, c, r, s, groups=c, dx="implicit", **kw)


CASES = {
    "one_octet_7x6": dwcase(2, 8, 7, 6, 3, pad=1),
    "three_octets_relu": dwcase(2, 24, 9, 9, 3, pad=1, relu=True),
    "stride2_pad1": dwcase(2, 16, 13, 13, 3, stride=2, pad=1),
    "stride2_pad0_4x4": dwcase(1, 8, 10, 10, 4, stride=2),
    "dil2": dwcase(2, 8, 11, 11, 3, dil=2, pad=2),
    "5x5_tap_chunks": dwcase(2, 8, 9, 9, 5, pad=2),
    "3x5_nobias": dwcase(2, 8, 9, 9, 3, 5, pad=1, bias=False),
    "dx_acc": dwcase(2, 16, 8, 8, 3, pad=1, dx_acc=True),
    "npq2178": dwcase(2, 8, 33, 33, 3, pad=1),
}


def dev():
    return torch.device("cuda:0")


def _seed(name, cls):
    return 700 + 2 * list(CASES).index(name) + CLASSES.index(cls)


def _geo(c):
    return ((c["stride"],) * 2, (c["pad"],) * 2, (c["dil"],) * 2,
            c["groups"])


@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("name", list(CASES))
def test_dwconv_route(name, cls):
    c = CASES[name]
    assert GB.conv_geometry_ok(c)
    inp = GB.conv_inputs(c, cls, _seed(name, cls))
    p, q = GB.conv_dims(c)
    slabs = G._dwc_slabs(c["c"], c["n"] * p * q)
    orc, peak = GB.conv_oracle(c, inp, splits_dw=slabs)
    if cls == "exact":
        assert peak <= 256, "exact-class precondition"
    x = inp["x"].to(BF).to(dev())
    w = inp["w"].to(dev())
    b = inp["b"].to(dev()) if inp["b"] is not None else None
    ctx = {}
    y = ops.conv2d_forward(x, w, b, *_geo(c), ctx=ctx, relu=c["relu"])
    assert ctx.get("dwc") is True and ctx["col"] is None
    dy = inp["dy"].to(BF).to(dev())
    dx_into = None
    if c["dx_acc"]:
        dx_into = inp["dx0"].to(BF).to(dev()).contiguous(
            memory_format=torch.channels_last)
    db0 = torch.zeros(c["k"], dtype=torch.float32, device=dev())
    dx, dw, db = ops.conv2d_backward(x, w, dy, *_geo(c), ctx=ctx,
                                     bias=c["bias"], db_out=db0,
                                     dx_into=dx_into)
    torch.cuda.synchronize()
    if c["dx_acc"]:
        assert dx.data_ptr() == dx_into.data_ptr(), \
            "the accumulating epilogue was not taken"
    out = {"y": y, "dx": dx, "dw": dw}
    if c["bias"]:
        out["db"] = db
    GB.within(out, {k: orc[k] for k in out}, f"{name}/{cls}")


def test_dw_forced_slabs():
    """dwconv_dw with 3 slabs forced at NPQ = 2178 (726 rows each, no
    multiple of the 256 position lanes): the same bits as one slab."""
    c = CASES["npq2178"]
    inp = GB.conv_inputs(c, "exact", 790)
    orc, _ = GB.conv_oracle(c, inp, splits_dw=3)
    cl = dict(memory_format=torch.channels_last)
    x = inp["x"].to(BF).to(dev()).contiguous(**cl)
    dy = inp["dy"].to(BF).to(dev()).contiguous(**cl)
    p, q = GB.conv_dims(c)
    geom = [c["n"], c["h"], c["w"], c["c"], p, q, c["r"], c["s"], 1, 1,
            c["pad"], c["pad"], 1]
    ext = ops.native()
    got = {}
    for want in (1, 3):
        slabs = torch.full((want * 9 * c["c"],), NAN, device=dev())
        dw = torch.full((c["c"], 1, 3, 3), NAN, device=dev())
        assert ext.dwconv_dw(dy, c["c"], x, slabs, want, geom) == want
        ext.dwconv_dw_finalize(slabs, want, dw, c["c"], 9)
        got[want] = dw
    torch.cuda.synchronize()
    assert torch.equal(got[1], got[3])
    GB.within({"dw": got[3]}, {"dw": orc["dw"]}, "forced slabs")


@pytest.mark.parametrize("cls", CLASSES)
def test_dwconv_concat_window(cls):
    """Forward into channels 8..23 of a 40-channel concat buffer, backward
    from the same window of a 40-channel diff whose other channels are NaN."""
    c = dwcase(2, 16, 8, 8, 3, pad=1, relu=True)
    inp = GB.conv_inputs(c, cls, 795 + CLASSES.index(cls))
    orc, _ = GB.conv_oracle(c, inp)
    p, q = GB.conv_dims(c)
    n, ch, npq, off = c["n"], c["c"], c["n"] * p * q, 8

    def window(fill):
        flat, _, ld = GB.out_buf(npq, ch, BF, fill, ld_x=24)
        flat = flat.to(dev())
        buf = flat[PADEL - off:PADEL - off + npq * ld].view(n, p, q, ld) \
            .permute(0, 3, 1, 2)
        return flat, buf, ld

    yflat, ybuf, ld = window(NAN)
    x = inp["x"].to(BF).to(dev())
    w, b = inp["w"].to(dev()), inp["b"].to(dev())
    ctx = {}
    y = ops.conv2d_forward(x, w, b, *_geo(c), ctx=ctx, relu=True,
                           out_into=(ybuf, off))
    assert ctx.get("dwc") is True
    _, dybuf, _ = window(inp["dy"].permute(0, 2, 3, 1).reshape(npq, ch))
    dybuf[:, :off] = NAN
    dybuf[:, off + ch:] = NAN
    db0 = torch.zeros(ch, dtype=torch.float32, device=dev())
    dx, dw, db = ops.conv2d_backward(x, w, dybuf[:, off:off + ch], *_geo(c),
                                     ctx=ctx, db_out=db0)
    torch.cuda.synchronize()
    assert GB.outside_untouched(yflat, npq, ch, ld), \
        "wrote outside the concat window"
    GB.within({"y": y, "dx": dx, "dw": dw, "db": db}, orc, f"window/{cls}")


def test_gate_keeps_c12():
    """C % 8 != 0 stays on the per-group route."""
    c = dwcase(2, 12, 8, 8, 3, pad=1)
    inp = GB.conv_inputs(c, "rounded", 799)
    ctx = {}
    ops.conv2d_forward(inp["x"].to(BF).to(dev()), inp["w"].to(dev()), None,
                       *_geo(c), ctx=ctx)
    torch.cuda.synchronize()
    assert not ctx.get("dwc") and ctx["col"] is not None
