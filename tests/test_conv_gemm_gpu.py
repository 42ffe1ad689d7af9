"""The convolution routes of gemm.hip through ops.conv2d_forward/backward —
implicit forward <8,2> / <8,4> / <4,2>, implicit dx (also accumulating),
the small-C kernels, the space-to-depth route, the 1x1 route and the
materialised-col fallback — against float64 F.conv2d and its gradients with
the bounds of _gemm_bounds.py: y, dx, dw and db bit-exact on the exact input
class, inside the derived bound on the rounded one.  Each case asserts the
route flags conv2d_forward left in ctx, so a shape cannot silently move to
another kernel.  Weights are fp32 tensors holding bf16 values: the repack
rounds nothing.

Direct _ext.gemm_conv_fwd calls run the implicit kernel on an input whose
surroundings, and whose channels outside the group window, are NaN."""

import pytest
import torch

import _gemm_bounds as GB
from _gemm_bounds import BF, NAN, PADEL

pytestmark = pytest.mark.gpu

from caffeonspark_amd import ops
from caffeonspark_amd.ops import gpu as G

CLASSES = ("exact", "rounded")
FLAGS = ("implicit", "implicit_sc", "s2d", "is_1x1", "wino")


def dev():
    return torch.device("cuda:0")


def _seed(table, name, cls):
    return 100 + 2 * list(table).index(name) + CLASSES.index(cls)


@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("name", list(GB.CONV_CASES))
def test_conv_route(name, cls):
    c = GB.CONV_CASES[name]
    inp = GB.conv_inputs(c, cls, _seed(GB.CONV_CASES, name, cls))
    orc, peak = GB.conv_oracle(c, inp)
    assert GB.conv_geometry_ok(c)
    if cls == "exact":
        assert peak <= 256, "exact-class precondition"
    geo = ((c["stride"],) * 2, (c["pad"],) * 2, (c["dil"],) * 2,
           c["groups"])
    x = inp["x"].to(BF).to(dev())
    w = inp["w"].to(dev())
    b = inp["b"].to(dev()) if inp["b"] is not None else None
    ctx = {}
    y = ops.conv2d_forward(x, w, b, *geo, ctx=ctx, relu=c["relu"])
    flags = {f: bool(ctx.get(f)) for f in FLAGS}
    assert flags == {f: f == c["route"] for f in FLAGS}, flags
    assert (ctx.get("col") is not None) == (c["route"] == "col")
    has_wrf = getattr(w, "_cos_wrF", None) is not None
    assert has_wrf == (c["dx"] == "implicit"), "dx route"

    dy = inp["dy"].to(BF).to(dev())
    dx_into = None
    if c["dx_acc"]:
        dx_into = inp["dx0"].to(BF).to(dev()).contiguous(
            memory_format=torch.channels_last)
    db0 = torch.zeros(c["k"], dtype=torch.float32, device=dev())
    dx, dw, db = ops.conv2d_backward(x, w, dy, *geo, ctx=ctx, db_out=db0,
                                     dx_into=dx_into)
    torch.cuda.synchronize()
    if c["dx_acc"]:
        assert dx.data_ptr() == dx_into.data_ptr(), \
            "the accumulating epilogue was not taken"
    GB.within({"y": y, "dx": dx, "dw": dw, "db": db}, orc, f"{name}/{cls}")


@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("name", list(GB.FWD_DIRECT_CASES))
def test_conv_fwd_poisoned_input(name, cls):
    c = GB.FWD_DIRECT_CASES[name]
    inp = GB.conv_inputs(c, cls, _seed(GB.FWD_DIRECT_CASES, name, cls))
    g, n, ch = c["groups"], c["n"], c["c"]
    cg, kg = ch // g, c["k"] // g
    p, q = GB.conv_dims(c)
    npq = n * p * q
    kcol = c["r"] * c["s"] * cg
    kpad = GB.kpad_dma(kcol)
    zpage = G._zpage(dev())
    ext = ops.native()
    for gi in range(g):
        # NHWC input: the group's channels, NaN in every other channel and
        # on both sides of the tensor
        xw = torch.full((n, c["h"], c["w"], ch), NAN)
        xw[..., gi * cg:(gi + 1) * cg] = \
            inp["x"][:, gi * cg:(gi + 1) * cg].permute(0, 2, 3, 1)
        flat = torch.full((PADEL + xw.numel() + PADEL,), NAN, dtype=BF)
        flat[PADEL:PADEL + xw.numel()] = xw.reshape(-1).to(BF)
        xd = flat.to(dev())[PADEL:]
        wg = inp["w"][gi * kg:(gi + 1) * kg]
        wrb = torch.zeros(-(-kg // 128) * 128, kpad, dtype=BF)
        wrb[:kg, :kcol] = wg.permute(0, 2, 3, 1).reshape(kg, kcol).to(BF)
        bg = inp["b"][gi * kg:(gi + 1) * kg].contiguous()
        cflat, _, ldc = GB.out_buf(npq, kg, BF, NAN)
        cd = cflat.to(dev())
        geom = [c["h"], c["w"], ch, p, q, c["stride"], c["stride"],
                c["pad"], c["pad"], c["dil"], c["s"], gi * cg, cg, kcol]
        ext.gemm_conv_fwd(xd, wrb.to(dev()), cd[PADEL:], bg.to(dev()), zpage,
                          npq, kg, kpad, kpad, ldc, c["relu"], False, geom)
        torch.cuda.synchronize()
        assert GB.outside_untouched(cd, npq, kg, ldc), \
            "wrote outside the output view"
        got = cd.cpu()[PADEL:PADEL + npq * ldc].view(npq, ldc)[:, :kg]
        sub = dict(c, c=cg, k=kg, groups=1)
        sub_inp = dict(inp, x=inp["x"][:, gi * cg:(gi + 1) * cg], w=wg,
                       b=bg, dy=inp["dy"][:, gi * kg:(gi + 1) * kg])
        orc, _ = GB.conv_oracle(sub, sub_inp)
        GB.within({"y": got.view(n, p, q, kg).permute(0, 3, 1, 2)},
                  {"y": orc["y"]}, f"{name}/{cls} group {gi}")


@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("name", list(GB.WINO_CASES))
def test_winograd(name, cls, monkeypatch):
    """COS_WINOGRAD=1 forward and data gradient (flip, C != K) against the
    float64 direct convolution; also the only run of gemm_bf16_batched with
    batch 16 and non-zero batch strides."""
    monkeypatch.setenv("COS_WINOGRAD", "1")
    c = GB.WINO_CASES[name]
    inp = GB.wino_inputs(c, cls, _seed(GB.WINO_CASES, name, cls))
    orc_y, peak_y = GB.wino_oracle(c, inp, False)
    orc_dx, peak_dx = GB.wino_oracle(c, inp, True)
    if cls == "exact":
        assert max(peak_y, peak_dx) <= 256, "exact-class precondition"
    geo = ((1, 1), (1, 1), (1, 1), 1)
    x = inp["x"].to(BF).to(dev())
    w = inp["w"].to(dev())
    b = inp["b"].to(dev()) if inp["b"] is not None else None
    ctx = {}
    y = ops.conv2d_forward(x, w, b, *geo, ctx=ctx, relu=c["relu"])
    assert ctx.get("wino") is True
    dy = inp["dy"].to(BF).to(dev())
    dx, _, _ = ops.conv2d_backward(x, w, dy, *geo, need_dw=False, bias=False,
                                   ctx=ctx)
    torch.cuda.synchronize()
    GB.within({"y": y, "dx": dx}, dict(orc_y, **orc_dx), f"{name}/{cls}")
