"""gemm_conv_fwd's N tiles (48, 64, 96 and 128 columns) and its grouped
launch, against float64 F.conv2d with the bounds of _gemm_bounds.py.

Every tile width keeps the k order of an output element (one 16x16x32 MFMA
per K tile, ascending), so a result must not only lie inside the bound but
equal the 128-wide tile's bit for bit; COS_CONV_BN forces a width and is
read on every call.  The grouped launch must equal the per-group calls of
the 13-argument binding bit for bit."""

import pytest
import torch

import _gemm_bounds as GB
from _gemm_bounds import BF, NAN, PADEL

pytestmark = pytest.mark.gpu

from caffeonspark_amd import ops
from caffeonspark_amd.ops import gpu as G

CLASSES = ("exact", "rounded")
WIDTHS = (None, "48", "64", "96", "128")      # None: automatic selection


def dev():
    return torch.device("cuda:0")


def _seed(table, name, cls):
    return 700 + 2 * list(table).index(name) + CLASSES.index(cls)


def _force(monkeypatch, bn):
    if bn is None:
        monkeypatch.delenv("COS_CONV_BN", raising=False)
    else:
        monkeypatch.setenv("COS_CONV_BN", bn)


# Kg of 16 .. 264 is, per width, exact (48, 96, 192), ragged in the last
# tile (40, 56, 104, 200, 264) or narrower than the tile (16).  8x8 images
# give NPQ = 128, one M tile; 9x9 give 162, a ragged second one.  C = 8 is
# Kpad 96 (three K tiles, depth 2), C = 16 Kpad 160 (depth 4).  Thinned
# inputs keep the exact class inside bf16's integers.
TILE_CASES = {
    "k16": GB.ccase(2, 8, 8, 8, 16, 3, pad=1),
    "k40": GB.ccase(2, 16, 9, 9, 40, 3, pad=1),
    "k48": GB.ccase(2, 8, 9, 9, 48, 3, pad=1, relu=True),
    "k56": GB.ccase(2, 16, 8, 8, 56, 3, pad=1),
    "k96": GB.ccase(2, 8, 9, 9, 96, 3, pad=1),
    "k104": GB.ccase(2, 16, 8, 8, 104, 3, pad=1, density=0.5),
    "k192": GB.ccase(2, 8, 8, 8, 192, 3, pad=1, density=0.25),
    "k200": GB.ccase(2, 16, 9, 9, 200, 3, pad=1, relu=True, density=0.25),
    "k264": GB.ccase(2, 8, 9, 9, 264, 3, pad=1, density=0.25),
    # Kpad 64: the two-tile minimum of the counted wait
    "k40_kpad64": GB.ccase(2, 8, 8, 9, 40, 2, 3),
    # Kpad 288: inside the depth-4 range; 1248: above it
    "k56_kpad288": GB.ccase(2, 32, 9, 9, 56, 3, pad=1, density=0.5),
    "k104_kpad1248": GB.ccase(1, 136, 7, 7, 104, 3, pad=1, density=0.25),
    # NPQ 288 and Kg 264: the 4-wave kernels
    "k264_npq288": GB.ccase(2, 8, 12, 12, 264, 3, pad=1, density=0.25),
    # NPQ 8320 >= 8192: the 256-row blocks of the 48- and 64-wide tiles,
    # 32 whole M tiles and half of one
    "k40_npq8320": GB.ccase(2, 8, 65, 64, 40, 3, pad=1),
    "k56_npq8320": GB.ccase(2, 8, 65, 64, 56, 3, pad=1, relu=True),
}


@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("name", list(TILE_CASES))
def test_tile_widths(name, cls, monkeypatch):
    c = TILE_CASES[name]
    inp = GB.conv_inputs(c, cls, _seed(TILE_CASES, name, cls))
    orc, peak = GB.conv_oracle(c, inp)
    assert GB.conv_geometry_ok(c)
    if cls == "exact":
        assert peak <= 256, "exact-class precondition"
    geo = ((1, 1), (c["pad"],) * 2, (1, 1), 1)
    x = inp["x"].to(BF).to(dev())
    dy = inp["dy"].to(BF).to(dev())
    got = {}
    for bn in WIDTHS:
        _force(monkeypatch, bn)
        w = inp["w"].to(dev())
        ctx = {}
        y = ops.conv2d_forward(x, w, inp["b"].to(dev()), *geo, ctx=ctx,
                               relu=c["relu"])
        assert ctx.get("implicit") is True
        assert getattr(w, "_cos_wrF", None) is not None, "dx route"
        dx, _, _ = ops.conv2d_backward(x, w, dy, *geo, need_dw=False,
                                       bias=False, ctx=ctx)
        torch.cuda.synchronize()
        GB.within({"y": y, "dx": dx}, {"y": orc["y"], "dx": orc["dx"]},
                  f"{name}/{cls} BN={bn}")
        got[bn] = (y.clone(), dx.clone())
    for bn in WIDTHS:
        assert torch.equal(got[bn][0], got["128"][0]), f"y, BN={bn}"
        assert torch.equal(got[bn][1], got["128"][1]), f"dx, BN={bn}"


# ---- grouped launch, direct calls.  The input carries GAP channels after
# every group's window, NaN like both sides of the buffer, so a window that
# is off by anything reads them; the output view is narrower than its row
# stride and surrounded by sentinels.
GAP = 8
GROUP_CASES = {
    "g2_kg24": GB.ccase(2, 32, 8, 8, 48, 3, pad=1, groups=2),
    "g4_kg24": GB.ccase(2, 32, 9, 9, 96, 3, pad=1, groups=4, relu=True),
    # Kg 56: ragged for every width, the next group's rows share the tile
    "g2_kg56": GB.ccase(2, 16, 9, 9, 112, 3, pad=1, groups=2),
}


@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("name", list(GROUP_CASES))
def test_grouped_launch(name, cls, monkeypatch):
    c = GROUP_CASES[name]
    inp = GB.conv_inputs(c, cls, _seed(GROUP_CASES, name, cls))
    orc, peak = GB.conv_oracle(c, inp)
    if cls == "exact":
        assert peak <= 256, "exact-class precondition"
    g, n, ch, k = c["groups"], c["n"], c["c"], c["k"]
    cg, kg = ch // g, k // g
    p, q = GB.conv_dims(c)
    npq = n * p * q
    kcol = c["r"] * c["s"] * cg
    kpad = GB.kpad_dma(kcol)
    ext = ops.native()
    zpage = G._zpage(dev())

    cs = cg + GAP                               # channel stride of a group
    xw = torch.full((n, c["h"], c["w"], g * cs), NAN)
    for gi in range(g):
        xw[..., gi * cs:gi * cs + cg] = \
            inp["x"][:, gi * cg:(gi + 1) * cg].permute(0, 2, 3, 1)
    flat = torch.full((PADEL + xw.numel() + PADEL,), NAN, dtype=BF)
    flat[PADEL:PADEL + xw.numel()] = xw.reshape(-1).to(BF)
    xd = flat.to(dev())[PADEL:]
    # group rows at stride Kg, as the layer keeps them; zero pad rows
    wrb = torch.zeros((g - 1) * kg + -(-kg // 128) * 128, kpad, dtype=BF)
    wrb[:k, :kcol] = inp["w"].permute(0, 2, 3, 1).reshape(k, kcol).to(BF)
    wrb, bias = wrb.to(dev()), inp["b"].to(dev())
    geom = [c["h"], c["w"], g * cs, p, q, 1, 1, c["pad"], c["pad"], 1,
            c["s"], 0, cg, kcol]

    def fresh():
        cflat, _, ldc = GB.out_buf(npq, k, BF, NAN)
        assert ldc > k
        return cflat.to(dev()), ldc

    for bn in WIDTHS:
        _force(monkeypatch, bn)
        one, ldc = fresh()
        ext.gemm_conv_fwd(xd, wrb, one[PADEL:], bias, zpage, npq, kg, kpad,
                          kpad, ldc, c["relu"], False, geom, g, cs, kg, kg)
        per, _ = fresh()
        for gi in range(g):
            gg = list(geom)
            gg[11] = gi * cs
            ext.gemm_conv_fwd(xd, wrb[gi * kg:], per[PADEL + gi * kg:],
                              bias[gi * kg:(gi + 1) * kg], zpage, npq, kg,
                              kpad, kpad, ldc, c["relu"], False, gg)
        torch.cuda.synchronize()
        assert GB.outside_untouched(one, npq, k, ldc), \
            f"BN={bn}: wrote outside the output view"
        got = one.cpu()[PADEL:PADEL + npq * ldc].view(npq, ldc)[:, :k]
        GB.within({"y": got.view(n, p, q, k).permute(0, 3, 1, 2)},
                  {"y": orc["y"]}, f"{name}/{cls} BN={bn}")
        assert torch.equal(one, per), f"BN={bn}: grouped != per-group"


# ---- every instantiation, selected by the plan or not, through the cfg
# argument: NPQ 338 is ragged for 128- and 256-row blocks, Kg 104 for every
# width, Kpad 160 is five K tiles
@pytest.mark.parametrize("cls", CLASSES)
def test_every_configuration(cls):
    c = GB.ccase(2, 16, 13, 13, 104, 3, pad=1, density=0.5)
    inp = GB.conv_inputs(c, cls, 790 + CLASSES.index(cls))
    orc, peak = GB.conv_oracle(c, inp)
    if cls == "exact":
        assert peak <= 256, "exact-class precondition"
    n, ch, k = c["n"], c["c"], c["k"]
    p, q = GB.conv_dims(c)
    npq, kcol = n * p * q, 9 * ch
    kpad = GB.kpad_dma(kcol)
    ext = ops.native()
    xd = inp["x"].permute(0, 2, 3, 1).contiguous().to(BF).to(dev())
    wrb = torch.zeros(128, kpad, dtype=BF)
    wrb[:k, :kcol] = inp["w"].permute(0, 2, 3, 1).reshape(k, kcol).to(BF)
    wrb, bias = wrb.to(dev()), inp["b"].to(dev())
    geom = [c["h"], c["w"], ch, p, q, 1, 1, 1, 1, 1, 3, 0, ch, kcol]
    table = ext.conv_fwd_cfgs()
    assert {t[1] for t in table} == {48, 64, 96, 128}
    ref = None
    for cfg in range(len(table)):
        # element-wise epilogue on an odd row stride, 16-byte epilogue on
        # an aligned one
        for vec, ld_x in ((0, 3), (1, 8)):
            cflat, _, ldc = GB.out_buf(npq, k, BF, NAN, ld_x=ld_x)
            assert (ldc % 8 == 0) == bool(vec)
            cd = cflat.to(dev())
            ext.gemm_conv_fwd(xd, wrb, cd[PADEL:], bias, G._zpage(dev()),
                              npq, k, kpad, kpad, ldc, False, False, geom, 1,
                              0, 0, 0, cfg, vec)
            torch.cuda.synchronize()
            what = f"cfg {cfg} {table[cfg]} vec {vec}"
            assert GB.outside_untouched(cd, npq, k, ldc), what
            got = cd.cpu()[PADEL:PADEL + npq * ldc].view(npq, ldc)[:, :k]
            if ref is None:
                ref = got.clone()
                GB.within({"y": got.view(n, p, q, k).permute(0, 3, 1, 2)},
                          {"y": orc["y"]}, f"cfg 0/{cls}")
            assert torch.equal(ref, got), what


# ---- grouped accumulating dx through conv2d_backward: Cg = 24 is the dx
# GEMM's N, ragged for the 48-wide tile it selects
ACC_CASE = GB.ccase(2, 48, 8, 8, 32, 3, pad=1, groups=2, dx_acc=True)


@pytest.mark.parametrize("cls", CLASSES)
def test_grouped_dx_accumulates(cls, monkeypatch):
    c = ACC_CASE
    inp = GB.conv_inputs(c, cls, 760 + CLASSES.index(cls))
    orc, peak = GB.conv_oracle(c, inp)
    if cls == "exact":
        assert peak <= 256, "exact-class precondition"
    geo = ((1, 1), (1, 1), (1, 1), c["groups"])
    x = inp["x"].to(BF).to(dev())
    dy = inp["dy"].to(BF).to(dev())
    got = {}
    for bn in (None, "128"):
        _force(monkeypatch, bn)
        w = inp["w"].to(dev())
        ctx = {}
        ops.conv2d_forward(x, w, inp["b"].to(dev()), *geo, ctx=ctx)
        assert getattr(w, "_cos_wrF", None) is not None, "dx route"
        dx_into = inp["dx0"].to(BF).to(dev()).contiguous(
            memory_format=torch.channels_last)
        dx, _, _ = ops.conv2d_backward(x, w, dy, *geo, need_dw=False,
                                       bias=False, ctx=ctx, dx_into=dx_into)
        torch.cuda.synchronize()
        assert dx.data_ptr() == dx_into.data_ptr(), \
            "the accumulating epilogue was not taken"
        GB.within({"dx": dx}, {"dx": orc["dx"]}, f"dx_acc/{cls} BN={bn}")
        got[bn] = dx.clone()
    _force(monkeypatch, None)
    assert ext_plan(2 * 8 * 8, 24, 160)[1] == 48
    assert torch.equal(got[None], got["128"])


def ext_plan(m, n, k):
    return tuple(ops.native().conv_fwd_plan(m, n, k))


# ---- epilogue paths.  The 16-byte epilogue needs N, ldc and the column
# offset in multiples of 8 and a 16-byte aligned C; every other view must
# take the element-wise path even when the vector one is asked for, and all
# of them must hold the same bits.  Views: (element offset, ldc, N, vec).
VIEWS = [
    (0, 104, 104, 1),     # aligned: the vector path
    (0, 104, 104, 0),     # the same view, element-wise
    (0, 104, 104, -1),    # automatic
    (1, 107, 104, 1),     # odd offset, odd stride
    (0, 107, 104, 1),     # ldc % 8 != 0
    (4, 104, 104, 1),     # C 8 bytes off alignment
    (0, 104, 100, 1),     # ragged last columns: N % 8 != 0
]


@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("accum", (False, True))
def test_epilogue_paths(cls, accum):
    c = GB.ccase(2, 16, 9, 9, 104, 3, pad=1, relu=not accum, density=0.5)
    inp = GB.conv_inputs(c, cls, 770 + CLASSES.index(cls))
    orc, peak = GB.conv_oracle(c, inp)
    n, ch, k = c["n"], c["c"], c["k"]
    p, q = GB.conv_dims(c)
    npq, kcol = n * p * q, 9 * ch
    kpad = GB.kpad_dma(kcol)
    ext = ops.native()
    xd = inp["x"].permute(0, 2, 3, 1).contiguous().to(BF).to(dev())
    wrb = torch.zeros(128, kpad, dtype=BF)
    wrb[:k, :kcol] = inp["w"].permute(0, 2, 3, 1).reshape(k, kcol).to(BF)
    wrb, bias = wrb.to(dev()), inp["b"].to(dev())
    geom = [c["h"], c["w"], ch, p, q, 1, 1, 1, 1, 1, 3, 0, ch, kcol]
    g = GB.gen(780)
    c0 = torch.randint(-8, 9, (npq, k), generator=g).float().to(BF)
    ref = None
    for off, ldc, nn, vec in VIEWS:
        buf = torch.full((PADEL + off + npq * ldc + PADEL,), GB.SENT,
                         dtype=BF)
        view = buf[PADEL + off:PADEL + off + npq * ldc].view(npq, ldc)
        view[:, :nn] = c0[:, :nn]
        bd = buf.to(dev())
        ext.gemm_conv_fwd(xd, wrb, bd[PADEL + off:], bias[:nn],
                          G._zpage(dev()), npq, nn, kpad, kpad, ldc,
                          c["relu"], accum, geom, 1, 0, 0, 0, -1, vec)
        torch.cuda.synchronize()
        what = f"view {(off, ldc, nn, vec)}"
        h = bd.cpu()
        assert (h[:PADEL + off] == GB.SENT).all(), what
        assert (h[PADEL + off + npq * ldc:] == GB.SENT).all(), what
        hv = h[PADEL + off:PADEL + off + npq * ldc].view(npq, ldc)
        assert (hv[:, nn:] == GB.SENT).all(), what
        got = hv[:, :nn].clone()
        if ref is None:
            ref = got
            assert torch.isfinite(ref.float()).all()
            if not accum:
                GB.within({"y": ref.view(n, p, q, k).permute(0, 3, 1, 2)},
                          {"y": orc["y"]}, f"vector epilogue/{cls}")
        assert torch.equal(ref[:, :nn], got), what


# ---- the padding property, at the launches of an AlexNet step (batch
# 256): (M, N, K) and the fixed 128-wide kernel's (waves, depth)
ALEXNET = [
    (774400, 96, 448, 8, 4), (186624, 128, 1216, 8, 2),
    (186624, 48, 3200, 8, 2), (43264, 384, 2304, 4, 2),
    (43264, 256, 3456, 8, 2), (43264, 192, 1728, 8, 2),
    (43264, 192, 1728, 8, 2), (43264, 128, 1728, 8, 2),
    (43264, 192, 1152, 8, 4),
]


def test_plan_pads_to_16(monkeypatch):
    monkeypatch.delenv("COS_CONV_BN", raising=False)
    monkeypatch.delenv("COS_CONVQ", raising=False)
    monkeypatch.delenv("COS_GEMM_W8", raising=False)
    for m, n, k, _, _ in ALEXNET:
        bm, bn, waves, depth = ext_plan(m, n, k)
        assert bn in (48, 64, 96, 128) and bm in (128, 256)
        assert -(-n // bn) * bn == -(-n // 16) * 16, (m, n, k, bn)
    monkeypatch.setenv("COS_CONV_BN", "128")
    for m, n, k, waves, depth in ALEXNET:
        assert ext_plan(m, n, k) == (128, 128, waves, depth), (m, n, k)
