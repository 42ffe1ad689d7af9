"""gemm_conv_fwd's two A stagings: walked addresses (incr=1) against the
divide form (incr=0).

Only source addresses differ between them: the same bytes land in the same
LDS positions and the MFMA order is the same, so the outputs must be equal
bit for bit, not merely close.  Every comparison runs on NaN-filled output
views inside sentinel buffers (an element one staging leaves unwritten
stays NaN and fails torch.equal) and on an input with NaN on both sides and
in every channel outside the group window (an address that is off by
anything reads one).  One case per N tile is also held to the float64
bounds of _gemm_bounds.py, so "equal" cannot mean "equally wrong".

Shapes: batch 2 on 9x9 to 13x13 images, NPQ never a multiple of the block
rows.  Cg = 32 carries into s on every K tile, 40 and 48 carry in the
middle of a tile, 128 rarely; 8 and 24 take the divide form under either
argument (the walk needs Cg >= 32) and must say so in the plan."""

import pytest
import torch

import _gemm_bounds as GB
from _gemm_bounds import BF, NAN, PADEL

pytestmark = pytest.mark.gpu

from caffeonspark_amd import ops
from caffeonspark_amd.ops import gpu as G

GAP = 8             # NaN channels after every group's window


def dev():
    return torch.device("cuda:0")


CASES = {
    # the carry: every tile, mid-tile (Kcol 360 and 432: zero tail octets in
    # the last K tile), rare
    "cg32": GB.ccase(2, 32, 9, 9, 40, 3, pad=1),
    "cg40": GB.ccase(2, 40, 9, 9, 40, 3, pad=1, relu=True),
    "cg48": GB.ccase(2, 48, 10, 9, 40, 3, pad=1),
    "cg128": GB.ccase(2, 128, 9, 9, 40, 3, pad=1, density=0.25),
    # Cg < 32: the divide form whatever incr says
    "cg8": GB.ccase(2, 8, 9, 9, 40, 3, pad=1),
    "cg24": GB.ccase(2, 24, 9, 9, 40, 3, pad=1),
    # kernel shapes: 1xS and Rx1 (s and r never carry), 5x5 dilated
    "1x3": GB.ccase(2, 32, 9, 10, 40, 1, 3, pad=1),
    "3x1": GB.ccase(2, 32, 10, 9, 40, 3, 1, pad=1),
    "5x5_dil2": GB.ccase(2, 32, 13, 13, 40, 5, dil=2, pad=4, density=0.25),
    "stride2": GB.ccase(2, 40, 13, 13, 40, 3, stride=2, pad=1),
    # K of exactly two tiles (1x2 taps of 32 channels) and three
    "k2tiles": GB.ccase(2, 32, 9, 9, 40, 1, 2, pad=1),
    "k3tiles": GB.ccase(2, 32, 9, 9, 40, 1, 3, pad=1),
    # two groups: the second window starts at a nonzero c0
    "g2_cg32": GB.ccase(2, 64, 9, 9, 48, 3, pad=1, groups=2),
    "g2_cg40": GB.ccase(2, 80, 9, 9, 112, 3, pad=1, groups=2, relu=True),
    # N of 104: ragged for every tile width, several N tiles for 48-96
    "k104": GB.ccase(2, 40, 11, 9, 104, 3, pad=1, density=0.5),
}

_CACHE = {}


def _prepared(name, cls="rounded"):
    """Device operands and the float64 oracle of a case, built once."""
    key = (name, cls)
    if key in _CACHE:
        return _CACHE[key]
    c = CASES[name]
    inp = GB.conv_inputs(c, cls, 900 + list(CASES).index(name))
    orc, _ = GB.conv_oracle(c, inp)
    # (a one-tap dimension cannot have both kinds of tap on a border)
    assert min(c["r"], c["s"]) == 1 or GB.conv_geometry_ok(c)
    g, n, ch, k = c["groups"], c["n"], c["c"], c["k"]
    cg, kg = ch // g, k // g
    p, q = GB.conv_dims(c)
    kcol = c["r"] * c["s"] * cg
    kpad = GB.kpad_dma(kcol)
    cs = cg + GAP
    xw = torch.full((n, c["h"], c["w"], g * cs), NAN)
    for gi in range(g):
        xw[..., gi * cs:gi * cs + cg] = \
            inp["x"][:, gi * cg:(gi + 1) * cg].permute(0, 2, 3, 1)
    flat = torch.full((PADEL + xw.numel() + PADEL,), NAN, dtype=BF)
    flat[PADEL:PADEL + xw.numel()] = xw.reshape(-1).to(BF)
    wrb = torch.zeros((g - 1) * kg + -(-kg // 128) * 128, kpad, dtype=BF)
    wrb[:k, :kcol] = inp["w"].permute(0, 2, 3, 1).reshape(k, kcol).to(BF)
    geom = [c["h"], c["w"], g * cs, p, q, c["stride"], c["stride"],
            c["pad"], c["pad"], c["dil"], c["s"], 0, cg, kcol]
    out = dict(c=c, orc=orc, xd=flat.to(dev())[PADEL:], wrb=wrb.to(dev()),
               bias=inp["b"].to(dev()), geom=geom, npq=n * p * q, p=p, q=q,
               kg=kg, cg=cg, cs=cs, kpad=kpad, inp=inp)
    _CACHE[key] = out
    return out


def _launch(d, incr, cfg=-1, grouped=True, accum_onto=None, ld_x=8):
    """One forward GEMM per group (or one grouped launch) into a fresh
    buffer; returns the whole flat buffer on the host and its row stride."""
    c, g, k, kg = d["c"], d["c"]["groups"], d["c"]["k"], d["kg"]
    fill = NAN if accum_onto is None else accum_onto
    cflat, _, ldc = GB.out_buf(d["npq"], k, BF, fill, ld_x=ld_x)
    cd = cflat.to(dev())
    ext, zpage = ops.native(), G._zpage(dev())
    acc = accum_onto is not None
    if grouped:
        ext.gemm_conv_fwd(d["xd"], d["wrb"], cd[PADEL:], d["bias"], zpage,
                          d["npq"], kg, d["kpad"], d["kpad"], ldc, c["relu"],
                          acc, d["geom"], g, d["cs"], kg, kg, cfg, -1, incr)
    else:
        for gi in range(g):
            gg = list(d["geom"])
            gg[11] = gi * d["cs"]
            ext.gemm_conv_fwd(d["xd"], d["wrb"][gi * kg:],
                              cd[PADEL + gi * kg:],
                              d["bias"][gi * kg:(gi + 1) * kg], zpage,
                              d["npq"], kg, d["kpad"], d["kpad"], ldc,
                              c["relu"], acc, gg, 1, 0, 0, 0, cfg, -1, incr)
    torch.cuda.synchronize()
    assert GB.outside_untouched(cd, d["npq"], k, ldc), \
        f"incr={incr} cfg={cfg}: wrote outside the output view"
    return cd.cpu(), ldc


def _view(flat, d, ldc):
    c = d["c"]
    got = flat[PADEL:PADEL + d["npq"] * ldc].view(d["npq"], ldc)[:, :c["k"]]
    return got.view(c["n"], d["p"], d["q"], c["k"]).permute(0, 3, 1, 2)


def _staging(d, incr):
    return ops.native().conv_fwd_plan(d["npq"], d["kg"], d["kpad"],
                                      d["geom"], incr)[4]


@pytest.mark.parametrize("name", [n for n in CASES if n != "k104"])
def test_incr_equals_divide(name, monkeypatch):
    monkeypatch.delenv("COS_CONV_BN", raising=False)
    monkeypatch.delenv("COS_CONV_INCR", raising=False)
    d = _prepared(name)
    walked = d["cg"] >= 32
    assert _staging(d, 1) == int(walked)
    assert _staging(d, -1) == int(walked)
    assert _staging(d, 0) == 0
    for grouped in ((True, False) if d["c"]["groups"] > 1 else (True,)):
        old, ldc = _launch(d, 0, grouped=grouped)
        new, _ = _launch(d, 1, grouped=grouped)
        assert torch.isfinite(_view(old, d, ldc).float()).all(), name
        assert torch.equal(new, old), f"{name} grouped={grouped}"
    # the element-wise epilogue (odd row stride) sees the same accumulators
    old, _ = _launch(d, 0, ld_x=3)
    new, _ = _launch(d, 1, ld_x=3)
    assert torch.equal(new, old), f"{name} element-wise epilogue"


@pytest.mark.parametrize("bn", ["48", "64", "96", "128"])
def test_every_n_tile_within_bounds(bn, monkeypatch):
    """Each forced N tile: walked == divided, and inside the float64 bound."""
    monkeypatch.setenv("COS_CONV_BN", bn)
    monkeypatch.delenv("COS_CONV_INCR", raising=False)
    d = _prepared("k104")
    assert ops.native().conv_fwd_plan(d["npq"], d["kg"], d["kpad"])[1] == \
        int(bn)
    assert _staging(d, -1) == 1
    old, ldc = _launch(d, 0)
    new, _ = _launch(d, 1)
    assert torch.equal(new, old), f"BN={bn}"
    GB.within({"y": _view(new, d, ldc)}, {"y": d["orc"]["y"]},
              f"k104 incr=1 BN={bn}")


@pytest.mark.parametrize("name", ["k2tiles", "k3tiles", "cg40"])
def test_every_configuration(name):
    """Every instantiation (depth 2 and 4, A_CPW 1 and 2) at two tiles (the
    loop body never runs), three (once; at depth 4 never) and twelve."""
    d = _prepared(name)
    assert d["kpad"] == {"k2tiles": 64, "k3tiles": 96, "cg40": 384}[name]
    table = ops.native().conv_fwd_cfgs()
    assert {t[3] for t in table} == {2, 4}
    ref = None
    for cfg in range(len(table)):
        old, ldc = _launch(d, 0, cfg=cfg)
        new, _ = _launch(d, 1, cfg=cfg)
        assert torch.equal(new, old), f"{name} cfg {cfg} {table[cfg]}"
        if ref is None:
            ref = old
            GB.within({"y": _view(new, d, ldc)}, {"y": d["orc"]["y"]},
                      f"{name} cfg 0")
        assert torch.equal(new, ref), f"{name} cfg {cfg} against cfg 0"


def test_accumulating_epilogue():
    """accum=1, the dx fan-in form: both stagings add onto the same bits."""
    d = _prepared("g2_cg40")
    g = GB.gen(977)
    onto = GB.rb(torch.randn((d["npq"], d["c"]["k"]), generator=g) * 2).to(BF)
    old, _ = _launch(d, 0, accum_onto=onto)
    new, ldc = _launch(d, 1, accum_onto=onto)
    plain, _ = _launch(d, 1)
    assert torch.equal(new, old)
    assert not torch.equal(new, plain), "nothing was accumulated"
    assert torch.isfinite(_view(new, d, ldc).float()).all()


def test_env_switch_and_dx_route(monkeypatch):
    """COS_CONV_INCR=0 reaches the layer code (read per call), and the
    accumulating implicit dx (a convolution of dy, Cg = Kg = 64) is the same
    bits either way and inside its float64 bound."""
    c = GB.ccase(2, 16, 9, 9, 64, 3, pad=1, dx_acc=True)
    inp = GB.conv_inputs(c, "rounded", 990)
    orc, _ = GB.conv_oracle(c, inp)
    geo = ((1, 1), (1, 1), (1, 1), 1)
    x, dy = inp["x"].to(BF).to(dev()), inp["dy"].to(BF).to(dev())
    ext = ops.native()
    geom_dx = [9, 9, 64, 9, 9, 1, 1, 1, 1, 1, 3, 0, 64, 9 * 64]
    got = {}
    for env in ("0", None):
        if env is None:
            monkeypatch.delenv("COS_CONV_INCR", raising=False)
        else:
            monkeypatch.setenv("COS_CONV_INCR", env)
        assert ext.conv_fwd_plan(162, 16, 576, geom_dx)[4] == \
            (0 if env == "0" else 1)
        assert ext.conv_fwd_plan(162, 16, 576, geom_dx, 1)[4] == 1
        w = inp["w"].to(dev())
        ctx = {}
        y = ops.conv2d_forward(x, w, inp["b"].to(dev()), *geo, ctx=ctx)
        assert ctx.get("implicit") is True
        dx_into = inp["dx0"].to(BF).to(dev()).contiguous(
            memory_format=torch.channels_last)
        dx, _, _ = ops.conv2d_backward(x, w, dy, *geo, need_dw=False,
                                       bias=False, ctx=ctx, dx_into=dx_into)
        torch.cuda.synchronize()
        assert dx.data_ptr() == dx_into.data_ptr()
        GB.within({"y": y, "dx": dx}, {"y": orc["y"], "dx": orc["dx"]},
                  f"COS_CONV_INCR={env}")
        got[env] = (y.clone(), dx.clone())
    assert torch.equal(got[None][0], got["0"][0])
    assert torch.equal(got[None][1], got["0"][1])
