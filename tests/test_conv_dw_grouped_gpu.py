"""The grouped slab route of the conv weight gradient: ONE launch of
gemm_conv_dw_tr_kernel over all groups into per-split slabs
(_ext.gemm_conv_dw_grouped), then dw_slab_finalize — the ordered slab sum
fused with the unpack to the caffe-layout arena — against a float64 oracle.

Oracle: dy64^T @ col64 from the same bf16-rounded tensors, col built by
F.unfold on the CPU.  unfold orders its rows (c, r, s), which IS the arena's
[Kout][Cg][R][S] order, so the oracle checks the GEMM's column order and the
finalize's inverse map together.  The space-to-depth case unfolds the
ORIGINAL 11 x 11 stride-4 convolution over 3 channels, while the kernel runs
the 3 x 3 stride-1 convolution over the 48 space-to-depth channels.

Tolerance (derived, not measured; rule B3 of _bf16_bounds.py).  bf16 x bf16
products are exact in fp32, so the roundings are the fp32 accumulation of
the NPQ products in the MFMA and across K tiles, the ordered fp32 sum of
`splits` slabs (the count the atomics had), and the multiplication by
alpha; single operations are folded in as +4:

    |got - want| <= (NPQ + splits + 4) * 2^-24 * |alpha| * (|dy|^T @ |col|)

per arena element.

Every case is poisoned: dy and x lie inside NaN-filled buffers (dy also
between its rows), the slabs are pre-filled with NaN and never zeroed — a
finite result proves every slab element the finalize reads was stored — and
the arena lies inside a NaN-filled buffer whose guards must stay NaN.

Shapes: n = 2, 7 x 7 outputs, NPQ = 98 = 4 K tiles with a 2-row tail; one
split, two uneven splits of 64 and 34 rows (splitk 3) and four single-tile
splits (splitk 4).  Kg = 96: the lower 64-row wave band has fragments 0-1
valid and 2-3 skipped; Kg = 72: a single, partial fragment of 8 rows;
Kg = 192: a second M tile whose lower band is skipped entirely.  Through
conv2d_backward the input is 23 x 23 (NPQ = 1058), the smallest at which
the planner splits K at all.
"""

import functools

import pytest
import torch
import torch.nn.functional as F

from _bf16_bounds import E32

pytestmark = pytest.mark.gpu

from caffeonspark_amd import ops
from caffeonspark_amd.ops import gpu as G

BF = torch.bfloat16
NAN = float("nan")
PAD = 64          # NaN elements on either side of every operand
ALPHA = -0.37

# name -> groups, Kg, channels, kernel, stride, pad, input size, s2d stride
CASES = {
    "g2_kg96": dict(grp=2, kg=96, c=32, ks=3, st=1, pad=1, hw=7, s2d=0),
    "g2_kg72": dict(grp=2, kg=72, c=32, ks=3, st=1, pad=1, hw=7, s2d=0),
    "g2_kg192": dict(grp=2, kg=192, c=32, ks=3, st=1, pad=1, hw=7, s2d=0),
    # the GEMM sees 9 x 9 x 48, 3 x 3, pad 0; the arena is [96][3][11][11]
    "s2d_kg96": dict(grp=1, kg=96, c=3, ks=11, st=4, pad=0, hw=36, s2d=4),
}
SPLITKS = (1, 3, 4)


def dev():
    return torch.device("cuda:0")


def _poisoned(t, pre=PAD, post=PAD, fill=NAN):
    """`t` copied into the middle of a NaN-filled device buffer; returns
    (view, whole buffer)."""
    flat = torch.full((pre + t.numel() + post,), fill, dtype=t.dtype,
                      device=dev())
    view = flat[pre:pre + t.numel()].view(t.shape)
    view.copy_(t)
    return view, flat


def _s2d(x, st):
    """NCHW -> the space-to-depth NHWC tensor the kernel reads:
    x'[n][h'][w'][(dy*st+dx)*C + c] = x[n][c][st*h'+dy][st*w'+dx]"""
    n, c, h, w = x.shape
    v = x.view(n, c, h // st, st, w // st, st)      # n c h' dy w' dx
    return v.permute(0, 2, 4, 3, 5, 1).reshape(n, h // st, w // st,
                                               st * st * c).contiguous()


@functools.lru_cache(maxsize=None)
def _inputs(name):
    """Host tensors, oracle and |.| product of a case — computed once and
    shared, never modified."""
    c = CASES[name]
    g = torch.Generator().manual_seed(4000 + list(CASES).index(name))
    n, grp, kg, ch, ks = 2, c["grp"], c["kg"], c["c"], c["ks"]
    kout, cg = grp * kg, ch // grp
    p = (c["hw"] + 2 * c["pad"] - ks) // c["st"] + 1
    npq = n * p * p
    x = torch.randn(n, ch, c["hw"], c["hw"], generator=g).to(BF)
    dy = torch.randn(npq, kout, generator=g).to(BF)
    want = torch.empty(kout, cg * ks * ks, dtype=torch.float64)
    absprod = torch.empty_like(want)
    for gi in range(grp):
        cols = F.unfold(x[:, gi * cg:(gi + 1) * cg].double(), ks,
                        padding=c["pad"], stride=c["st"])
        col = cols.permute(0, 2, 1).reshape(npq, cg * ks * ks)
        dyg = dy[:, gi * kg:(gi + 1) * kg].double()
        want[gi * kg:(gi + 1) * kg] = ALPHA * (dyg.t() @ col)
        absprod[gi * kg:(gi + 1) * kg] = abs(ALPHA) * (
            dyg.abs().t() @ col.abs())
    shape = (kout, cg, ks, ks)
    return dict(x=x, dy=dy, want=want.view(shape),
                absprod=absprod.view(shape), npq=npq, p=p, kout=kout,
                cg=cg, shape=shape)


def _operands(name):
    """Device operands of the GEMM as the kernel sees them."""
    c, inp = CASES[name], _inputs(name)
    kout, npq, p = inp["kout"], inp["npq"], inp["p"]
    if c["s2d"]:
        st = c["s2d"]
        xs = _s2d(inp["x"], st)
        rp = -(-c["ks"] // st)
        cp = st * st * c["c"]
        kcol = rp * rp * cp
        geom = [xs.shape[1], xs.shape[2], cp, p, p, 1, 1, 0, 0, 1, rp, 0,
                cp, kcol]
        x_dev, _ = _poisoned(xs)
    else:
        kcol = c["ks"] * c["ks"] * inp["cg"]
        geom = [c["hw"], c["hw"], c["c"], p, p, c["st"], c["st"], c["pad"],
                c["pad"], 1, c["ks"], 0, inp["cg"], kcol]
        x_dev, _ = _poisoned(inp["x"].permute(0, 2, 3, 1).contiguous())
    npad = -(-kcol // 32) * 32
    lda, off = kout + 16, 8
    rows = torch.full((npq, lda), NAN, dtype=BF)
    rows[:, off:off + kout] = inp["dy"]
    dy_dev, _ = _poisoned(rows)
    return x_dev, dy_dev[:, off:], lda, geom, kcol, npad


def _gemm(name, splitk, x_dev, a, lda, geom, npad, grp=None, kg=None):
    """Grouped launch into NaN-filled slabs; returns (slabs, wrote)."""
    c, inp = CASES[name], _inputs(name)
    grp = c["grp"] if grp is None else grp
    kg = c["kg"] if kg is None else kg
    splits = G._split_count(inp["npq"], splitk)
    slabs = torch.full((splits, grp * kg, npad), NAN, dtype=torch.float32,
                       device=dev())
    wrote = ops.native().gemm_conv_dw_grouped(
        a, x_dev, slabs, G._zpage(dev()), kg, npad, inp["npq"], lda, npad,
        splitk, ALPHA, geom, grp)
    assert wrote == splits
    return slabs, wrote


def _finalize(name, slabs, wrote, npad, arena, accumulate=False, kout=None,
              cg=None):
    c, inp = CASES[name], _inputs(name)
    ops.native().dw_slab_finalize(
        slabs, wrote, arena, inp["kout"] if kout is None else kout,
        inp["cg"] if cg is None else cg, c["ks"], c["ks"], c["s2d"], npad,
        accumulate, 0)


def _bound(name, splits):
    inp = _inputs(name)
    return (inp["npq"] + splits + 4) * E32 * inp["absprod"]


def _check(got, want, bound, what):
    assert torch.isfinite(got).all(), f"{what}: NaN/inf reached the arena"
    err = (got.double() - want).abs()
    used = (err / bound.clamp_min(1e-300)).max().item()
    print(f"{what}: max err {err.max().item():.3e}, "
          f"max err/bound {used:.3f}")
    assert (err <= bound).all(), \
        f"{what}: {int((err > bound).sum())} beyond the bound, " \
        f"worst err/bound {used:.3f}"


@pytest.mark.parametrize("splitk", SPLITKS)
@pytest.mark.parametrize("name", list(CASES))
def test_grouped_slab(name, splitk):
    c, inp = CASES[name], _inputs(name)
    x_dev, a, lda, geom, kcol, npad = _operands(name)
    shape = inp["shape"]
    zero = torch.zeros(shape, dtype=torch.float32)

    slabs, wrote = _gemm(name, splitk, x_dev, a, lda, geom, npad)
    arena, whole = _poisoned(zero)
    arena.fill_(NAN)
    _finalize(name, slabs, wrote, npad, arena)
    got = arena.cpu()
    _check(got, inp["want"], _bound(name, wrote),
           f"{name} splitk {splitk} ({wrote} slabs)")
    guards = torch.cat([whole[:PAD], whole[PAD + arena.numel():]])
    assert torch.isnan(guards).all(), "finalize wrote outside the arena"

    # the same inputs again, fresh NaN slabs: the same bits
    slabs2, wrote2 = _gemm(name, splitk, x_dev, a, lda, geom, npad)
    arena2 = torch.full(shape, NAN, dtype=torch.float32, device=dev())
    _finalize(name, slabs2, wrote2, npad, arena2)
    assert torch.equal(arena2.cpu(), got), "two runs differ"

    # one launch over the groups == a launch per group, bit for bit
    if c["grp"] > 1:
        kg, cg = c["kg"], inp["cg"]
        parts = []
        for gi in range(c["grp"]):
            gg = list(geom)
            gg[11] = gi * cg
            s_g, w_g = _gemm(name, splitk, x_dev, a[:, gi * kg:], lda, gg,
                             npad, grp=1, kg=kg)
            a_g = torch.full((kg,) + shape[1:], NAN, dtype=torch.float32,
                             device=dev())
            _finalize(name, s_g, w_g, npad, a_g, kout=kg)
            parts.append(a_g.cpu())
        assert torch.equal(torch.cat(parts), got), \
            "grouped launch differs from per-group launches"

    # accumulate onto a pre-filled arena == pre-fill + overwrite result
    # within one fp32 rounding; pad and phantom columns (poisoned here)
    # never reach the arena
    valid = torch.zeros(npad, dtype=torch.bool)
    for col in range(kcol):
        tap, ch = divmod(col, inp["cg"])
        if c["s2d"]:
            st = c["s2d"]
            sp_ = -(-c["ks"] // st)
            tp, d = divmod(tap, st * st)
            r = (tp // sp_) * st + d // st
            s = (tp % sp_) * st + d % st
            valid[col] = r < c["ks"] and s < c["ks"]
        else:
            valid[col] = True
    slabs[:, :, ~valid.to(dev())] = NAN
    g = torch.Generator().manual_seed(7)
    pre = torch.randn(shape, generator=g)
    acc, whole = _poisoned(pre)
    _finalize(name, slabs, wrote, npad, acc, accumulate=True)
    acc = acc.cpu()
    assert torch.isfinite(acc).all(), "a pad or phantom column was read"
    exact = pre.double() + got.double()
    assert ((acc.double() - exact).abs() <= E32 * exact.abs()).all(), \
        "accumulate is more than one rounding from pre-fill + result"
    guards = torch.cat([whole[:PAD], whole[PAD + acc.numel():]])
    assert torch.isnan(guards).all(), "finalize wrote outside the arena"


@pytest.mark.parametrize("how", ["env", "lda"])
def test_grouped_gate(how, monkeypatch):
    """Outside the DMA kernel's gate the grouped entry launches nothing and
    says so; the per-group entry point still serves those calls
    (tests/test_conv_dw_tr_gpu.py holds it to the same bound)."""
    name = "g2_kg96"
    inp = _inputs(name)
    x_dev, a, lda, geom, kcol, npad = _operands(name)
    if how == "env":
        monkeypatch.setenv("COS_DW_TR", "0")
    else:
        rows = torch.zeros((inp["npq"], inp["kout"] + 4), dtype=BF)
        rows[:, :inp["kout"]] = inp["dy"]
        a, _ = _poisoned(rows)
        lda = inp["kout"] + 4
    slabs = torch.full((1, inp["kout"], npad), NAN, dtype=torch.float32,
                       device=dev())
    wrote = ops.native().gemm_conv_dw_grouped(
        a, x_dev, slabs, G._zpage(dev()), CASES[name]["kg"], npad,
        inp["npq"], lda, npad, 1, ALPHA, geom, 2)
    assert wrote == 0
    assert torch.isnan(slabs).all(), "a kernel ran all the same"


def test_finalize_rejects_unaligned():
    """The finalize reads four columns with one 16-byte load: a slab view
    off by one float, or a row pitch that is no multiple of 4, is an error
    (no route produces either)."""
    ext = ops.native()
    arena = torch.zeros((8, 8, 1, 1), dtype=torch.float32, device=dev())
    flat = torch.zeros(8 * 36 + 4, dtype=torch.float32, device=dev())
    ext.dw_slab_finalize(flat[:8 * 32].view(1, 8, 32), 1, arena, 8, 8, 1, 1,
                         0, 32, False, 0)
    with pytest.raises(RuntimeError, match="16-byte"):
        ext.dw_slab_finalize(flat[1:1 + 8 * 32].view(1, 8, 32), 1, arena, 8,
                             8, 1, 1, 0, 32, False, 0)
    with pytest.raises(RuntimeError, match="16-byte"):
        ext.dw_slab_finalize(flat[:8 * 34].view(1, 8, 34), 1, arena, 8, 8, 1,
                             1, 0, 34, False, 0)


# ------------------------------------------------ through conv2d_backward

LAYERS = {
    # groups, Kout, C, kernel, stride, pad, input size
    "grouped": (2, 192, 32, 3, 1, 1, 23),
    "s2d": (1, 96, 3, 11, 4, 0, 4 * 22 + 11),
    "unaligned": (1, 100, 16, 3, 1, 1, 23),
}
ROUTED = ["grouped", "s2d"]


@functools.lru_cache(maxsize=None)
def _layer(name):
    grp, kout, ch, ks, st, pad, hw = LAYERS[name]
    g = torch.Generator().manual_seed(5000 + list(LAYERS).index(name))
    n, cg, kg = 2, ch // grp, kout // grp
    p = (hw + 2 * pad - ks) // st + 1
    npq = n * p * p
    x = torch.randn(n, ch, hw, hw, generator=g).to(BF)
    w = torch.randn(kout, cg, ks, ks, generator=g).to(BF)
    dy = torch.randn(n, kout, p, p, generator=g).to(BF)
    dy2 = dy.permute(0, 2, 3, 1).reshape(npq, kout)
    want = torch.empty(kout, cg * ks * ks, dtype=torch.float64)
    absprod = torch.empty_like(want)
    for gi in range(grp):
        cols = F.unfold(x[:, gi * cg:(gi + 1) * cg].double(), ks,
                        padding=pad, stride=st)
        col = cols.permute(0, 2, 1).reshape(npq, cg * ks * ks)
        dyg = dy2[:, gi * kg:(gi + 1) * kg].double()
        want[gi * kg:(gi + 1) * kg] = dyg.t() @ col
        absprod[gi * kg:(gi + 1) * kg] = dyg.abs().t() @ col.abs()
    shape = (kout, cg, ks, ks)
    return dict(x=x, w=w, dy=dy, npq=npq, shape=shape,
                want=want.view(shape), absprod=absprod.view(shape))


def _backward(name):
    grp, _, ch, ks, st, pad, hw = LAYERS[name]
    L = _layer(name)
    x, w, dy = L["x"].to(dev()), L["w"].to(dev()), L["dy"].to(dev())
    arena, whole = _poisoned(torch.zeros(w.shape, dtype=torch.float32))
    arena.fill_(NAN)
    ctx = {}
    _, dw, _ = G.conv2d_backward(x, w, dy, (st, st), (pad, pad), (1, 1),
                                 grp, need_dx=False, need_dw=True,
                                 bias=False, ctx=ctx, dw_out=arena)
    assert dw.data_ptr() == arena.data_ptr(), "dw_out was not used"
    guards = torch.cat([whole[:PAD], whole[PAD + arena.numel():]])
    assert torch.isnan(guards).all(), "wrote outside dw_out"
    return arena.cpu(), ctx


def _plan_args(name, ctx):
    (N, C, H, W, P, Q, R, S, sh, sw, ph, pw, dil, Gr, Cg, Kg, Kpad,
     Kcol) = ctx["shape"]
    if ctx.get("s2d"):
        Kpad = ctx["s2d"][7]
    return Gr, Kg, Kpad, N * P * Q


@pytest.mark.parametrize("name", ROUTED)
def test_conv2d_backward_routes(name, monkeypatch):
    L = _layer(name)
    for k in ("COS_DW_TR", "COS_SPLITK_TARGET"):
        monkeypatch.delenv(k, raising=False)
    # slabs this small keep the legacy route unless asked for
    monkeypatch.setenv("COS_DW_SLAB", "1")

    new, ctx = _backward(name)
    route, splits, _ = G.conv_dw_plan(*_plan_args(name, ctx))
    assert route == "slab" and ctx["dw_route"] == "slab"
    assert splits == 2        # NPQ = 1058: two splits of 544 and 514 rows
    b_new = (L["npq"] + splits + 4) * E32 * L["absprod"]
    _check(new, L["want"], b_new, f"{name} slab route")
    again, _ = _backward(name)
    assert torch.equal(new, again), "two runs of the slab route differ"

    monkeypatch.setenv("COS_DW_SLAB", "0")
    old, ctx = _backward(name)
    route, splits_old, _ = G.conv_dw_plan(*_plan_args(name, ctx))
    assert route == "legacy" and ctx["dw_route"] == "legacy"
    b_old = (L["npq"] + splits_old + 4) * E32 * L["absprod"]
    _check(old, L["want"], b_old, f"{name} COS_DW_SLAB=0")
    assert ((new.double() - old.double()).abs() <= b_new + b_old).all(), \
        "the two routes differ by more than the sum of their bounds"
    monkeypatch.delenv("COS_DW_SLAB")
    auto, ctx = _backward(name)
    assert ctx["dw_route"] == "legacy", "small slabs take the legacy route"
    monkeypatch.setenv("COS_DW_SLAB", "1")

    # fallbacks: the register-staged kernel, with atomics
    monkeypatch.setenv("COS_DW_TR", "0")
    old, ctx = _backward(name)
    route, splits_old, _ = G.conv_dw_plan(*_plan_args(name, ctx))
    assert route == "legacy" and ctx["dw_route"] == "legacy"
    _check(old, L["want"],
           (L["npq"] + splits_old + 4) * E32 * L["absprod"],
           f"{name} COS_DW_TR=0")


def test_conv2d_backward_unaligned_lda():
    """Kout = 100: dy rows of 100 elements are not 16-byte aligned, so the
    layer keeps the register-staged kernel and its atomics."""
    name = "unaligned"
    L = _layer(name)
    got, ctx = _backward(name)
    assert ctx["dw_route"] == "legacy"
    splits = G.conv_dw_plan(*_plan_args(name, ctx), aligned=False)[1]
    _check(got, L["want"], (L["npq"] + splits + 4) * E32 * L["absprod"],
           "lda % 8 != 0")
