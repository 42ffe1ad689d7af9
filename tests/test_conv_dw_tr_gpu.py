"""The DMA-staged conv dW GEMM (gemm_conv_dw_tr_kernel in gemm.hip) against
a float64 oracle, through _ext.gemm_conv_dw so the split count is forced.

Oracle: dy64^T @ col64 from the same bf16-rounded tensors, col built by
F.unfold on the CPU.

Tolerance (derived, not measured).  bf16 x bf16 products are exact in fp32
(8 + 8 significand bits), so the only roundings are the fp32 accumulation of
the K products — in the MFMA and across K tiles — the `splits` atomic adds
onto C, and the multiplication by alpha.  Rule B3 of _bf16_bounds.py charges
an fp32 accumulation of n terms n * 2^-24 * sum|terms| in any order, single
operations folded in as +4:

    |got - want| <= (K + splits + 4) * 2^-24 * |alpha| * (|dy|^T @ |col|)

elementwise.  Columns Kcol..N-1 of C are padding and must be exactly 0.

Every case is poisoned: dy and x live inside larger buffers filled with NaN
on both sides (dy also between its rows when lda > Kout), and C is
pre-filled with NaN for the plain-store mode, so anything staged from out of
range, or any output left unwritten, shows up as NaN.

Shapes are the smallest at which each mechanism can go wrong: M = 96 is one
partial 128-row tile and M = 192 a second tile half valid; Cg = 16 gives
Kcol 144 in N 160 (one 256-column block, 16 pad columns), Cg = 32 gives 288
(two blocks); NPQ = 2*7*7 = 98 is 4 K tiles with a 2-row tail, one split,
two splits of 64 and 34 rows (splitk 3) or four single-tile splits (splitk
4).
"""

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


def dev():
    return torch.device("cuda:0")


def case(**kw):
    c = dict(n=2, hw=7, c=16, groups=1, kout=96, ks=3, stride=1, pad=1,
             dil=1, dy_extra=16, dy_off=8, splitk=1, store=1, alpha=1.0)
    c.update(kw)
    return c


CASES = {
    # K tails and splits, N pad columns (Kcol 144 in N 160), M = 96
    "split1_store": case(),
    "split3_atomic": case(splitk=3, store=2),
    "split4_single_tile_splits": case(splitk=4, store=2),
    "split1_atomic": case(store=2),
    # two n-blocks (Kcol 288), second m-tile half valid (M = 192)
    "two_nblocks_m192": case(c=32, kout=192),
    "two_nblocks_m192_split3": case(c=32, kout=192, splitk=3, store=2),
    # geometry
    "stride2": case(hw=13, stride=2),
    "dilation2": case(pad=2, dil=2, splitk=3, store=2),
    "groups2": case(c=32, groups=2, kout=192),
    "groups2_split4": case(c=32, groups=2, kout=192, splitk=4, store=2),
    "dense_dy": case(dy_extra=0, dy_off=0),
    "s2d_geometry": case(hw=9, c=48, pad=0, splitk=3, store=2),
    "alpha": case(alpha=-0.37, splitk=3, store=2),
    "alpha_store": case(alpha=0.37),
}


def _split_count(k, splitk):
    """zblocks of split_k() in gemm.hip"""
    ks = -(-k // max(1, splitk))
    ks = -(-ks // 32) * 32
    return -(-k // ks)


def _poisoned(t, pre=PAD, post=PAD):
    """`t` copied into the middle of a NaN-filled device buffer; returns the
    view (same shape, contiguous) — its data pointer is 16-byte aligned."""
    flat = torch.full((pre + t.numel() + post,), NAN, dtype=t.dtype,
                      device=dev())
    view = flat[pre:pre + t.numel()].view(t.shape)
    view.copy_(t)
    return view


def _run(c, seed):
    g = torch.Generator().manual_seed(seed)
    n, hw, ch, grp, kout = c["n"], c["hw"], c["c"], c["groups"], c["kout"]
    ks, st, pad, dil = c["ks"], c["stride"], c["pad"], c["dil"]
    cg, kg = ch // grp, kout // grp
    p = (hw + 2 * pad - dil * (ks - 1) - 1) // st + 1
    npq = n * p * p
    kcol = ks * ks * cg
    npad = -(-kcol // 32) * 32
    lda = kout + c["dy_extra"]

    x = torch.randn(n, ch, hw, hw, generator=g).to(BF)
    dy = torch.randn(npq, kout, generator=g).to(BF)

    x_dev = _poisoned(x.permute(0, 2, 3, 1).contiguous())      # NHWC
    dy_rows = torch.full((npq, lda), NAN, dtype=BF)
    dy_rows[:, c["dy_off"]:c["dy_off"] + kout] = dy
    dy_dev = _poisoned(dy_rows)
    zpage = G._zpage(dev())
    ext = ops.native()

    splits = _split_count(npq, c["splitk"])
    alpha = c["alpha"]
    worst = 0.0
    for gi in range(grp):
        fill = NAN if c["store"] == 1 else 0.0
        cbuf = torch.full((kg, npad), fill, dtype=torch.float32,
                          device=dev())
        a = dy_dev[:, c["dy_off"] + gi * kg:]
        geom = [hw, hw, ch, p, p, st, st, pad, pad, dil, ks, gi * cg, cg,
                kcol]
        ext.gemm_conv_dw(a, x_dev, cbuf, None, zpage, kg, npad, npq, lda,
                         npad, c["store"], c["splitk"], alpha, geom)
        got = cbuf.cpu().double()

        xg = x[:, gi * cg:(gi + 1) * cg].double()
        cols = F.unfold(xg, ks, dilation=dil, padding=pad, stride=st)
        # unfold orders rows (c, r, s); the kernel's column is (r*S+s)*Cg+c
        col = cols.view(n, cg, ks * ks, p * p).permute(0, 3, 2, 1).reshape(
            npq, kcol)
        dyg = dy[:, gi * kg:(gi + 1) * kg].double()
        want = alpha * (dyg.t() @ col)
        bound = (npq + splits + 4) * E32 * abs(alpha) * (
            dyg.abs().t() @ col.abs())

        assert torch.isfinite(got).all(), "NaN/inf reached the output"
        err = (got[:, :kcol] - want).abs()
        used = (err / bound.clamp_min(1e-300)).max().item()
        worst = max(worst, used)
        print(f"group {gi}: max err {err.max().item():.3e}, "
              f"max err/bound {used:.3f}")
        assert (err <= bound).all(), \
            f"group {gi}: {int((err > bound).sum())} beyond the bound, " \
            f"worst err/bound {used:.3f}"
        assert (got[:, kcol:] == 0).all(), "pad columns not exactly 0"
    return worst


@pytest.mark.parametrize("name", list(CASES))
def test_conv_dw_tr(name):
    _run(CASES[name], 1000 + list(CASES).index(name))


@pytest.mark.parametrize("name", ["split1_store", "split3_atomic", "groups2"])
def test_fallback_env(name, monkeypatch):
    """COS_DW_TR=0 routes the same call to the register-staged kernel."""
    monkeypatch.setenv("COS_DW_TR", "0")
    _run(CASES[name], 2000)


@pytest.mark.parametrize("store,splitk", [(1, 1), (2, 3)])
def test_fallback_unaligned_lda(store, splitk):
    """lda % 8 != 0: dy rows are not 16-byte aligned, old kernel."""
    _run(case(dy_extra=4, dy_off=0, store=store, splitk=splitk), 3000)
