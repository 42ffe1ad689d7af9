"""gemm_conv_fwd's large block tiles (256x128, 256x96 and, in a
-DCOS_CONV_SWEEP build, 128x192 and 256x192) against the 128x128 4-wave
tile, configuration 2.

Every tile runs one 16x16x32 MFMA per K tile in ascending k, so an output
element sees the same sum in the same order whatever the tile: the results
must be equal bit for bit.  Outputs live in NaN-filled buffers with spare
columns after each row and spare rows after row M; buffers are compared as
bit patterns, so an element a tile leaves unwritten, or writes outside its
group's columns or below row M, fails the comparison.

Shapes are the smallest that reach each path: N 192 (a whole 192-wide
tile), 200 (16-byte epilogue, an 8-column tail tile), 196 (N % 8 != 0: the
element-wise epilogue), 100 (less than one tile); M 130 (a row tail) and
300 (the second half of a 256-row block, ragged); Kpad 64 (two K tiles,
the minimum) and 288 / 96 (3x3 taps); Cg 32 (walked A staging) and 8 (the
divide form); two groups of N 192 in one launch; accum once."""

import pytest
import torch

from caffeonspark_amd import ops
from caffeonspark_amd.ops import gpu as G

BF = torch.bfloat16
REF_CFG = 2
SPARE_ROWS = 3
SPARE_COLS = 8

# name: (n, h, w, cg, r, s, pad, N per group, groups)
CASES = {
    "n192_m130_kpad64": (2, 5, 14, 32, 1, 2, 0, 192, 1),
    "n200_m300_3x3": (3, 10, 10, 32, 3, 3, 1, 200, 1),
    "n196_m300_cg8": (3, 10, 10, 8, 3, 3, 1, 196, 1),
    "n100_m130_cg8": (2, 5, 13, 8, 3, 3, 1, 100, 1),
    "g2_n192_m300": (3, 10, 10, 32, 3, 3, 1, 192, 2),
}
M_OF = {"n192_m130_kpad64": 130, "n200_m300_3x3": 300, "n196_m300_cg8": 300,
        "n100_m130_cg8": 130, "g2_n192_m300": 300}

_CACHE = {}


def dev():
    return torch.device("cuda:0")


def _pad(v, m):
    return -(-v // m) * m


def _case(name):
    """Device operands of a case, built once."""
    if name in _CACHE:
        return _CACHE[name]
    n, h, w, cg, r, s, pad, nn, g = CASES[name]
    p, q = h + 2 * pad - r + 1, w + 2 * pad - s + 1
    m = n * p * q
    assert m == M_OF[name]
    kcol = r * s * cg
    kpad = max(64, _pad(kcol, 32))
    gen = torch.Generator().manual_seed(4100 + list(CASES).index(name))
    x = torch.randn((n, h, w, g * cg), generator=gen).to(BF)
    # every group's rows at stride N, as the layer keeps them; the rows
    # up to the next multiple of 128 and the columns beyond Kcol are zero
    wrb = torch.zeros(((g - 1) * nn + _pad(nn, 128), kpad), dtype=BF)
    wrb[:g * nn, :kcol] = \
        (0.1 * torch.randn((g * nn, kcol), generator=gen)).to(BF)
    bias = torch.randn((g * nn,), generator=gen)
    onto = torch.randn((m, g * nn), generator=gen).to(BF)
    d = dict(m=m, nn=nn, g=g, cg=cg, kpad=kpad, ldc=g * nn + SPARE_COLS,
             geom=[h, w, g * cg, p, q, 1, 1, pad, pad, 1, s, 0, cg, kcol],
             x=x.to(dev()), wrb=wrb.to(dev()), bias=bias.to(dev()),
             onto=onto)
    _CACHE[name] = d
    return d


def _run(d, cfg, accum=False):
    """One launch into a fresh NaN-filled buffer; the whole buffer as bit
    patterns on the host."""
    m, nn, g, ldc = d["m"], d["nn"], d["g"], d["ldc"]
    c = torch.full((m + SPARE_ROWS, ldc), float("nan"), dtype=BF)
    if accum:
        c[:m, :g * nn] = d["onto"]
    cd = c.to(dev())
    ops.native().gemm_conv_fwd(
        d["x"], d["wrb"], cd, d["bias"], G._zpage(dev()), m, nn, d["kpad"],
        d["kpad"], ldc, False, accum, d["geom"], g, d["cg"], nn, nn, cfg)
    torch.cuda.synchronize()
    return cd.cpu().view(torch.int16)


def _wide_ids():
    table = ops.native().conv_fwd_cfgs()
    return [i for i, (bm, bn, _, _) in enumerate(table)
            if bn == 192 or (bm == 256 and bn >= 96)]


def _check(name, accum):
    d = _case(name)
    m, cols = d["m"], d["g"] * d["nn"]
    ref = _run(d, REF_CFG, accum)
    nan_bits = torch.full((1,), float("nan"), dtype=BF).view(torch.int16)[0]
    assert torch.isfinite(ref[:m, :cols].view(BF).float()).all(), name
    assert (ref[m:] == nan_bits).all() and (ref[:, cols:] == nan_bits).all()
    table = ops.native().conv_fwd_cfgs()
    for cfg in _wide_ids():
        got = _run(d, cfg, accum)
        assert torch.equal(got, ref), f"{name} cfg {cfg} {table[cfg]}"


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_wide_tiles_equal_reference_tile(name):
    _check(name, accum=False)


@pytest.mark.gpu
def test_wide_tiles_accumulate():
    d = _case("n200_m300_3x3")
    _check("n200_m300_3x3", accum=True)
    assert not torch.equal(_run(d, REF_CFG, True), _run(d, REF_CFG, False))


@pytest.mark.gpu
def test_wide_tiles_present():
    table = [tuple(t) for t in ops.native().conv_fwd_cfgs()]
    assert (256, 128, 8, 2) in table
    assert _wide_ids(), "no large tile to test"


# ---- the planner, host code only: no GPU needed
def _ext():
    import importlib
    return ops.native() or importlib.import_module(
        "caffeonspark_amd.ops._cosamd_hip")


# AlexNet, batch 256: (M, N per group, Kpad, groups) -> (BM, BN, waves,
# depth) as measured in profiles/alexnet_1gpu_conv_wide.md
ALEXNET_PLAN = [
    ((774400, 96, 448, 1), (256, 96, 8, 2)),       # conv1 fwd (s2d)
    ((186624, 128, 1216, 2), (256, 128, 8, 2)),    # conv2 fwd
    ((186624, 48, 3200, 2), (256, 48, 8, 2)),      # conv2 dx
    ((43264, 384, 2304, 1), (256, 128, 8, 2)),     # conv3 fwd
    ((43264, 256, 3456, 1), (128, 128, 8, 2)),     # conv3 dx
    ((43264, 192, 1728, 2), (256, 96, 8, 2)),      # conv4 fwd, conv4 dx
    ((43264, 128, 1728, 2), (128, 128, 8, 2)),     # conv5 fwd
    ((43264, 192, 1152, 2), (256, 96, 8, 2)),      # conv5 dx
]


def test_plan_alexnet_and_forced_width(monkeypatch):
    for k in ("COS_CONV_BN", "COS_CONVQ", "COS_GEMM_W8"):
        monkeypatch.delenv(k, raising=False)
    ext = _ext()
    for (m, n, k, g), want in ALEXNET_PLAN:
        assert tuple(ext.conv_fwd_plan(m, n, k, groups=g)) == want, (m, n, k)
    # below 384 blocks of 256 rows the 128-row tiles stay; small M too
    assert tuple(ext.conv_fwd_plan(43264, 192, 1728)) == (128, 96, 8, 2)
    assert tuple(ext.conv_fwd_plan(4096, 128, 1728, groups=64))[0] == 128
    # a forced width names the 128-row kernels of 96 and 128 columns
    monkeypatch.setenv("COS_CONV_BN", "128")
    assert tuple(ext.conv_fwd_plan(186624, 128, 1216, groups=2)) == \
        (128, 128, 8, 2)
    # 192 columns exist only in a sweep build; elsewhere asking is an error
    monkeypatch.setenv("COS_CONV_BN", "192")
    if any(t[1] == 192 for t in ext.conv_fwd_cfgs()):
        assert ext.conv_fwd_plan(43264, 192, 1728)[1] == 192
    else:
        with pytest.raises(RuntimeError, match="COS_CONV_SWEEP"):
            ext.conv_fwd_plan(43264, 192, 1728)
