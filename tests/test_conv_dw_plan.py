"""conv_dw_plan (ops/gpu.py) and a numpy model of dw_slab_finalize's two
index maps (repack.hip).  CPU only.

The planner: one grouped launch of about 256 blocks over all groups, every
split at least one 32-wide K tile and none empty, _splitk_tt's caps kept
(no split below K = 1024, at least 512 K per split), slab bytes
splits * G*Kg * Kpad * 4, and G = 1 the count _splitk_dw gives today.

The maps: finalize walks slab columns and scatters into [Kout][Cg][R][S];
for both column orders the map from the non-pad, non-phantom columns must
be a bijection onto the filter's Cg*R*S elements, and must invert the pack
side (the plain (r*S+s)*Cg + c order, and s2d_col).
"""

import numpy as np
import pytest

from caffeonspark_amd.ops import gpu as G

TARGET = 256
BK = 32

# (name, G, Kg, Kpad, NPQ)
ALEXNET = [
    ("conv1_s2d", 1, 96, 448, 256 * 55 * 55),
    ("conv2", 2, 128, 1216, 256 * 27 * 27),
    ("conv3", 1, 384, 2304, 256 * 13 * 13),
    ("conv4", 2, 192, 1728, 256 * 13 * 13),
    ("conv5", 2, 128, 1728, 256 * 13 * 13),
]
GOOGLENET = [   # batch 32: the 3x3 and 5x5 branch shapes, first to last
    ("conv2_3x3", 1, 192, 576, 32 * 56 * 56),
    ("3a_3x3", 1, 128, 864, 32 * 28 * 28),
    ("3a_5x5", 1, 32, 416, 32 * 28 * 28),
    ("3b_3x3", 1, 192, 1152, 32 * 28 * 28),
    ("4a_3x3", 1, 208, 864, 32 * 14 * 14),
    ("4e_5x5", 1, 128, 800, 32 * 14 * 14),
    ("5b_3x3", 1, 384, 1728, 32 * 7 * 7),
    ("5b_5x5", 1, 128, 1216, 32 * 7 * 7),
]
DEGENERATE = [
    ("below_one_tile", 2, 96, 288, 18),
    ("one_tile", 1, 96, 160, 32),
    ("k_below_1024", 2, 192, 288, 1023),
    ("k_1024", 2, 192, 288, 1024),
    ("tiles_exceed_target", 4, 512, 4608, 8192),
]
SHAPES = ALEXNET + GOOGLENET + DEGENERATE


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in ("COS_DW_SLAB", "COS_DW_TR", "COS_DW_TT", "COS_FUSE_DB",
              "COS_SPLITK_TARGET"):
        monkeypatch.delenv(k, raising=False)


def _tiles(Kg, Kpad):
    nb = -(-Kpad // 256) if Kpad > 128 else -(-Kpad // 128)
    return -(-Kg // 128) * nb


@pytest.mark.parametrize("name,g,kg,kpad,npq", SHAPES,
                         ids=[s[0] for s in SHAPES])
def test_plan(name, g, kg, kpad, npq, monkeypatch):
    monkeypatch.setenv("COS_DW_SLAB", "1")      # the slab route at any size
    route, splits, slab_bytes = G.conv_dw_plan(g, kg, kpad, npq)
    assert route == "slab"
    tiles = g * _tiles(kg, kpad)
    # about one block per CU over all groups; a layer with more tiles than
    # the target runs one split
    assert splits >= 1
    assert splits == 1 or tiles * splits <= TARGET
    # every split at least one K tile, none empty (split_k's arithmetic)
    ksplit = -(-(-(-npq // splits)) // BK) * BK
    assert ksplit >= BK and ksplit % BK == 0
    assert (splits - 1) * ksplit < npq <= splits * ksplit
    assert G._split_count(npq, splits) == splits      # a fixed point
    # _splitk_tt's caps
    if npq < 1024:
        assert splits == 1
    assert splits <= max(1, npq // 512)
    # slab workspace
    want = splits * g * kg * kpad * 4 if splits > 1 else 0
    assert slab_bytes == want
    if g == 1:
        assert splits == G._split_count(
            npq, G._splitk_dw(kg, kpad, npq, True))


def test_small_slabs_keep_legacy(monkeypatch):
    """Unforced, a layer whose slabs would hold less than
    _DW_SLAB_MIN_BYTES keeps the legacy route and reports its splits."""
    for name, g, kg, kpad, npq in SHAPES:
        auto = G.conv_dw_plan(g, kg, kpad, npq)
        monkeypatch.setenv("COS_DW_SLAB", "1")
        slab = G.conv_dw_plan(g, kg, kpad, npq)
        monkeypatch.delenv("COS_DW_SLAB")
        if slab[2] >= G._DW_SLAB_MIN_BYTES:
            assert auto == slab
        else:
            assert auto == ("legacy", G._split_count(
                npq, G._splitk_dw(kg, kpad, npq, True)), 0)
    for _, g, kg, kpad, npq in ALEXNET:
        assert G.conv_dw_plan(g, kg, kpad, npq)[0] == "slab"
    # CIFAR-10 quick, batch 100: conv2 and conv3
    assert G.conv_dw_plan(1, 32, 800, 100 * 16 * 16)[0] == "legacy"
    assert G.conv_dw_plan(1, 64, 800, 100 * 8 * 8)[0] == "legacy"


def test_alexnet_splits():
    """The counts the grouped launch is built for: a two-group layer gets
    half the per-group splits of today's per-group launches."""
    got = {n: G.conv_dw_plan(g, kg, kpad, npq)[1]
           for n, g, kg, kpad, npq in ALEXNET}
    assert got == {"conv1_s2d": 128, "conv2": 25, "conv3": 9, "conv4": 9,
                   "conv5": 18}
    for n, g, kg, kpad, npq in ALEXNET:
        if g == 2:
            legacy = G._split_count(npq, G._splitk_dw(kg, kpad, npq, True))
            assert got[n] in (legacy // 2, (legacy + 1) // 2)


@pytest.mark.parametrize("env,val", [("COS_DW_SLAB", "0"), ("COS_DW_TR", "0"),
                                     ("COS_DW_TT", "0"), ("COS_FUSE_DB", "1")])
def test_legacy_switches(monkeypatch, env, val):
    monkeypatch.setenv(env, val)
    for _, g, kg, kpad, npq in ALEXNET:
        route, splits, slab_bytes = G.conv_dw_plan(g, kg, kpad, npq)
        assert route == "legacy" and slab_bytes == 0
        assert splits == G._split_count(
            npq, G._splitk_dw(kg, kpad, npq, True))


def test_unaligned_is_legacy():
    assert G.conv_dw_plan(2, 192, 1728, 43264, aligned=False)[0] == "legacy"


# ------------------------------------------------ finalize's index maps

def _s2d_col(c, r, s, Cg, S, st):
    """s2d_col of repack.hip (the pack side)"""
    Sp = -(-S // st)
    rp, dy = divmod(r, st)
    sp, dx = divmod(s, st)
    return ((rp * Sp + sp) * st * st + dy * st + dx) * Cg + c


def _finalize_map(col, Cg, R, S, st):
    """dw_slab_finalize_kernel's column -> (c, r, s), None for a phantom
    tap; mirrors the kernel's integer arithmetic line by line."""
    tap, c = divmod(col, Cg)
    if st >= 2:
        Sp = -(-S // st)
        tp, d = divmod(tap, st * st)
        rp = tp // Sp
        dy = d // st
        r = rp * st + dy
        sx = (tp - rp * Sp) * st + (d - dy * st)
        if r >= R or sx >= S:
            return None
    else:
        r = tap // S
        sx = tap - r * S
    return c, r, sx


def _ncol(Cg, R, S, st):
    if st >= 2:
        return -(-R // st) * -(-S // st) * st * st * Cg
    return R * S * Cg


MAPS = [  # Cg, R, S, st
    (48, 5, 5, 0), (16, 3, 3, 0), (8, 1, 7, 0), (3, 11, 11, 4),
    (48, 3, 3, 2), (3, 7, 7, 2), (8, 5, 3, 3),
]


@pytest.mark.parametrize("Cg,R,S,st", MAPS)
def test_finalize_map_is_bijection(Cg, R, S, st):
    ncol = _ncol(Cg, R, S, st)
    hit = np.zeros((Cg, R, S), dtype=np.int64)
    phantom = 0
    for col in range(ncol):
        m = _finalize_map(col, Cg, R, S, st)
        if m is None:
            phantom += 1
            continue
        c, r, s = m
        assert 0 <= c < Cg and 0 <= r < R and 0 <= s < S
        hit[c, r, s] += 1
        # inverse of the pack side
        want = _s2d_col(c, r, s, Cg, S, st) if st >= 2 \
            else (r * S + s) * Cg + c
        assert want == col
    assert (hit == 1).all()
    assert phantom == ncol - Cg * R * S
    if st < 2:
        assert phantom == 0
