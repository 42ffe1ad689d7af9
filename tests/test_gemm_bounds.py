"""CPU validation of the oracles in _gemm_bounds.py: for every case of every
table a torch fp32 emulation with the kernels' rounding points must sit
inside the derived bound (rounded class) or be bit-exact (exact class), the
exact class must satisfy its precondition, and every mutant must be rejected
by at least one case of its table.  This is what shows, without a GPU, that
test_gemm_bf16_gpu.py, test_conv_gemm_gpu.py and test_col_kernels_gpu.py
fail when a kernel is subtly wrong."""

import pytest
import torch

import _gemm_bounds as GB
from _gemm_bounds import violations, within

CLASSES = ("exact", "rounded")
GEMM_TABLE = dict(GB.GEMM_CASES, **GB.WIDE_CASES,
                  split3_bias=GB.RAISES_CASES["split3_bias"])


def _seed(table, name, cls):
    return 100 + 2 * list(table).index(name) + CLASSES.index(cls)


def _gemm_setup(name, cls):
    c = GEMM_TABLE[name]
    inp = GB.gemm_inputs(c, cls, _seed(GEMM_TABLE, name, cls))
    orc, peak = GB.gemm_oracle(c, inp)
    return c, inp, orc, peak


# --------------------------------------------------------------------- GEMM

@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("name", list(GEMM_TABLE))
def test_gemm_emulation_within_bound(name, cls):
    c, inp, orc, peak = _gemm_setup(name, cls)
    if cls == "exact":
        assert peak <= 256, f"exact-class precondition: max|sum| {peak}"
    lay = GB.gemm_layout(c, inp)
    A, B = GB.layout_operands(c, lay)
    # the layout holds the operands where the leading dimensions say, and
    # NaN everywhere else
    assert torch.equal(A.float(), inp["A"]) and torch.equal(B.float(),
                                                            inp["B"])
    for key, mat in (("A", inp["A"]), ("B", inp["B"])):
        assert int((~torch.isnan(lay[key].float())).sum()) == mat.numel()
    within(GB.gemm_emulate(c, inp, A, B), orc, f"{name}/{cls}")


def test_gemm_split_counts():
    """The shapes reach the split layouts their comments claim."""
    assert GB.split_k(1030, 3) == (352, 3)
    assert GB.split_k(1030, 33) == (32, 33)
    assert GB.split_k(1024, 3) == (352, 3)
    assert GB.split_k(98, 3) == (64, 2)
    assert GB.split_k(98, 4) == (32, 4)


def _rejected(table, mutant, setup, emulate):
    for name in table:
        for cls in CLASSES:
            c, inp, orc = setup(name, cls)
            if violations(emulate(c, inp, mutant), orc):
                return f"{name}/{cls}"
    return None


@pytest.mark.parametrize("mutant", GB.GEMM_MUTANTS)
def test_gemm_mutants_rejected(mutant):
    table = dict(GB.GEMM_CASES, split3_bias=GB.RAISES_CASES["split3_bias"])
    hit = _rejected(table, mutant, lambda n, k: _gemm_setup(n, k)[:3],
                    lambda c, i, m: GB.gemm_emulate(c, i, mutant=m))
    assert hit, f"no GEMM case rejects mutant {mutant}"


@pytest.mark.parametrize("mutant", GB.WIDE_MUTANTS)
def test_wide_mutants_rejected(mutant):
    hit = _rejected(GB.WIDE_CASES, mutant,
                    lambda n, k: _gemm_setup(n, k)[:3],
                    lambda c, i, m: GB.gemm_emulate(c, i, mutant=m))
    assert hit, f"no wide case rejects mutant {mutant}"


@pytest.mark.parametrize("mutant", ["drop_last_k", "truncate"])
def test_every_plain_gemm_case_rejects(mutant):
    """A dropped k element is caught by the exact class of every case (its
    product is non-zero somewhere); truncation by the rounded class of
    every bf16-output case."""
    for name, c in GB.GEMM_CASES.items():
        cls = "exact" if mutant == "drop_last_k" else "rounded"
        if mutant == "truncate" and c["store"] not in (0, 3):
            continue
        if c["M"] * c["N"] < 64:
            continue        # too few elements to be sure of a hit
        c, inp, orc, _ = _gemm_setup(name, cls)
        assert violations(GB.gemm_emulate(c, inp, mutant=mutant), orc), \
            f"{name}/{cls} accepts mutant {mutant}"


# -------------------------------------------------------------- convolution

CONV_TABLE = dict(GB.CONV_CASES, **{"direct_" + k: v for k, v in
                                    GB.FWD_DIRECT_CASES.items()})


def _conv_setup(name, cls):
    c = CONV_TABLE[name]
    inp = GB.conv_inputs(c, cls, _seed(CONV_TABLE, name, cls))
    orc, peak = GB.conv_oracle(c, inp)
    return c, inp, orc, peak


@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("name", list(CONV_TABLE))
def test_conv_emulation_within_bound(name, cls):
    c, inp, orc, peak = _conv_setup(name, cls)
    assert GB.conv_geometry_ok(c), "geometry precondition"
    p, q = GB.conv_dims(c)
    assert c["n"] * p * q < 1024, "dw must stay a single split"
    if cls == "exact":
        assert peak <= 256, f"exact-class precondition: max|sum| {peak}"
    if c["groups"] > 1:
        cg = c["c"] // c["groups"]
        assert not torch.equal(inp["x"][:, :cg], inp["x"][:, cg:2 * cg])
    within(GB.conv_emulate(c, inp), orc, f"{name}/{cls}")


@pytest.mark.parametrize("mutant", GB.CONV_MUTANTS)
def test_conv_mutants_rejected(mutant):
    hit = _rejected(CONV_TABLE, mutant, lambda n, k: _conv_setup(n, k)[:3],
                    lambda c, i, m: GB.conv_emulate(c, i, mutant=m))
    assert hit, f"no conv case rejects mutant {mutant}"


def test_conv_gates():
    """The shapes sit where the table's comments put them."""
    def kpad(c):
        return GB.kpad_dma(c["r"] * c["s"] * c["c"] // c["groups"])

    def w8(c):
        p, q = GB.conv_dims(c)
        return c["n"] * p * q <= 256 or c["k"] // c["groups"] <= 256
    C = GB.CONV_CASES
    assert kpad(C["imp82_k64"]) == 64 and kpad(C["imp82_k96_npq98"]) == 96
    assert kpad(C["imp84_k128"]) == 128 and kpad(C["imp84_k288"]) == 288
    assert kpad(C["imp84_k1152"]) == 1152
    assert kpad(C["imp82_k1248"]) == 1248
    assert all(w8(C[n]) for n in C if n != "imp42_k264")
    assert not w8(C["imp42_k264"])
    for n in ("imp82_k96_npq98", "imp82_k96_npq288"):
        p, q = GB.conv_dims(C[n])
        assert C[n]["n"] * p * q == int(n.rsplit("npq", 1)[1])
    assert GB.conv_dims(C["imp_nonsquare_7x5"]) == (7, 5)


# ----------------------------------------------------------- column kernels

def _naive_im2col(c, x):
    p, q = GB.conv_dims(c)
    out = torch.zeros(c["n"] * p * q, c["kpad"], dtype=x.dtype)
    for n in range(c["n"]):
        for pi in range(p):
            for qi in range(q):
                row = (n * p + pi) * q + qi
                for r in range(c["r"]):
                    for s in range(c["s"]):
                        h = pi * c["stride"] - c["pad"] + r * c["dil"]
                        w = qi * c["stride"] - c["pad"] + s * c["dil"]
                        if 0 <= h < c["h"] and 0 <= w < c["w"]:
                            k = (r * c["s"] + s) * c["ct"]
                            out[row, k:k + c["ct"]] = \
                                x[n, c["c0"]:c["c0"] + c["ct"], h, w]
    return out


@pytest.mark.parametrize("name", list(GB.IM2COL_CASES))
def test_im2col_oracle(name):
    """The unfold construction equals the definition, tap by tap."""
    c = GB.IM2COL_CASES[name]
    x = GB.col_inputs(c, "rounded", 7)["x"]
    assert torch.equal(GB.im2col_want(c, x), _naive_im2col(c, x))


def test_im2col_lut_carry_rejected():
    hits = 0
    for name, c in GB.IM2COL_CASES.items():
        x = GB.col_inputs(c, "rounded", 7)["x"]
        differs = not torch.equal(GB.im2col_want(c, x),
                                  GB.im2col_want(c, x, mutant="lut_carry"))
        assert differs == (c["ct"] > 1024), name
        hits += differs
    assert hits >= 3


@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("name", list(GB.COL2IM_CASES))
def test_col2im_emulation_within_bound(name, cls):
    c = GB.COL2IM_CASES[name]
    inp = GB.col_inputs(c, cls, _seed(GB.COL2IM_CASES, name, cls))
    orc, peak = GB.col2im_oracle(c, inp)
    assert peak <= 256
    within(GB.col2im_emulate(c, inp), orc, f"{name}/{cls}")


@pytest.mark.parametrize("mutant", ["rs_swapped", "truncate"])
def test_col2im_mutants_rejected(mutant):
    def setup(n, k):
        c = GB.COL2IM_CASES[n]
        inp = GB.col_inputs(c, k, 5)
        return c, inp, GB.col2im_oracle(c, inp)[0]
    assert _rejected(GB.COL2IM_CASES, mutant, setup,
                     lambda c, i, m: GB.col2im_emulate(c, i, m))


@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("rows,cols,_gap", GB.COLSUM_CASES)
def test_colsum_emulation_within_bound(rows, cols, _gap, cls):
    inp = GB.colsum_inputs(rows, cols, cls, rows + cols)
    orc = GB.colsum_oracle(inp)
    within(GB.colsum_emulate(inp), orc, f"colsum {rows}x{cols}/{cls}")
    for mutant in ("drop_last_row", "out0_dropped"):
        if cols >= 8:
            assert violations(GB.colsum_emulate(inp, mutant), orc), mutant


@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("rows,cols", GB.BIAS_ACT_SHAPES)
def test_bias_act_emulation_within_bound(rows, cols, cls):
    inp = GB.bias_act_inputs(rows, cols, cls, rows + cols)
    for bias in (False, True):
        for relu in (False, True):
            orc = GB.bias_act_oracle(inp, bias, relu)
            within(GB.bias_act_emulate(inp, bias, relu), orc,
                   f"bias_act {rows}x{cols}/{cls}")
    if rows * cols >= 64:
        orc = GB.bias_act_oracle(inp, True, True)
        assert violations(GB.bias_act_emulate(inp, True, True,
                                              "relu_before_bias"), orc)
        if cls == "rounded":
            assert violations(GB.bias_act_emulate(inp, True, True,
                                                  "truncate"), orc)


# ----------------------------------------------------------------- Winograd

@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("name", list(GB.WINO_CASES))
def test_winograd_emulation_within_bound(name, cls, flip):
    """The emulation of exactly the kernels' four rounding points stays
    inside the derived bound; checked here, before any GPU run."""
    c = GB.WINO_CASES[name]
    inp = GB.wino_inputs(c, cls, _seed(GB.WINO_CASES, name, cls))
    orc, peak = GB.wino_oracle(c, inp, flip)
    if cls == "exact":
        assert peak <= 256, f"exact-class precondition: {peak}"
    within(GB.wino_emulate(c, inp, flip), orc, f"{name}/{cls}/flip={flip}")


def test_winograd_ragged_guard_mutant_rejected():
    for name in ("13x13_c8_k8", "13x12_c8_k16_bias_relu"):
        c = GB.WINO_CASES[name]
        for cls in CLASSES:
            inp = GB.wino_inputs(c, cls, 5)
            orc, _ = GB.wino_oracle(c, inp, False)
            assert violations(GB.wino_emulate(c, inp, False,
                                              "no_ragged_guard"), orc)
    c = GB.WINO_CASES["6x8_c8_k8"]      # no ragged tile: nothing to wrap
    inp = GB.wino_inputs(c, "exact", 5)
    orc, _ = GB.wino_oracle(c, inp, False)
    assert not violations(GB.wino_emulate(c, inp, False, "no_ragged_guard"),
                          orc)
