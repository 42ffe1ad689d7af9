"""CPU check of the bounds in _fused_bwd_cases.py: each oracle bound passes
a faithful emulation of its kernel (including the two-level db sum in a
shuffled block order) and fails the mutants a wrong fusion would produce.
test_fused_bwd_gpu.py asserts the same bounds on the kernels."""

import pytest
import torch

import _bf16_bounds as B
import _fused_bwd_cases as F


@pytest.mark.parametrize("slope", F.RELU_DB_SLOPES)
@pytest.mark.parametrize("shape", F.RELU_DB_SHAPES,
                         ids=lambda s: f"{s[0]}x{s[1]}")
def test_relu_db_bound(shape, slope):
    inp = F.relu_db_inputs(*shape, 900 + shape[0])
    orc = F.relu_db_oracle(inp, slope)
    for nb in F.FORCED_BLOCKS + (7,):
        B.assert_within(F.relu_db_emulate(inp, slope, nb, seed=nb), orc,
                        f"relu+db {shape} slope={slope} blocks={nb}")
    for name, mut in F.RELU_DB_MUTANTS.items():
        assert B.violations(mut(inp, slope), orc), \
            f"bound too loose for mutant {name} at {shape} slope={slope}"


@pytest.mark.parametrize("case", F.POOL_CASES, ids=F.case_id)
def test_pool_relu_db_bound(case):
    c, geom = case
    inp = F.pool_relu_inputs(c, geom, 940 + c)
    zero_win, multi = F.pool_data_facts(inp)
    # without these the mask and the multi-window sum are not exercised
    assert zero_win >= 1, "no window with maximum 0 and a non-zero dy"
    k, s = geom[2], geom[3]
    if s[0] < k[0]:                     # windows overlap
        assert multi >= 1, "no pixel is the argmax of two windows"
    orc = F.pool_relu_oracle(inp)
    for nb in F.FORCED_BLOCKS + (7,):
        B.assert_within(F.pool_relu_emulate(inp, nb, seed=nb), orc,
                        f"pool+relu+db {F.case_id(case)} blocks={nb}")
    for name, mut in F.POOL_RELU_MUTANTS.items():
        assert B.violations(mut(inp), orc), \
            f"bound too loose for mutant {name} at {F.case_id(case)}"


def test_pool_data_hold_multi_window_pixels():
    """Over the cases as a whole: at least one pixel is the argmax of two
    or more windows (only the overlapping geometries can hold one)."""
    total = sum(F.pool_data_facts(F.pool_relu_inputs(c, g, 940 + c))[1]
                for c, g in F.POOL_CASES)
    assert total >= 1


def test_emulation_equals_unfused_pair():
    """The fused arithmetic gives bit-identical dx to max-pool backward
    followed by ReLU backward (slope 0): the property the GPU test checks
    with torch.equal."""
    for c, geom in F.POOL_CASES:
        inp = F.pool_relu_inputs(c, geom, 940 + c)
        plain = B.maxpool_emulate(inp)["dx"].float()
        pair = B.bf16(plain * (inp["x"].float() > 0).float())
        assert torch.equal(F.pool_relu_emulate(inp)["dx"], pair)


def test_uncovered_pixels():
    inp = F.pool_relu_inputs(8, F.POOL_GEOMS[2], 948)
    unc = F.uncovered(inp)
    assert unc.any()                    # stride 3 > kernel 2
    dx = F.pool_relu_emulate(inp)["dx"]
    assert not dx[:, :, unc].any()
