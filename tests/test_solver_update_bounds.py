"""CPU check of the bounds in _solver_update_cases.py: on every layout and
for every solver type a faithful fp32 emulation of the update stays inside
the float64 bound, each mutant leaves it on the layouts built to show it,
the oracles are the formulas of ops/reference.py, and the bounds are a
small multiple of the fp32 roundoff.  test_solver_update_gpu.py asserts the
same bounds on the kernels."""

import pytest
import torch

import _bf16_bounds as B
import _solver_update_cases as S
from caffeonspark_amd.ops import reference


@pytest.mark.parametrize("solver", S.SOLVERS)
@pytest.mark.parametrize("layout", list(S.LAYOUTS))
def test_emulation_within_bound(layout, solver):
    case = S.make_case(layout, solver)
    out = S.emulate(case)
    what = f"{solver} {layout}"
    state = {n: t for n, t in out.items() if n != "sh"}
    B.assert_within(state, S.oracle(case), what)
    B.assert_within({"sh": out["sh"]}, S.shadow_expect(case, out["p"]), what)
    assert not S.missed_elements(case, out)
    frozen = ~S.trainable(case)
    for name in state:
        assert torch.equal(out[name][frozen], case[name][frozen])
    assert (out["sh"][frozen].float() == S.SENTINEL).all()


def test_inputs_hold_the_special_elements():
    """Non-zero momentum, a non-negative second moment, and elements with
    g == 0 and v == 0 in trainable segments (for Adam a division whose
    denominator is eps, or nearly)."""
    for layout in ("straddle", "lenet", "grid_stride"):
        case = S.make_case(layout, "adam")
        assert (case["v"] >= 0).all() and case["m"].abs().min() > 0
        special = (case["g"] == 0) & (case["v"] == 0) & S.trainable(case)
        assert special.sum() >= 2
        sgd = S.make_case(layout, "sgd")
        assert (sgd["v"] != 0).sum() >= sgd["n"] - sgd["n"] // 7 - 1


# layouts on which a mutant must be caught, beyond "somewhere"
MUST_CATCH = {
    "quad_owner": S.QUAD_OWNER_CAUGHT,
    "neighbour_params": ("straddle",),
    "frozen_touched": ("straddle", "frozen_edges"),
    "no_decay": ("aligned",),
    "decay_after_lr": ("aligned",),
    "stale_shadow": ("aligned", "single3"),
    "last_table_entry_dropped": ("table_full",),
    "plain_momentum": ("aligned",),
    "eps_inside_sqrt": ("straddle",),
    "unfolded_correction": ("aligned",),
}


@pytest.mark.parametrize("solver", S.SOLVERS)
def test_mutants_are_caught(solver):
    for mutant in S.MUTANTS[solver]:
        caught = []
        for layout in S.LAYOUTS:
            if layout == "grid_stride" and mutant != "quad_owner":
                continue                # the one large case: once is enough
            case = S.make_case(layout, solver)
            if S.all_violations(case, S.emulate(case, mutant)):
                caught.append(layout)
        print(f"{solver} {mutant}: caught on {caught}")
        missing = [n for n in MUST_CATCH[mutant] if n not in caught]
        assert not missing, f"{solver} {mutant} survives {missing}"
    assert set(S.MUTANTS[solver]) <= set(MUST_CATCH)


@pytest.mark.parametrize("solver", S.SOLVERS)
def test_quad_owner_survives_aligned_layouts(solver):
    """Where every boundary is on a quad the old indexing is right: the
    control that the straddle layouts, not the arithmetic, catch it."""
    for layout in ("aligned", "single1", "single3", "single4", "single5"):
        case = S.make_case(layout, solver)
        out = S.emulate(case, "quad_owner")
        assert not S.all_violations(case, out), layout
        for name, t in S.emulate(case).items():
            assert torch.equal(out[name], t)


@pytest.mark.parametrize("solver", S.SOLVERS)
def test_quad_owner_misses_on_lenet(solver):
    """The first two elements of ip1.w, ip1.b, ip2.w and ip2.b of the
    shipped LeNet never train under the quad-owner indexing."""
    case = S.make_case("lenet", solver)
    out = S.emulate(case, "quad_owner")
    assert S.missed_elements(case, out) == S.LENET_QUAD_OWNER_MISSES
    for name, (want, tol) in S.oracle(case).items():
        over = ~((out[name].double() - want).abs() <= tol)
        assert torch.nonzero(over).reshape(-1).tolist() \
            == S.LENET_QUAD_OWNER_MISSES, name
    unwritten = out["sh"] != S.emulate(case)["sh"]
    assert unwritten.nonzero().reshape(-1).tolist() \
        == S.LENET_QUAD_OWNER_MISSES
    assert (out["sh"][unwritten].float() == S.SENTINEL).all()


def test_quad_owner_misses_on_straddle():
    case = S.make_case("straddle", "sgd")
    out = S.emulate(case, "quad_owner")
    assert S.missed_elements(case, out) == [5, 6, 7, 15]


@pytest.mark.parametrize("solver", S.SOLVERS)
@pytest.mark.parametrize("layout", S.FOLLOWS_REFERENCE)
def test_oracle_is_the_reference_formula(layout, solver):
    """Segment by segment the oracle equals ops/reference.py run in
    float64 on the same fp32-rounded parameters."""
    case = S.make_case(layout, solver)
    orc = S.oracle(case)
    off = case["off"].tolist()
    mu, b1, b2, eps = (S._f32(x) for x in (S.MU, S.B1, S.B2, S.EPS))
    for s in range(len(off) - 1):
        sl = slice(off[s], off[s + 1])
        lr, wd = float(case["seg_lr"][s]), float(case["seg_wd"][s])
        p, g, v = (case[n][sl].double().clone() for n in "pgv")
        got = {"p": p, "v": v}
        if lr == 0:
            pass
        elif solver == "sgd":
            reference.sgd_update(p, g, v, lr, mu, wd)
        elif solver == "nesterov":
            reference.nesterov_update(p, g, v, lr, mu, wd)
        else:
            # the caller folds the correction into seg_lr: hand the
            # reference the unfolded rate and let it apply its own
            m = case["m"][sl].double().clone()
            got["m"] = m
            corr = S.adam_correction(S.ADAM_T, b1, b2)
            reference.adam_update(p, g, m, v, lr / corr, b1, b2, eps, wd,
                                  S.ADAM_T)
        for name, t in got.items():
            want = orc[name][0][sl]
            err = (t - want).abs().max().item() if t.numel() else 0.0
            assert err <= 1e-12 * max(1.0, want.abs().max().item()), \
                f"{name} segment {s}: {err}"


@pytest.mark.parametrize("solver", S.SOLVERS)
@pytest.mark.parametrize("layout", list(S.LAYOUTS))
def test_bound_is_not_slack(layout, solver):
    """Every bound on p' is at most 1e-6 of T (2e-6 for Adam), T being the
    magnitudes its expression handles: |p|, |v|, lr |g| and, for Adam,
    the quotient lr T_m / (sqrt(v') + eps).  The frozen elements' bound
    is 0.

    Relative to |p| + |v| alone no sound bound can hold: an element with
    p and v near 0 moves by lr g; Adam's quotient has nothing to do with
    |p| + |v| where the second moment is near 0 (at g == 0 and v == 0 the
    step is lr m / eps); and Nesterov's (1 + mu) v' - mu v handles
    2.61 |v| through 8 roundings, 1.4e-6 |v| already.  Largest tol_p / T
    over the cases: SGD 3.6e-7 (6e), Nesterov 5.4e-7 (9e), Adam 1.14e-6
    (16.5e where gg does not cancel, more where g and wd p do)."""
    case = S.make_case(layout, solver)
    tol = S.oracle(case)["p"][1]
    mag = S.magnitude(case)
    live = S.trainable(case)
    assert (tol[~live] == 0).all()
    ratio = (tol[live] / mag[live].clamp_min(1e-300)).max().item()
    print(f"{solver} {layout}: max tol_p / T = {ratio:.3e}")
    limit = 2e-6 if solver == "adam" else 1e-6
    assert (tol[live] <= limit * mag[live] + 1e-30).all()
    assert limit < B.U / 1000           # far below a bf16-level mistake
    if solver == "sgd":
        # against |p| + |v| alone wherever the gradient's own step is no
        # larger than that
        pv = case["p"].double().abs() + case["v"].double().abs()
        seg = S.owner(case["off"], case["n"])
        step = case["seg_lr"].double()[seg] * case["g"].double().abs()
        sel = live & (step <= pv)
        assert sel.sum() > 0.9 * live.sum() - 2
        assert (tol[sel] <= 1e-6 * pv[sel] + 1e-30).all()
