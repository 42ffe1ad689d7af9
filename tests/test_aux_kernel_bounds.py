"""The bounds of _bf16_bounds.py can pass and can fail, shown without a GPU.

For every op and every case of test_gpu_aux_kernels.py a CPU emulation of the
kernel (fp32 arithmetic, bf16 where the kernel rounds) stays inside the
bound, and every mutant of that op leaves it on at least one case.  The GPU
file asserts the same bounds on the real kernels."""

import pytest
import torch

import _bf16_bounds as B


def _sweep(cases, oracle, emulate, mutants, what):
    """Emulation inside the bound on every case; returns, per mutant, the
    cases on which it was caught."""
    caught = {name: [] for name in mutants}
    for label, inp in cases:
        orc = oracle(inp)
        B.assert_within(emulate(inp), orc, f"{what} {label} emulation")
        for name, fn in mutants.items():
            if B.violations(fn(inp), orc):
                caught[name].append(label)
    for name, where in caught.items():
        print(f"{what} mutant {name}: caught on {len(where)}/{len(cases)}")
        assert where, f"{what}: mutant {name} survives every case"
    return caught


def test_pool_out_clamp_and_ceil():
    assert B.pool_out(12, 3, 2, 0) == 6 and B.pool_out(12, 3, 2, 0, True) == 5
    assert B.pool_out(5, 2, 2, 1) == 3          # clamp: 4 -> 3
    assert B.pool_out(112, 3, 2, 0) == 56       # GoogLeNet 112 -> 56
    assert B.pool_out(11, 2, 3, 0) == 4


def test_maxpool():
    cases = [(f"C{c} {g}", B.pool_inputs(c, g, 200 + i, ties=True))
             for i, (c, g) in enumerate(B.MAXPOOL_CASES)]
    caught = _sweep(cases, B.maxpool_oracle, B.maxpool_emulate,
                    B.MAXPOOL_MUTANTS, "maxpool")
    # ties are everywhere, so the tie rule is pinned on every geometry
    assert len(caught["tie_last"]) == len(cases)


def test_maxpool_oracle_matches_torch_where_no_ties():
    """Without ties the argmax is unique: the unfold oracle must agree
    with torch's own ceil-mode max pooling on values."""
    for i, (c, g) in enumerate(B.MAXPOOL_CASES):
        inp = B.pool_inputs(c, g, 300 + i, ties=False)
        _, _, k, s, p = g
        want = torch.nn.functional.max_pool2d(
            inp["x"].float(), k, s, p, ceil_mode=True)
        got = B.maxpool_oracle(inp)["y"][0]
        assert torch.equal(got.float(), want), g


def test_maxpool_stride_gt_kernel_leaves_zeros():
    inp = B.pool_inputs(16, B.POOL_GEOMS[4], 7, ties=True)
    dx = B.maxpool_oracle(inp)["dx"][0]
    assert torch.equal(dx[:, :, 2::3, :], torch.zeros_like(dx[:, :, 2::3, :]))
    assert torch.equal(dx[:, :, :, 2::3], torch.zeros_like(dx[:, :, :, 2::3]))


def test_avgpool():
    cases = [(f"C{c} {g}", B.pool_inputs(c, g, 400 + i, ties=False))
             for i, (c, g) in enumerate(B.AVGPOOL_CASES)]
    cases += [(f"global C{c}", B.global_avg_inputs(c, h, w, 450 + i))
              for i, (c, h, w) in enumerate(B.GLOBAL_AVG_CASES)]
    _sweep(cases, B.avgpool_oracle, B.avgpool_emulate, B.AVGPOOL_MUTANTS,
           "avgpool")


def test_avgpool_oracle_matches_reference():
    from caffeonspark_amd.ops import reference
    for i, (c, g) in enumerate(B.AVGPOOL_CASES):
        inp = B.pool_inputs(c, g, 400 + i, ties=False)
        _, _, k, s, p = g
        x, dy = inp["x"].double(), inp["dy"].double()
        orc = B.avgpool_oracle(inp)
        torch.testing.assert_close(
            orc["y"][0], reference.avgpool_forward(x, k, s, p),
            rtol=1e-12, atol=1e-12)
        torch.testing.assert_close(
            orc["dx"][0], reference.avgpool_backward(x, k, s, p, dy),
            rtol=1e-12, atol=1e-12)


def test_lrn():
    cases = [(str(c), B.lrn_inputs(c, 500 + i))
             for i, c in enumerate(B.LRN_CASES)]
    caught = _sweep(cases, B.lrn_oracle, B.lrn_emulate, B.LRN_MUTANTS, "lrn")
    # the window matters on every case, AlexNet's parameters included
    for name in ("radius_minus_1", "identity", "no_second_term"):
        assert len(caught[name]) == len(cases), (name, caught[name])


def test_lrn_oracle_matches_reference():
    from caffeonspark_amd.ops import reference
    for i, c in enumerate(B.LRN_CASES):
        inp = B.lrn_inputs(c, 500 + i)
        x, dy = inp["x"].double(), inp["dy"].double()
        args = (inp["local_size"], inp["alpha"], inp["beta"])
        orc = B.lrn_oracle(inp)
        # the project's reference computes LRN in fp32 whatever it is given
        y, scale = reference.lrn_forward(x, *args, inp["k"])
        kw = dict(rtol=1e-5, atol=1e-5, check_dtype=False)
        torch.testing.assert_close(orc["y"][0], y, **kw)
        torch.testing.assert_close(orc["scale"][0], scale, **kw)
        dx = reference.lrn_backward(x, y, scale, dy, *args)
        torch.testing.assert_close(orc["dx"][0], dx, **kw)


def test_softmax_loss():
    cases = list(B.softmax_cases().items())
    caught = _sweep(cases, B.softmax_oracle, B.softmax_emulate,
                    B.SOFTMAX_MUTANTS, "softmax")
    assert "special_4x65" in caught["no_max_subtraction"]
    assert {"ignore_32x11", "ignore_axis2_3x4x11",
            "ignore_axis1_2x5x3x2"} <= set(caught["no_ignore"])


def test_softmax_ignored_rows_are_zero():
    inp = B.softmax_cases()["ignore_axis2_3x4x11"]
    dx, tol = B.softmax_oracle(inp)["dx"]
    ign = inp["label"] == -1
    assert ign.any() and not ign.all()
    assert torch.equal(dx[ign], torch.zeros_like(dx[ign]))
    assert torch.equal(tol[ign], torch.zeros_like(tol[ign]))


def test_batchnorm():
    caught = []
    for i, case in enumerate(B.BN_CASES):
        inp = B.bn_inputs(case, 600 + i)
        what = f"bn {case[0]}"
        emu = B.bn_train_emulate(inp)
        B.assert_within(emu, B.bn_train_oracle(inp), what + " train")
        B.assert_within(B.bn_infer_emulate(inp), B.bn_infer_oracle(inp),
                        what + " infer")
        xhat, inv = emu["y"], emu["invstd"]
        for train in (True, False):
            orc = B.bn_backward_oracle(xhat, inp["dy"], inv, train)
            B.assert_within(
                B.bn_backward_emulate(xhat, inp["dy"], inv, train), orc,
                f"{what} backward train={train}")
            if train and B.violations(
                    B.BN_BACKWARD_MUTANTS["no_s2_term"](xhat, inp["dy"],
                                                        inv), orc):
                caught.append(case[0])
    assert len(caught) == len(B.BN_CASES), caught


def test_batchnorm_shifted_bound_is_not_slack():
    """On the shifted case (mean^2 is 250x var) the absolute-term bound on
    var is still below 1 % of var and the one on y below 3u."""
    inp = B.bn_inputs(B.BN_CASES[4], 604)
    orc = B.bn_train_oracle(inp)
    var, tol = orc["var"]
    assert (tol < 0.01 * var).all()
    y, tol_y = orc["y"]
    assert (tol_y <= 3 * B.U * y.abs() + 1e-3).all()


@pytest.mark.parametrize("slope", B.RELU_SLOPES)
def test_relu(slope):
    for i, n in enumerate(B.RELU_SIZES):
        inp = B.relu_inputs(n, 700 + i)
        orc = B.relu_oracle(inp, slope)
        assert (orc["y"][1] is None) == (slope == 0.25)
        B.assert_within(B.relu_emulate(inp, slope), orc, f"relu n={n}")
        wrong = {"y": B.bf16(inp["x"].float().clamp_min(0))}
        assert B.violations(wrong, orc)          # slope dropped


def test_relu_fused():
    for c in (8, 12):
        inp = B.relu_window_inputs(c, 710 + c)
        sl = slice(inp["off"], inp["off"] + c)
        y, dy = inp["ybuf"][:, sl], inp["dybuf"][:, sl]
        assert y.stride(1) == 1 and y.stride(3) == 24
        orc = B.relu_fused_oracle(y, dy, inp["db0"], 0.25)
        B.assert_within(B.relu_fused_emulate(y, dy, inp["db0"], 0.25), orc,
                        f"relu window C={c}")
        overwrite = B.relu_fused_emulate(y, dy, torch.zeros(c), 0.25)
        assert B.violations(overwrite, orc)      # db not accumulated into


def test_embed():
    inp = B.embed_inputs(800)
    idx = inp["idx"].long()
    assert idx.min() == 0 and idx.max() == B.EMBED_V - 1
    B.assert_within(B.embed_emulate(inp), B.embed_oracle(inp), "embed")


def test_lstm_unit():
    inp = B.lstm_inputs(900)
    orc = B.lstm_oracle(inp)
    B.assert_within(B.lstm_emulate(inp), orc, "lstm")
    act = orc["act"][0]                 # both saturations are reached
    assert (act[:, :3] > 0.999).any() and (act[:, :3] < 0.001).any()
    wrong = B.lstm_emulate(inp)         # gate order (i, f, o, g) is pinned
    wrong["dgates"] = wrong["dgates"].reshape(12, 4, 20)[:, [1, 0, 2, 3]] \
        .reshape(12, 80)
    assert B.violations(wrong, orc)


def test_sgd():
    for i, n in enumerate(B.SGD_SIZES):
        inp = B.sgd_inputs(n, 950 + i)
        B.assert_within(B.sgd_emulate(inp), B.sgd_oracle(inp), f"sgd n={n}")
