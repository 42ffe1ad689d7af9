"""The non-GEMM bf16 HIP kernels against float64 oracles with derived bounds.

Oracles, bounds and their derivation live in _bf16_bounds.py;
test_aux_kernel_bounds.py shows on the CPU that each bound passes a faithful
emulation of the kernel and fails its mutants.  Here the same bounds are
asserted on the kernels themselves, at the shapes where they change path:
8-wide and scalar pooling, int8 and int32 argmax, ceil overhang and pad
clamp, LRN window edges and beta specialisations, softmax rows around the
wave width, BatchNorm block shapes, strided and fused ReLU backward."""

import math

import pytest
import torch

import _bf16_bounds as B

pytestmark = pytest.mark.gpu

from caffeonspark_amd import ops
from caffeonspark_amd.ops import gpu as G


def dev():
    return torch.device("cuda:0")


def d(t):
    return t.to(dev())


# ---------------------------------------------------------------- pooling

@pytest.mark.parametrize("case", list(enumerate(B.MAXPOOL_CASES)),
                         ids=lambda c: f"C{c[1][0]}-{c[1][1]}")
def test_maxpool(case):
    i, (c, geom) = case
    inp = B.pool_inputs(c, geom, 200 + i, ties=True)
    k, s, p = inp["kernel"], inp["stride"], inp["pad"]
    x = d(inp["x"])
    y, pack = ops.maxpool_forward(x, k, s, p)
    want_idx = torch.int8 if k[0] * k[1] < 128 else torch.int32
    assert pack[0].dtype == want_idx
    dx = ops.maxpool_backward(list(x.shape), pack, d(inp["dy"]))
    B.assert_within({"y": y, "dx": dx}, B.maxpool_oracle(inp),
                    f"maxpool C{c} {geom}")
    if s[0] > k[0]:     # pixels no window covers get exactly zero
        assert not dx[:, :, k[0]::s[0], :].any()
        assert not dx[:, :, :, k[1]::s[1]].any()


@pytest.mark.parametrize("case", list(enumerate(B.AVGPOOL_CASES)),
                         ids=lambda c: f"C{c[1][0]}-{c[1][1]}")
def test_avgpool(case):
    i, (c, geom) = case
    inp = B.pool_inputs(c, geom, 400 + i, ties=False)
    k, s, p = inp["kernel"], inp["stride"], inp["pad"]
    x = d(inp["x"])
    y = ops.avgpool_forward(x, k, s, p)
    dx = ops.avgpool_backward(x, k, s, p, d(inp["dy"]))
    B.assert_within({"y": y, "dx": dx}, B.avgpool_oracle(inp),
                    f"avgpool C{c} {geom}")


@pytest.mark.parametrize("case", list(enumerate(B.GLOBAL_AVG_CASES)),
                         ids=lambda c: f"C{c[1][0]}")
def test_global_avgpool(case):
    i, (c, h, w) = case
    inp = B.global_avg_inputs(c, h, w, 450 + i)
    x = d(inp["x"])
    y = ops.global_avgpool_forward(x)
    dx = ops.global_avgpool_backward(list(x.shape), d(inp["dy"]))
    B.assert_within({"y": y, "dx": dx}, B.avgpool_oracle(inp),
                    f"global avgpool C{c}")


# -------------------------------------------------------------------- LRN

@pytest.mark.parametrize("case", list(enumerate(B.LRN_CASES)),
                         ids=lambda c: "C%d-n%d-a%g-b%g" % c[1][:4])
def test_lrn(case):
    i, params = case
    inp = B.lrn_inputs(params, 500 + i)
    args = (inp["local_size"], inp["alpha"], inp["beta"])
    x = d(inp["x"])
    y, pack = ops.lrn_forward(x, *args, inp["k"])
    dx = ops.lrn_backward(x, y, pack, d(inp["dy"]), *args)
    scale = pack[0].permute(0, 3, 1, 2)          # stored NHWC
    B.assert_within({"y": y, "scale": scale, "dx": dx}, B.lrn_oracle(inp),
                    f"lrn {params}")


def test_lrn_fallback_contract():
    """C % 8 != 0 runs the torch fallback: (y, pack) comes back and the
    backward accepts that pack."""
    inp = B.lrn_inputs((12, 5, 1.0, 0.75, 1.0, 1.0), 520)
    orc = B.lrn_oracle(inp)
    x = d(inp["x"])
    y, pack = ops.lrn_forward(x, 5, 1.0, 0.75, 1.0)
    assert y.dtype == torch.bfloat16 and y.shape == x.shape
    torch.testing.assert_close(y.double().cpu(), orc["y"][0], rtol=0.02,
                               atol=0.02)
    dx = ops.lrn_backward(x, y, pack, d(inp["dy"]), 5, 1.0, 0.75)
    assert dx.dtype == torch.bfloat16 and dx.shape == x.shape
    torch.testing.assert_close(dx.double().cpu(), orc["dx"][0], rtol=0.03,
                               atol=0.03)


# ----------------------------------------------------------- softmax loss

_SOFTMAX = B.softmax_cases()


@pytest.mark.parametrize("name", list(_SOFTMAX))
def test_softmax_loss(name):
    inp = _SOFTMAX[name]
    ig, axis = inp["ignore_label"], inp["axis"]
    x, lab = d(inp["x"]), d(inp["label"])
    loss, pack, cnt = ops.softmax_loss_forward(x, lab, ig, axis)
    dx = ops.softmax_loss_backward(pack, lab, ig, 1.0 / cnt, axis)
    assert dx.shape == x.shape and dx.dtype == torch.bfloat16
    B.assert_within({"loss": loss, "count": cnt, "prob": pack[0], "dx": dx},
                    B.softmax_oracle(inp), f"softmax {name}")
    if ig is not None:
        ign = (inp["label"] == ig).unsqueeze(axis).expand(x.shape)
        assert ign.any() and not dx.cpu()[ign].any()


# -------------------------------------------------------------- batchnorm

@pytest.mark.parametrize("case", list(enumerate(B.BN_CASES)),
                         ids=lambda c: "x".join(map(str, c[1][0]))
                         + ("-shifted" if c[1][1] else ""))
def test_batchnorm(case):
    i, params = case
    inp = B.bn_inputs(params, 600 + i)
    what = f"bn {params[0]}"
    x, dy = d(inp["x"]), d(inp["dy"])
    y, mean, var, invstd = G.bn_forward_train(x, inp["eps"])
    B.assert_within({"y": y, "mean": mean, "var": var, "invstd": invstd},
                    B.bn_train_oracle(inp), what + " train")
    G.begin_backward()
    dx = G.bn_backward(y, dy, invstd, train=True)
    B.assert_within({"dx": dx}, B.bn_backward_oracle(
        y.cpu(), inp["dy"], invstd.cpu(), True), what + " train backward")

    y2, inv2 = G.bn_forward_infer(x, d(inp["gmean"]), d(inp["gvar"]),
                                  inp["eps"])
    B.assert_within({"y": y2, "invstd": inv2}, B.bn_infer_oracle(inp),
                    what + " infer")
    G.begin_backward()
    dx2 = G.bn_backward(y2, dy, inv2, train=False)
    B.assert_within({"dx": dx2}, B.bn_backward_oracle(
        y2.cpu(), inp["dy"], inv2.cpu(), False), what + " infer backward")


# ------------------------------------------------------------------- ReLU

@pytest.mark.parametrize("slope", B.RELU_SLOPES)
@pytest.mark.parametrize("n", B.RELU_SIZES)
def test_relu(n, slope):
    inp = B.relu_inputs(n, 700 + B.RELU_SIZES.index(n))
    y = ops.relu_forward(d(inp["x"]), slope)
    dx = ops.relu_backward(y, d(inp["dy"]), slope)
    B.assert_within({"y": y, "dx": dx}, B.relu_oracle(inp, slope),
                    f"relu n={n} slope={slope}")


@pytest.mark.parametrize("fused", [False, True], ids=["plain", "db_out"])
@pytest.mark.parametrize("c", [8, 12], ids=["vector", "scalar"])
def test_relu_backward_channel_window(c, fused):
    inp = B.relu_window_inputs(c, 710 + c)
    sl = slice(inp["off"], inp["off"] + c)
    y, dy = d(inp["ybuf"])[:, sl], d(inp["dybuf"])[:, sl]
    assert y.stride(1) == 1 and y.stride(3) == 24 and dy.stride(3) == 24
    orc = B.relu_fused_oracle(inp["ybuf"][:, sl], inp["dybuf"][:, sl],
                              inp["db0"], 0.25)
    if fused:
        db = d(inp["db0"]).clone()
        dx, done = ops.relu_backward(y, dy, 0.25, db_out=db)
        assert done is True
        out = {"dx": dx, "db": db}
    else:
        out = {"dx": ops.relu_backward(y, dy, 0.25)}
    B.assert_within(out, orc, f"relu window C={c} fused={fused}")


def test_relu_backward_fused_2d():
    g = B.gen(730)
    y = B.bf16(torch.randn(37, 20, generator=g))
    dy = B.bf16(torch.randn(37, 20, generator=g))
    db0 = torch.randn(20, generator=g) * 3 + 1
    db = d(db0).clone()
    dx, done = ops.relu_backward(d(y), d(dy), 0.25, db_out=db)
    assert done is True
    B.assert_within({"dx": dx, "db": db},
                    B.relu_fused_oracle(y, dy, db0, 0.25), "relu fused 2-D")


# ---------------------------------------------------------------- dropout

def test_dropout():
    n, ratio = 100000, 0.4
    keep = 1.0 - ratio
    seed = G._dropout_seed(dev())
    seed.fill_(0x5EED5EED)       # in place: the address may be captured
    x = d(B.bf16(torch.randn(n, generator=B.gen(750))))
    y, mask = ops.dropout_forward(x, ratio)
    y2, mask2 = ops.dropout_forward(x, ratio)
    x, y, mask, mask2 = x.cpu(), y.cpu(), mask.cpu(), mask2.cpu()

    assert torch.equal(y, x * mask)              # bf16 product, bit-exact
    on = B.bf16(torch.tensor(1.0 / keep))
    kept = mask == on
    assert torch.equal(mask, torch.where(kept, on, torch.zeros_like(on)))

    def near(frac, p, count, what):
        sigma = math.sqrt(p * (1 - p) / count)
        print(f"dropout {what}: {frac:.5f} vs {p} (4 sigma {4 * sigma:.5f})")
        assert abs(frac - p) <= 4 * sigma, what

    near(kept.float().mean().item(), keep, n, "keep fraction")
    for j, chunk in enumerate(kept.reshape(10, -1)):
        near(chunk.float().mean().item(), keep, chunk.numel(), f"chunk {j}")
    assert not torch.equal(mask, mask2)
    agree = ((mask2 == on) == kept).float().mean().item()
    near(agree, keep * keep + ratio * ratio, n, "agreement of two draws")


# ------------------------------------------------------------------ embed

def test_embed():
    inp = B.embed_inputs(800)
    idx = d(inp["idx"])
    # bf16 weights: with fp32-only arguments the dispatch would take the
    # declared-fp32 route, which is torch indexing and not the kernel
    y = ops.embed_forward(idx, d(B.bf16(inp["w"])))
    G.begin_backward()
    dw, db = ops.embed_backward(idx, d(inp["dy"]), B.EMBED_V)
    B.assert_within({"y": y, "dw": dw, "db": db}, B.embed_oracle(inp),
                    "embed")


# -------------------------------------------------------------- LSTM unit

def test_lstm_unit():
    inp = B.lstm_inputs(900)
    c_prev = d(inp["c_prev"])
    c, h, cache = ops.lstm_unit_forward(c_prev, d(inp["gates"]),
                                        d(inp["cont"]))
    dc_prev, dgates = ops.lstm_unit_backward(c_prev, cache,
                                             d(inp["dc_next"]), d(inp["dh"]))
    assert c.dtype == torch.float32 and h.dtype == torch.bfloat16
    assert dc_prev.dtype == torch.float32 and dgates.dtype == torch.bfloat16
    B.assert_within({"c": c, "h": h, "act": cache[2], "dc_prev": dc_prev,
                     "dgates": dgates}, B.lstm_oracle(inp), "lstm unit")


# -------------------------------------------------------------------- SGD

@pytest.mark.parametrize("n", B.SGD_SIZES)
def test_sgd_update(n):
    inp = B.sgd_inputs(n, 950 + B.SGD_SIZES.index(n))
    p, g, v = d(inp["p"]).clone(), d(inp["g"]), d(inp["v"]).clone()
    ops.sgd_update(p, g, v, *B.SGD_HYPER)
    B.assert_within({"p": p, "v": v}, B.sgd_oracle(inp), f"sgd n={n}")
