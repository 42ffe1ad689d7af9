"""Deconvolution on the CPU: the depth-to-space weight map and route
algebra in float64, the reference ops against autograd, the layer, and a
small net that trains and round-trips through its snapshots."""

import os

import pytest
import torch
import torch.nn.functional as F

import _deconv_cases as dc
from test_layers import make_layer, run_grad_check

from caffeonspark_amd import ops
from caffeonspark_amd.core import Solver
from caffeonspark_amd.core.blob import Blob
from caffeonspark_amd.ops import reference as ref
from caffeonspark_amd.proto import caffe_pb, read_binary_proto, text_format


# ------------------------------------------------------------- weight map

@pytest.mark.parametrize("Ci,Co,R,S,st", [
    (8, 8, 4, 4, 2),
    (16, 6, 5, 3, 2),      # phantom taps, non-square
    (8, 8, 7, 7, 3),
    (8, 4, 2, 2, 2),       # R' = 1, K padded to 64
])
def test_weight_map_matches_definition(Ci, Co, R, S, st):
    g = torch.Generator().manual_seed(R * 10 + S)
    wd = torch.randn(Ci, Co, R, S, generator=g, dtype=torch.float64)
    Rp, Sp, kcol, kpad = dc.d2s_dims(R, S, st, Ci)
    assert kpad >= 64 and kpad % 32 == 0 and kpad >= kcol
    rows = dc.pad128(st * st * Co)
    got = dc.pack_weight(wd, st, rows, kpad)
    want = dc.pack_weight_brute(wd, st)
    assert torch.equal(got[:st * st * Co, :kcol], want)
    assert not got[st * st * Co:].any(), "pad rows must be zero"
    assert not got[:, kcol:].any(), "pad columns must be zero"
    # every real tap appears exactly once, phantom taps are zero
    assert int((want != 0).sum()) == wd.numel()


# ---------------------------------------------------------- route algebra

@pytest.mark.parametrize("N,Ci,Co,H,W,R,S,st,ph,pw", [
    (2, 8, 8, 5, 7, 4, 4, 2, 1, 1),
    (1, 8, 6, 4, 3, 5, 3, 2, 0, 1),
    (2, 3, 4, 3, 5, 7, 7, 3, 2, 0),
    (1, 8, 2, 6, 6, 2, 2, 2, 0, 0),
    (1, 4, 4, 3, 3, 16, 16, 8, 4, 4),
])
def test_route_algebra_float64(N, Ci, Co, H, W, R, S, st, ph, pw):
    g = torch.Generator().manual_seed(H * 100 + W)
    x = torch.randn(N, Ci, H, W, generator=g, dtype=torch.float64)
    wd = torch.randn(Ci, Co, R, S, generator=g, dtype=torch.float64)
    b = torch.randn(Co, generator=g, dtype=torch.float64)
    want = F.conv_transpose2d(x, wd, b, stride=st, padding=(ph, pw))
    got = dc.d2s_route(x, wd, b, st, ph, pw)
    assert got.shape == want.shape
    err = (got - want).abs().max().item()
    print(f"max |d2s route - conv_transpose2d| = {err:.3e}")
    assert err <= 1e-12 * max(1.0, want.abs().max().item())


# ---------------------------------------------------------- reference ops

@pytest.mark.parametrize("kw", [
    dict(stride=(2, 2), pad=(1, 1), dilation=(1, 1), groups=1),
    dict(stride=(2, 2), pad=(1, 0), dilation=(1, 1), groups=2),
    dict(stride=(2, 2), pad=(1, 1), dilation=(2, 2), groups=1),
    dict(stride=(2, 3), pad=(0, 1), dilation=(1, 1), groups=1),
    dict(stride=(1, 1), pad=(1, 1), dilation=(1, 1), groups=4),
])
def test_reference_backward_matches_autograd(kw):
    g = torch.Generator().manual_seed(3)
    G = kw["groups"]
    x = torch.randn(2, 4, 5, 6, generator=g, dtype=torch.float64,
                    requires_grad=True)
    w = torch.randn(4, 8 // G, 3, 4, generator=g, dtype=torch.float64,
                    requires_grad=True)
    b = torch.randn(8, generator=g, dtype=torch.float64, requires_grad=True)
    y = F.conv_transpose2d(x, w, b, stride=kw["stride"], padding=kw["pad"],
                           dilation=kw["dilation"], groups=G)
    y_op = ref.deconv2d_forward(x, w, b, **kw)
    assert torch.equal(y_op, y)
    assert torch.equal(ref.deconv2d_forward(x, w, b, relu=True, **kw),
                       F.relu(y))
    dy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    gx, gw, gb = torch.autograd.grad(y, (x, w, b), dy)
    dw_out = torch.empty_like(w)
    dx, dw, db = ref.deconv2d_backward(x.detach(), w.detach(), dy,
                                       dw_out=dw_out, **kw)
    assert dw is dw_out
    for name, a, o in (("dx", gx, dx), ("dw", gw, dw), ("db", gb, db)):
        assert o.shape == a.shape, name
        assert (o - a).abs().max().item() <= 1e-12 * max(
            1.0, a.abs().max().item()), name
    dx, dw, db = ref.deconv2d_backward(x.detach(), w.detach(), dy,
                                       need_dx=False, need_dw=False,
                                       bias=False, **kw)
    assert dx is None and dw is None and db is None


def _fp32_emulation(inp, relu, route):
    """What a correct kernel may return at worst: fp32 arithmetic, rounded
    to bf16 where the route rounds."""
    x, w = inp["x"].float(), inp["w"].float()
    kw = dict(stride=inp["stride"], padding=inp["pad"],
              dilation=inp["dilation"], groups=inp["groups"])
    if route == "d2s":
        y = F.conv_transpose2d(x, w, inp["b"], **kw).to(dc.BF)
    else:
        y = F.conv_transpose2d(x, w, None, **kw).to(dc.BF)
        if inp["b"] is not None:
            y = y + inp["b"].to(dc.BF).reshape(1, -1, 1, 1)
    return F.relu(y) if relu else y


@pytest.mark.parametrize("relu", [False, True])
def test_float64_oracle_sits_inside_its_bounds(relu):
    """The bounds the GPU tests use are wide enough for correct fp32
    arithmetic with margin, and narrow enough to catch a dropped tap."""
    cases = [(dc.make_inputs(*c, seed=len(n)), "d2s")
             for n, c in dc.D2S_CASES.items()]
    cases += [(dc.make_inputs(seed=len(n), **c), "col2im")
              for n, c in dc.FALLBACK_CASES.items()]
    for inp, route in cases:
        want, tol = dc.forward_oracle(inp, relu, route)
        got = _fp32_emulation(inp, relu, route).double()
        used = ((got - want).abs() / tol.clamp_min(1e-300)).max().item()
        assert used < 1.0, (route, used)
        # a mutant without the last kernel row is far outside
        mut = dict(inp, w=inp["w"].clone())
        mut["w"][:, :, -1] = 0
        bad = _fp32_emulation(mut, relu, route).double()
        if not relu:
            assert ((bad - want).abs() > tol).any()
        orc = dc.backward_oracle(inp)
        dx, dw, db = ref.deconv2d_backward(
            inp["x"].float(), inp["w"].float(), inp["dy"].float(),
            inp["stride"], inp["pad"], inp["dilation"], inp["groups"])
        for name, g in (("dx", dx.to(dc.BF)), ("dw", dw), ("db", db)):
            w_, t_ = orc[name]
            used = ((g.double() - w_).abs() / t_.clamp_min(1e-300)).max()
            assert used.item() < 1.0, (name, used.item())


def test_ops_registered_on_fp32_reference_route():
    assert {"deconv2d_forward", "deconv2d_backward"} <= ops._FP32_REF_ON_GPU
    x = torch.randn(1, 2, 3, 3)
    w = torch.randn(2, 3, 2, 2)
    y = ops.deconv2d_forward(x, w, None, (2, 2), (0, 0), (1, 1), 1)
    assert torch.equal(y, F.conv_transpose2d(x, w, stride=2))


# ------------------------------------------------------------------ layer

def _setup(layer, x):
    b = Blob(x.shape)
    b.data = x
    top = Blob([0])
    layer.setup([b], [top])
    return b, top


def test_layer_top_and_blob_shapes():
    layer = make_layer("""
        name: "u" type: "Deconvolution" bottom: "x" top: "y"
        convolution_param { num_output: 6 kernel_h: 5 kernel_w: 3
          stride_h: 2 stride_w: 3 pad_h: 1 pad_w: 0 dilation: 2 group: 2
          weight_filler { type: "xavier" } }""")
    x = torch.randn(2, 4, 5, 7)
    b, top = _setup(layer, x)
    layer.forward([b], [top])
    assert list(layer.blobs[0].shape) == [4, 3, 5, 3]
    assert list(layer.blobs[1].shape) == [6]
    # stride*(H-1) + dil*(k-1) + 1 - 2*pad
    assert tuple(top.data.shape) == (2, 6, 2 * 4 + 2 * 4 + 1 - 2,
                                     3 * 6 + 2 * 2 + 1)


@pytest.mark.parametrize("text,shape", [
    ("num_output: 6 kernel_size: 4 stride: 2 pad: 1", (2, 4, 5, 6)),
    ("num_output: 6 kernel_size: 3 stride: 2 group: 2", (2, 4, 4, 5)),
    ("num_output: 5 kernel_size: 3 stride: 2 pad: 1 dilation: 2",
     (2, 4, 4, 4)),
    ("num_output: 6 kernel_size: 4 stride: 2 pad: 1 bias_term: false",
     (2, 4, 5, 5)),
], ids=["plain", "grouped", "dilated", "bias_free"])
def test_layer_grads(text, shape):
    layer = make_layer(f"""
        name: "u" type: "Deconvolution" bottom: "x" top: "y"
        convolution_param {{ {text}
          weight_filler {{ type: "gaussian" std: 0.2 }}
          bias_filler {{ type: "constant" value: 0.3 }} }}""")
    run_grad_check(layer, [torch.randn(*shape)])


def test_layer_bilinear_upsampler():
    """FCN's fixed upsampler: group == C, bilinear filler, lr_mult 0."""
    C = 5
    layer = make_layer(f"""
        name: "up" type: "Deconvolution" bottom: "x" top: "y"
        param {{ lr_mult: 0 }}
        convolution_param {{ num_output: {C} group: {C} kernel_size: 4
          stride: 2 pad: 1 bias_term: false
          weight_filler {{ type: "bilinear" }} }}""")
    x = torch.randn(2, C, 4, 6)
    b, top = _setup(layer, x)
    layer.forward([b], [top])
    k = dc.bilinear_kernel(4).float()
    want = F.conv_transpose2d(x, k.expand(C, 1, 4, 4).contiguous(),
                              stride=2, padding=1, groups=C)
    assert tuple(top.data.shape) == (2, C, 8, 12)
    torch.testing.assert_close(top.data, want, rtol=1e-6, atol=1e-6)
    top.diff = torch.randn_like(top.data)
    layer.blobs[0].zero_diff()
    layer.backward([top], [True], [b])
    assert b.diff is not None and tuple(b.diff.shape) == tuple(x.shape)
    d = layer.blobs[0].diff
    assert d is None or not d.any(), "lr_mult 0: no weight gradient"


# -------------------------------------------------------------------- net

def _solver(seed=11):
    sp = caffe_pb.SolverParameter(
        net_param=text_format.parse(dc.NET_TEXT, caffe_pb.NetParameter),
        base_lr=0.1, momentum=0.9, weight_decay=0.0, lr_policy="fixed",
        max_iter=100, random_seed=seed, snapshot_prefix="deconv_net")
    return Solver(sp)


def test_net_trains_and_roundtrips(tmp_path):
    here = os.getcwd()
    os.chdir(tmp_path)
    try:
        s = _solver()
        up = s.net.layer_by_name("up")
        assert list(up.blobs[0].shape) == [8, 3, 4, 4]
        x, t = dc.net_batch()
        s.net.data_layers()[0].reset(x, t)
        first = s._step_one()
        last = s.step(29)
        print(f"loss {first:.4f} -> {last:.4f} over 30 steps")
        assert last < 0.8 * first
        assert tuple(s.net.blob_by_name("u").data.shape) == (4, 3, 8, 8)

        model = s.snapshot()
        state = s.snapshot_filename("state")
        assert model.endswith(".caffemodel") and os.path.exists(state)
        s2 = _solver(seed=12)
        s2.restore(state)
        assert s2.iter == s.iter
        up2 = s2.net.layer_by_name("up")
        assert list(up2.blobs[0].shape) == [8, 3, 4, 4]
        for a, b in zip(s.params, s2.params):
            assert list(a.shape) == list(b.shape)
            torch.testing.assert_close(a.data, b.data)
        for a, b in zip(s.history, s2.history):
            torch.testing.assert_close(a, b)
        # the weights alone, from the .caffemodel
        s3 = _solver(seed=13)
        saved = read_binary_proto(model, caffe_pb.NetParameter)
        saved_up = [lp for lp in saved.layer if lp.name == "up"][0]
        assert Blob.shape_from_proto(saved_up.blobs[0]) == [8, 3, 4, 4]
        s3.net.copy_trained_layers_from(saved)
        torch.testing.assert_close(
            s3.net.layer_by_name("up").blobs[0].data, up.blobs[0].data)
    finally:
        os.chdir(here)


# -------------------------------------------------------------- benchmark

def test_bench_shape_counts():
    from caffeonspark_amd.tools import deconv_bench as db
    c = db.shape_counts(32, 64, 64, 56, 56, 4, 2, 1)
    assert c["out_hw"] == [112, 112]
    assert c["y_bytes"] == 32 * 64 * 112 * 112 * 2
    assert c["z_bytes"] == 32 * 57 * 57 * 4 * 64 * 2
    assert c["dcol_bytes"] == 32 * 56 * 56 * 16 * 64 * 2
    assert c["d2s_gemm_flops"] == 2 * 32 * 57 * 57 * 256 * 256
    assert c["col2im_gemm_flops"] == 2 * 32 * 56 * 56 * 1024 * 64
    if not torch.cuda.is_available():
        with pytest.raises(SystemExit):     # no quiet CPU fall-back
            db.main([])
