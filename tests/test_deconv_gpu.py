"""Deconvolution on the GPU: the two depth-to-space kernels bit-for-bit
against their torch constructions, the whole op on both routes against
float64 with the bounds derived in _deconv_cases.py, a net step against the
CPU, and the single-K-tile convolution a 2x2/stride-2 deconvolution's
backward pass runs."""

import pytest
import torch
import torch.nn.functional as F

import _deconv_cases as dc

from caffeonspark_amd import ops
from caffeonspark_amd.core import Net
from caffeonspark_amd.proto import caffe_pb, text_format

pytestmark = pytest.mark.gpu

BF = torch.bfloat16


def dev():
    return torch.device("cuda:0")


def within(name, got, want, tol):
    err = (got.detach().double().cpu() - want).abs()
    used = (err / tol.clamp_min(1e-300)).max().item()
    print(f"{name}: max err {err.max().item():.3e}, max err/bound {used:.3f}")
    over = ~(err <= tol)
    assert not over.any(), (
        f"{name}: {int(over.sum())}/{over.numel()} beyond the bound, worst "
        f"excess {(err - tol)[over].max().item():.3e}")


# ---------------------------------------------------------------- kernels

@pytest.mark.parametrize("Ci,Co,R,S,st", [
    (8, 8, 4, 4, 2), (16, 6, 5, 3, 2), (8, 8, 7, 7, 3), (8, 4, 2, 2, 2),
    (8, 8, 16, 16, 8),
])
def test_pack_weight_kernel(Ci, Co, R, S, st):
    ext = ops.native()
    g = torch.Generator().manual_seed(R + S)
    wd = torch.randn(Ci, Co, R, S, generator=g).to(BF)
    _, _, kcol, kpad = dc.d2s_dims(R, S, st, Ci)
    rows = dc.pad128(st * st * Co)
    dst = torch.zeros((rows, kpad), dtype=BF, device=dev())
    # poison the live region: the kernel must write all of it, phantom
    # zeros included
    dst[:st * st * Co, :kcol] = 7.0
    ext.d2s_pack_weight(wd.to(dev()), dst, Ci, Co, R, S, st, kpad)
    assert torch.equal(dst.cpu(), dc.pack_weight(wd, st, rows, kpad))


@pytest.mark.parametrize("Co,N,H,W,R,S,st,ph,pw", [
    (8, 2, 4, 5, 5, 3, 2, 1, 0),     # vector path, odd Ho and Wo, ph != pw
    (6, 2, 4, 5, 5, 3, 2, 1, 0),     # scalar path
    (8, 1, 3, 3, 7, 7, 3, 2, 1),     # stride 3
    (6, 1, 3, 4, 4, 4, 2, 0, 1),     # scalar path, even sizes
])
def test_unpack_kernel(Co, N, H, W, R, S, st, ph, pw):
    ext = ops.native()
    Rp, Sp = -(-R // st), -(-S // st)
    Hp, Wp = H + Rp - 1, W + Sp - 1
    Ho, Wo = dc.out_dim(H, R, st, ph), dc.out_dim(W, S, st, pw)
    g = torch.Generator().manual_seed(Co + st)
    z = torch.randn(N, Hp, Wp, st * st * Co, generator=g).to(BF)
    want = dc.unpack(z, Co, st, ph, pw, Ho, Wo)
    y = torch.full((N, Co, Ho, Wo), 7.0, dtype=BF, device=dev()) \
        .contiguous(memory_format=torch.channels_last)
    ext.d2s_unpack(z.to(dev()), y, st, ph, pw, Hp, Wp)
    assert y.is_contiguous(memory_format=torch.channels_last)
    assert torch.equal(y.cpu(), want)
    # planar destination: written through its strides
    y2 = torch.full((N, Co, Ho, Wo), 7.0, dtype=BF, device=dev())
    ext.d2s_unpack(z.to(dev()), y2, st, ph, pw, Hp, Wp)
    assert torch.equal(y2.cpu(), want)


# --------------------------------------------------------------- whole op

def _forward(inp, relu, ctx):
    d = dev()
    b = inp["b"].to(d) if inp["b"] is not None else None
    return ops.deconv2d_forward(
        inp["x"].to(d), inp["w"].to(d).float(), b, inp["stride"],
        inp["pad"], inp["dilation"], inp["groups"], ctx=ctx, relu=relu)


def _check_forward(inp, relu, route):
    ctx = {}
    y = _forward(inp, relu, ctx)
    assert ctx["route"] == route
    assert y.dtype == BF
    want, tol = dc.forward_oracle(inp, relu, route)
    assert tuple(y.shape) == tuple(want.shape)
    within(f"y[{route}]", y, want, tol)


D2S_VARIANTS = [(name, bias, relu) for name in dc.D2S_CASES
                for bias, relu in ((True, False), (False, False),
                                   (True, True))]


@pytest.mark.parametrize("name,bias,relu", D2S_VARIANTS)
def test_forward_d2s(name, bias, relu, monkeypatch):
    monkeypatch.setenv("COS_DECONV_D2S", "1")
    inp = dc.make_inputs(*dc.D2S_CASES[name], seed=len(name), bias=bias)
    _check_forward(inp, relu, "d2s")


@pytest.mark.parametrize("name", list(dc.FALLBACK_CASES))
def test_forward_fallback(name, monkeypatch):
    monkeypatch.setenv("COS_DECONV_D2S", "1")
    inp = dc.make_inputs(seed=len(name), **dc.FALLBACK_CASES[name])
    if name == "depthwise":
        inp["w"] = dc.bilinear_kernel(4).to(BF).expand(6, 1, 4, 4) \
            .contiguous()
    _check_forward(inp, False, "col2im")
    _check_forward(inp, True, "col2im")


def test_forward_d2s_switched_off(monkeypatch):
    monkeypatch.setenv("COS_DECONV_D2S", "0")
    for name in ("partial_m_tile", "phantom_nonsquare"):
        inp = dc.make_inputs(*dc.D2S_CASES[name], seed=3)
        _check_forward(inp, False, "col2im")
        inp["b"] = None
        _check_forward(inp, True, "col2im")


def _check_backward(inp):
    from caffeonspark_amd.ops import gpu as G
    d = dev()
    x, dy = inp["x"].to(d), inp["dy"].to(d)
    w = inp["w"].to(d).float()
    orc = dc.backward_oracle(inp)
    args = (inp["stride"], inp["pad"], inp["dilation"], inp["groups"])
    G.begin_backward()
    dx, dw, db = ops.deconv2d_backward(x, w, dy, *args)
    assert dx.dtype == BF and dw.dtype == torch.float32
    for name, got in (("dx", dx), ("dw", dw), ("db", db)):
        assert tuple(got.shape) == tuple(orc[name][0].shape), name
        within(name, got, *orc[name])
    # arena hand-off: the gradients land in the tensors passed in
    dw_out = torch.full_like(w, float("nan"))
    db_out = torch.zeros(dy.shape[1], device=d)
    G.begin_backward()
    dx2, dw2, db2 = ops.deconv2d_backward(x, w, dy, *args, dw_out=dw_out,
                                          db_out=db_out)
    assert dw2 is dw_out and db2 is db_out
    within("dw_out", dw_out, *orc["dw"])
    within("db_out", db_out, *orc["db"])
    G.begin_backward()
    dx3, dw3, db3 = ops.deconv2d_backward(x, w, dy, *args, need_dx=False,
                                          need_dw=False, bias=False)
    assert dx3 is None and dw3 is None and db3 is None
    G.begin_backward()
    _, dw4, _ = ops.deconv2d_backward(x, w, dy, *args, need_dx=False,
                                      bias=False)
    within("dw without dx", dw4, *orc["dw"])


@pytest.mark.parametrize("name", ["partial_m_tile", "phantom_nonsquare",
                                  "single_k_tile"])
def test_backward_d2s_cases(name):
    _check_backward(dc.make_inputs(*dc.D2S_CASES[name], seed=len(name)))


def test_backward_grouped():
    _check_backward(dc.make_inputs(seed=9, **dc.FALLBACK_CASES["groups2"]))


# -------------------------------------------------------------------- net

def test_net_step_parity(monkeypatch):
    """One forward/backward of conv -> ReLU -> Deconvolution -> per-pixel
    loss: bf16 on the GPU against fp32 on the CPU."""
    monkeypatch.setenv("COS_DECONV_D2S", "1")
    param = text_format.parse(dc.NET_TEXT, caffe_pb.NetParameter)
    state = caffe_pb.NetState(phase=caffe_pb.Phase.TRAIN)
    cpu_net = Net(param, state, seed=3)
    gpu_net = Net(param, state, device=dev(), dtype=BF, seed=3)
    for cl, gl in zip(cpu_net.layers, gpu_net.layers):
        for cb, gb in zip(cl.blobs, gl.blobs):
            gb.data.copy_(cb.data.to(gb.data.device))
    x, t = dc.net_batch()
    cpu_net.data_layers()[0].reset(x, t)
    gpu_net.data_layers()[0].reset(x.to(dev(), BF), t.to(dev()))
    closs = float(cpu_net.forward())
    gloss = float(gpu_net.forward())
    print(f"loss cpu {closs:.5f} gpu {gloss:.5f}")
    assert gpu_net.layer_by_name("up")._ctx["route"] == "d2s"
    assert abs(closs - gloss) / max(abs(closs), 1e-6) < 0.05
    cpu_net.backward()
    gpu_net.backward()
    for cl, gl in zip(cpu_net.layers, gpu_net.layers):
        for cb, gb in zip(cl.blobs, gl.blobs):
            if cb.diff is None:
                continue
            cg, gg = cb.diff.float(), gb.diff.float().cpu()
            rel = (cg - gg).norm() / cg.norm().clamp_min(1e-4)
            print(f"{cl.name} grad relL2 {rel:.4f}")
            assert rel < 0.08, f"{cl.name} grad mismatch relL2={rel:.3f}"


# ------------------------------------------------- single-K-tile convolution

def test_conv_single_k_tile():
    """A 2x2/stride-2 convolution over 8 channels: R*S*C = 32, one real K
    tile of the implicit forward GEMM, whose pipelined loop needs at least
    two (the second is zero padding).  It is the dx convolution of a
    2x2/stride-2 deconvolution.  Bounds as in _deconv_cases.py."""
    from caffeonspark_amd.ops import gpu as G
    g = torch.Generator().manual_seed(21)
    N, C, K, H, W = 4, 8, 8, 16, 16             # N*P*Q = 256: two M tiles
    x = torch.randn(N, C, H, W, generator=g).to(BF)
    w = (torch.randn(K, C, 2, 2, generator=g) * 0.25).to(BF)
    b = torch.randn(K, generator=g)
    dy = torch.randn(N, K, H // 2, W // 2, generator=g).to(BF)
    d = dev()
    args = ((2, 2), (0, 0), (1, 1), 1)
    ctx = {}
    y = ops.conv2d_forward(x.to(d), w.to(d).float(), b.to(d), *args, ctx=ctx)
    assert ctx.get("implicit"), "expected the implicit forward route"
    xd, wd_, dyd = x.double(), w.double(), dy.double()
    want = F.conv2d(xd, wd_, b.double(), stride=2)
    t = F.conv2d(xd.abs(), wd_.abs(), b.double().abs(), stride=2)
    Kc = 2 * 2 * C
    within("y", y, want, (dc.U + 2 * (Kc + 2) * dc.E32) * t)

    G.begin_backward()
    dx, dw, db = ops.conv2d_backward(x.to(d), w.to(d).float(), dy.to(d),
                                     *args, ctx=ctx)
    wdx = torch.nn.grad.conv2d_input(list(x.shape), wd_, dyd, stride=2)
    tdx = torch.nn.grad.conv2d_input(list(x.shape), wd_.abs(), dyd.abs(),
                                     stride=2)
    # kernel == stride: one tap per input pixel, so col2im adds nothing to
    # the single rounding of the dcol GEMM (K = Kout terms)
    within("dx", dx, wdx, (dc.U + 2 * (K + 2) * dc.E32) * tdx)
    wdw = torch.nn.grad.conv2d_weight(xd, list(w.shape), dyd, stride=2)
    tdw = torch.nn.grad.conv2d_weight(xd.abs(), list(w.shape), dyd.abs(),
                                      stride=2)
    npq = N * (H // 2) * (W // 2)
    within("dw", dw, wdw, 2 * (npq + 2) * dc.E32 * tdw)
    within("db", db, dyd.sum(dim=(0, 2, 3)),
           2 * (npq + 2) * dc.E32 * dyd.abs().sum(dim=(0, 2, 3)))


def test_conv_single_k_tile_dx():
    """The stride-1 2x2 convolution over 8 output channels: its data
    gradient is the flipped-weight implicit GEMM with R*S*Kout = 32, one
    real K tile, the same invariant on the dx side."""
    from caffeonspark_amd.ops import gpu as G
    g = torch.Generator().manual_seed(22)
    N, C, K, H, W = 4, 8, 8, 9, 9               # N*H*W = 324: three M tiles
    x = torch.randn(N, C, H, W, generator=g).to(BF)
    w = (torch.randn(K, C, 2, 2, generator=g) * 0.25).to(BF)
    dy = torch.randn(N, K, H - 1, W - 1, generator=g).to(BF)
    d = dev()
    args = ((1, 1), (0, 0), (1, 1), 1)
    ctx = {}
    wg = w.to(d).float()
    y = ops.conv2d_forward(x.to(d), wg, None, *args, ctx=ctx)
    assert ctx.get("implicit") and getattr(wg, "_cos_wrF", None) is not None
    xd, wd_, dyd = x.double(), w.double(), dy.double()
    Kc = 2 * 2 * C
    within("y", y, F.conv2d(xd, wd_),
           (dc.U + 2 * (Kc + 2) * dc.E32) * F.conv2d(xd.abs(), wd_.abs()))
    G.begin_backward()
    dx, _, _ = ops.conv2d_backward(x.to(d), wg, dy.to(d), *args,
                                   need_dw=False, bias=False, ctx=ctx)
    wdx = torch.nn.grad.conv2d_input(list(x.shape), wd_, dyd)
    tdx = torch.nn.grad.conv2d_input(list(x.shape), wd_.abs(), dyd.abs())
    Kd = 2 * 2 * K
    within("dx", dx, wdx, (dc.U + 2 * (Kd + 2) * dc.E32) * tdx)


# ------------------------------------------------------ weights that change

@pytest.mark.parametrize("name,route", [
    ("partial_m_tile", "d2s"), ("stride1", "col2im"), ("groups2", "col2im")])
def test_forward_repacks_changed_weights(name, route, monkeypatch):
    """The packed layouts cached on the weight tensor (depth-to-space,
    flipped, dcol) are rebuilt on every call: an in-place update between
    two forwards must show in the second."""
    monkeypatch.setenv("COS_DECONV_D2S", "1")
    if route == "d2s":
        inp = dc.make_inputs(*dc.D2S_CASES[name], seed=4)
    else:
        inp = dc.make_inputs(seed=4, **dc.FALLBACK_CASES[name])
    d = dev()
    x, b = inp["x"].to(d), inp["b"].to(d)
    w = inp["w"].to(d).float()
    args = (inp["stride"], inp["pad"], inp["dilation"], inp["groups"])
    ctx = {}
    ops.deconv2d_forward(x, w, b, *args, ctx=ctx)
    assert ctx["route"] == route
    g = torch.Generator().manual_seed(5)
    new_w = (torch.randn(inp["w"].shape, generator=g) * 0.25).to(BF)
    w.copy_(new_w.to(d))
    y = ops.deconv2d_forward(x, w, b, *args, ctx=ctx)
    want, tol = dc.forward_oracle(dict(inp, w=new_w), False, route)
    within(f"y after update [{route}]", y, want, tol)
