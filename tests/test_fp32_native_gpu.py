"""Native fp32 path (gemm_f32.hip): the f32-MFMA GEMM, the fp32 conv
lowering on top of it, and its routing through the public op dispatch.

Tolerance is derived, not measured.  The f32 MFMA is an fmaf chain with one
rounding per product, so for ANY summation order (split-K included)

    |C - C64| <= 2*K*2^-24 * (|A|.|B|) + 2^-23 * |C64|

where C64 is the same product in float64 on the CPU from the same fp32
inputs, |A|.|B| the product of the absolute values and K the reduction
length of that GEMM; the factor 2 covers the bias add and the atomic
split-K combine.  A bf16-input path misses this bound by orders of
magnitude, so passing it also proves the fp32 kernel ran.
"""

import os

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from caffeonspark_amd import ops
from caffeonspark_amd.ops import dispatcher


def dev():
    return torch.device("cuda:0")


def _check(got, c64, absprod, K, what):
    got = got.detach().double().cpu()
    assert got.shape == c64.shape, f"{what}: shape {got.shape} vs {c64.shape}"
    tol = 2.0 * K * 2.0 ** -24 * absprod + 2.0 ** -23 * c64.abs()
    err = (got - c64).abs()
    worst = (err - tol).max().item()
    print(f"{what}: max err {err.max().item():.3e}, "
          f"min slack {-worst:.3e}")
    assert torch.isfinite(got).all(), f"{what}: non-finite output"
    assert worst <= 0.0, f"{what}: bound exceeded by {worst:.3e}"


def _rand(shape, seed):
    g = torch.Generator().manual_seed(seed)
    # asymmetric, not bf16-representable
    return torch.randn(shape, generator=g) + 0.123


def _gemm_case(m, n, k, ta, tb, seed, bias=False, relu=False, splitk=1):
    gemm = ops.gpu_op("gemm_f32")
    assert gemm is not None, "gemm_f32 is not registered"
    a = _rand((k, m) if ta else (m, k), seed)
    b = _rand((k, n) if tb else (n, k), seed + 1)
    bv = _rand((n,), seed + 2) if bias else None
    al = (a.t() if ta else a).double()
    bl = (b if tb else b.t()).double()
    c64 = al @ bl
    absprod = al.abs() @ bl.abs()
    if bv is not None:
        c64 = c64 + bv.double()
    if relu:
        c64 = c64.clamp_min(0)
    c = (torch.zeros if splitk > 1 else torch.empty)(
        (m, n), dtype=torch.float32, device=dev())
    out = gemm(a.to(dev()), b.to(dev()), c,
               None if bv is None else bv.to(dev()), m, n, k,
               a.shape[1], b.shape[1], n, ta, tb, splitk, relu)
    assert out is c
    _check(c, c64, absprod, k, f"gemm_f32 {m}x{n}x{k} ta={ta} tb={tb}")


@pytest.mark.parametrize("ta", [False, True])
@pytest.mark.parametrize("tb", [False, True])
@pytest.mark.parametrize("mnk", [(1, 1, 1), (33, 17, 5), (130, 70, 41),
                                 (128, 128, 64), (257, 129, 1030)])
def test_gemm_f32_transposes(mnk, ta, tb):
    _gemm_case(*mnk, ta, tb, seed=3)


def test_gemm_f32_bias_relu():
    _gemm_case(200, 130, 96, False, False, seed=5, bias=True, relu=True)


@pytest.mark.parametrize("splitk", [3, 65])
def test_gemm_f32_splitk(splitk):
    # 65 slices over ceil(1030/16) = 65 k-tiles: one tile per slice, the
    # last one a 6-element tail; the bias must be added exactly once
    _gemm_case(257, 129, 1030, True, True, seed=7, bias=True, splitk=splitk)


def test_gemm_f32_row_subviews():
    """Operands whose base is only 4-byte aligned and whose ld != row
    length; C outside the view keeps its sentinel."""
    gemm = ops.gpu_op("gemm_f32")
    assert gemm is not None, "gemm_f32 is not registered"
    m, n, k = 130, 70, 41
    abuf = _rand((m, k + 3), 11).to(dev())
    bbuf = _rand((n, k + 3), 12).to(dev())
    cbuf = torch.full((m, n + 3), -7.5, dtype=torch.float32, device=dev())
    a, b, c = abuf[:, 1:k + 1], bbuf[:, 1:k + 1], cbuf[:, 1:n + 1]
    assert a.data_ptr() % 8 == 4 and c.data_ptr() % 8 == 4
    gemm(a, b, c, None, m, n, k, k + 3, k + 3, n + 3, False, False, 1,
         False)
    al, bl = a.double().cpu(), b.double().cpu().t()
    _check(c, al @ bl, al.abs() @ bl.abs(), k, "gemm_f32 sub-view")
    assert (cbuf[:, 0] == -7.5).all() and (cbuf[:, n + 1:] == -7.5).all()


# ---------------------------------------------------------------- dispatch


class _Counter:
    def __init__(self, fn):
        self.fn, self.n = fn, 0

    def __call__(self, *a, **k):
        self.n += 1
        return self.fn(*a, **k)


@pytest.fixture
def native(monkeypatch):
    """Select the native fp32 route and count the calls that reach it."""
    assert ops.native_available()
    monkeypatch.setenv("COS_FP32_NATIVE", "1")
    counters = {}
    for name in ("conv2d_forward_f32", "conv2d_backward_f32",
                 "fc_forward_f32", "fc_backward_f32"):
        assert name in dispatcher.gpu_impls, f"{name} is not registered"
        counters[name] = _Counter(dispatcher.gpu_impls[name])
        monkeypatch.setitem(dispatcher.gpu_impls, name, counters[name])
    return counters


@pytest.mark.parametrize("mkn", [(5, 800, 500), (5, 500, 10)])
@pytest.mark.parametrize("bias", [False, True])
def test_fc_f32_dispatch(native, mkn, bias):
    M, K, N = mkn
    x, w, dy = _rand((M, K), 21), _rand((N, K), 22), _rand((M, N), 23)
    b = _rand((N,), 24) if bias else None
    xg, wg, dyg = x.to(dev()), w.to(dev()), dy.to(dev())
    bg = None if b is None else b.to(dev())
    x64, w64, dy64 = x.double(), w.double(), dy.double()
    absy = x64.abs() @ w64.abs().t()
    y64 = x64 @ w64.t() + (0 if b is None else b.double())

    _check(ops.fc_forward(xg, wg, bg), y64, absy, K, "fc y")
    _check(ops.fc_forward(xg, wg, bg, relu=True), y64.clamp_min(0), absy, K,
           "fc y relu")
    assert native["fc_forward_f32"].n == 2

    dw_out = torch.full((N, K), 3.0, dtype=torch.float32, device=dev())
    dx, dw, db = ops.fc_backward(xg, wg, dyg, need_dx=True, bias=bias,
                                 dw_out=dw_out)
    assert dw is dw_out
    _check(dx, dy64 @ w64, dy64.abs() @ w64.abs(), N, "fc dx")
    _check(dw_out, dy64.t() @ x64, dy64.abs().t() @ x64.abs(), M, "fc dw")
    if bias:
        _check(db, dy64.sum(0), dy64.abs().sum(0), M, "fc db")
    else:
        assert db is None
    dx, dw, db = ops.fc_backward(xg, wg, dyg, need_dx=False, bias=False)
    assert dx is None and db is None
    _check(dw, dy64.t() @ x64, dy64.abs().t() @ x64.abs(), M, "fc dw (own)")
    assert native["fc_backward_f32"].n == 2


def _pair(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (v, v)


CONV_CASES = [
    dict(n=4, c=3, h=33, w=33, k=32, r=11, stride=4, pad=0, g=1),
    dict(n=2, c=16, h=15, w=15, k=32, r=5, stride=1, pad=2, g=2),
    dict(n=2, c=1, h=28, w=28, k=20, r=5),
    dict(n=3, c=20, h=7, w=7, k=24, r=1),
    dict(n=2, c=8, h=13, w=13, k=12, r=3, pad=2, dilation=2),
    dict(n=2, c=6, h=11, w=14, k=10, r=(3, 5), stride=(2, 1), pad=(1, 2)),
]


@pytest.mark.parametrize("case", CONV_CASES,
                         ids=[f"case{i}" for i in range(len(CONV_CASES))])
def test_conv_f32_dispatch(native, case):
    n, c, h, w_, k = (case[key] for key in ("n", "c", "h", "w", "k"))
    R, S = _pair(case["r"])
    stride, pad = _pair(case.get("stride", 1)), _pair(case.get("pad", 0))
    dil, g = _pair(case.get("dilation", 1)), case.get("g", 1)
    cg, kg = c // g, k // g
    x, w, b = _rand((n, c, h, w_), 31), _rand((k, cg, R, S), 32), \
        _rand((k,), 33)
    kw = dict(stride=stride, padding=pad, dilation=dil, groups=g)
    x64, w64, b64 = x.double(), w.double(), b.double()
    y64 = F.conv2d(x64, w64, b64, **kw)
    absy = F.conv2d(x64.abs(), w64.abs(), None, **kw)
    dy = _rand(tuple(y64.shape), 34)
    dy64 = dy.double()
    xg, wg, bg, dyg = (t.to(dev()) for t in (x, w, b, dy))
    args = (stride, pad, dil, g)

    y = ops.conv2d_forward(xg, wg, bg, *args, ctx={})
    assert tuple(y.shape) == tuple(y64.shape)
    _check(y, y64, absy, cg * R * S, "conv y")
    yr = ops.conv2d_forward(xg, wg, bg, *args, ctx={}, relu=True)
    _check(yr, y64.clamp_min(0), absy, cg * R * S, "conv y relu")
    y0 = ops.conv2d_forward(xg, wg, None, *args)
    _check(y0, y64 - b64.view(1, -1, 1, 1), absy, cg * R * S, "conv y nobias")
    assert native["conv2d_forward_f32"].n == 3

    dx, dw, db = ops.conv2d_backward(xg, wg, dyg, *args, need_dx=True,
                                     need_dw=True, bias=True, ctx={})
    P, Q = y64.shape[2:]
    _check(dx,
           torch.nn.grad.conv2d_input(list(x.shape), w64, dy64, **kw),
           torch.nn.grad.conv2d_input(list(x.shape), w64.abs(), dy64.abs(),
                                      **kw),
           kg * R * S, "conv dx")
    dw64 = torch.nn.grad.conv2d_weight(x64, list(w.shape), dy64, **kw)
    absdw = torch.nn.grad.conv2d_weight(x64.abs(), list(w.shape),
                                        dy64.abs(), **kw)
    _check(dw, dw64, absdw, n * P * Q, "conv dw")
    _check(db, dy64.sum(dim=(0, 2, 3)), dy64.abs().sum(dim=(0, 2, 3)),
           n * P * Q, "conv db")

    dw_out = torch.full(tuple(w.shape), 3.0, dtype=torch.float32,
                        device=dev())
    dx, dw, db = ops.conv2d_backward(xg, wg, dyg, *args, need_dx=False,
                                     need_dw=True, bias=False,
                                     dw_out=dw_out)
    assert dx is None and db is None and dw is dw_out
    _check(dw_out, dw64, absdw, n * P * Q, "conv dw_out")
    assert native["conv2d_backward_f32"].n == 2


def test_conv_f32_channels_last_input_and_dy(native):
    """Downstream reference ops hand channels-last tensors back in: x and
    dy in channels-last memory give the same result."""
    x, w = _rand((2, 16, 9, 9), 41), _rand((8, 16, 3, 3), 42)
    kw = dict(stride=(1, 1), padding=(1, 1), dilation=(1, 1), groups=1)
    x64, w64 = x.double(), w.double()
    y64 = F.conv2d(x64, w64, None, **kw)
    dy = _rand(tuple(y64.shape), 43)
    cl = torch.channels_last
    xg = x.to(dev()).contiguous(memory_format=cl)
    dyg = dy.to(dev()).contiguous(memory_format=cl)
    args = ((1, 1), (1, 1), (1, 1), 1)
    y = ops.conv2d_forward(xg, w.to(dev()), None, *args)
    _check(y, y64, F.conv2d(x64.abs(), w64.abs(), None, **kw), 144, "cl y")
    dx, dw, db = ops.conv2d_backward(xg, w.to(dev()), dyg, *args,
                                     bias=False)
    _check(dx, torch.nn.grad.conv2d_input(list(x.shape), w64, dy.double(),
                                          **kw),
           torch.nn.grad.conv2d_input(list(x.shape), w64.abs(),
                                      dy.double().abs(), **kw), 72, "cl dx")
    _check(dw, torch.nn.grad.conv2d_weight(x64, list(w.shape), dy.double(),
                                           **kw),
           torch.nn.grad.conv2d_weight(x64.abs(), list(w.shape),
                                       dy.double().abs(), **kw), 162, "cl dw")


def test_conv_f32_ctx_col_reuse_and_revalidation(native):
    """The forward leaves its col matrices in the context for the backward
    pass; they are used only while they still describe x."""
    n, c, k, g = 2, 16, 32, 2
    x, w = _rand((n, c, 15, 15), 51), _rand((k, c // g, 5, 5), 52)
    kw = dict(stride=(1, 1), padding=(2, 2), dilation=(1, 1), groups=g)
    dy = _rand((n, k, 15, 15), 53)
    x64, w64, dy64 = x.double(), w.double(), dy.double()
    args = ((1, 1), (2, 2), (1, 1), g)
    xg, wg, dyg = x.to(dev()), w.to(dev()), dy.to(dev())
    K = n * 15 * 15

    def refs(xx):
        return (torch.nn.grad.conv2d_weight(xx, list(w.shape), dy64, **kw),
                torch.nn.grad.conv2d_weight(xx.abs(), list(w.shape),
                                            dy64.abs(), **kw))

    ctx = {}
    ops.conv2d_forward(xg, wg, None, *args, ctx=ctx)
    assert "col_f32" in ctx
    dx, dw, _ = ops.conv2d_backward(xg, wg, dyg, *args, bias=False, ctx=ctx)
    assert "col_f32" not in ctx          # consumed: dcol overwrote it
    _check(dw, *refs(x64), K, "ctx dw")
    _check(dx, torch.nn.grad.conv2d_input(list(x.shape), w64, dy64, **kw),
           torch.nn.grad.conv2d_input(list(x.shape), w64.abs(), dy64.abs(),
                                      **kw), (k // g) * 25, "ctx dx")
    # x changed in place after the forward: the cached cols are stale
    ops.conv2d_forward(xg, wg, None, *args, ctx=ctx)
    xg.mul_(2.0)
    _, dw, _ = ops.conv2d_backward(xg, wg, dyg, *args, need_dx=False,
                                   bias=False, ctx=ctx)
    _check(dw, *refs(2.0 * x64), K, "stale-ctx dw")


# ------------------------------------------------------------ LeNet, solver


def _lenet_solver(device):
    from caffeonspark_amd.core.solver import Solver
    from caffeonspark_amd.proto import caffe_pb, text_format

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sp_file = os.path.join(root, "caffeonspark_amd", "models",
                           "lenet_memory_solver.prototxt")
    sp = text_format.parse_file(sp_file, caffe_pb.SolverParameter)
    sp.random_seed = 9
    sp.display = 0
    s = Solver(text_format.parse(text_format.dumps(sp),
                                 caffe_pb.SolverParameter),
               device=device, dtype=torch.float32,
               proto_dir=os.path.dirname(sp_file))
    return s


def _lenet_run(device, steps, s=None):
    s = s if s is not None else _lenet_solver(device)
    g = torch.Generator().manual_seed(21)
    for _ in range(steps):
        x = torch.randn(32, 1, 28, 28, generator=g)
        y = torch.randint(0, 10, (32,), generator=g).float()
        s.net.data_layers()[0].reset(x.to(device), y.to(device))
        s._step_one()
    return s


def _layer_count(s, kind):
    return sum(1 for l in s.net.layers if l.param.type == kind)


def _reset(counters):
    for c in counters.values():
        c.n = 0


def test_fp32_solver_takes_native_route(native):
    # building the nets runs every layer once for shape propagation:
    # count the training step alone
    s = _lenet_solver(dev())
    _reset(native)
    _lenet_run(dev(), 1, s)
    n_conv, n_ip = _layer_count(s, "Convolution"), \
        _layer_count(s, "InnerProduct")
    assert n_conv == 2 and n_ip == 2
    assert native["conv2d_forward_f32"].n == n_conv
    assert native["fc_forward_f32"].n == n_ip
    assert native["conv2d_backward_f32"].n == n_conv
    assert native["fc_backward_f32"].n == n_ip


def test_fp32_library_route_still_selectable(native, monkeypatch):
    monkeypatch.setenv("COS_FP32_NATIVE", "0")
    s = _lenet_solver(dev())
    _reset(native)
    _lenet_run(dev(), 1, s)
    assert all(c.n == 0 for c in native.values())


def test_fp32_native_end_to_end_parity(native):
    """Three LeNet fp32 steps on the native route against CPU fp32: the
    criterion of test_fp32_gpu_path_parity (2e-3 separates fp32 numerics
    from bf16 numerics)."""
    w_cpu = _lenet_run(torch.device("cpu"), 3).flat_w.cpu()
    s = _lenet_solver(dev())
    _reset(native)
    w_gpu = _lenet_run(dev(), 3, s).flat_w.cpu()
    assert native["conv2d_forward_f32"].n == 6
    rel = (w_cpu - w_gpu).norm() / w_cpu.norm().clamp_min(1e-6)
    print(f"relL2 after 3 steps: {rel:.3e}")
    assert rel < 2e-3, f"native fp32 path diverged from CPU fp32: {rel}"
