"""Space-to-depth route for strided small-C convolutions (conv1-class).

A stride-st convolution over C channels runs as a stride-1 R'xS'
convolution over the st*st*C channels of a rearranged input.  The index
maps are checked on the CPU against a brute-force evaluation of their
definitions and against the convolution they must reproduce; the HIP
kernels are checked for exact equality against the same torch
constructions, and the whole op against the fp32 reference on
bf16-rounded inputs with the tolerances test_gpu_numerics uses."""

import pytest
import torch
import torch.nn.functional as F

from caffeonspark_amd import ops
from caffeonspark_amd.ops import gpu as gpu_ops
from caffeonspark_amd.ops import reference


def dev():
    return torch.device("cuda:0")


def bf(x):
    return x.to(torch.bfloat16)


def agree(got, want, rtol=0.02, atol=0.02):
    torch.testing.assert_close(got.float().cpu(), want.float().cpu(),
                               rtol=rtol, atol=atol)


@pytest.fixture(scope="module", autouse=True)
def _seed():
    torch.manual_seed(11)


# ------------------------------------------------ torch constructions

def _dims(H, W, R, S, st, ph, pw):
    P = (H + 2 * ph - R) // st + 1
    Q = (W + 2 * pw - S) // st + 1
    Rp, Sp = -(-R // st), -(-S // st)
    return P, Q, Rp, Sp, P + Rp - 1, Q + Sp - 1


def pack_ref(x, R, S, st, ph, pw):
    """X'[n][h'][w'][(dy*st+dx)*C + c] = x[n][c][st*h'+dy-ph][st*w'+dx-pw]
    by pad / crop / reshape / permute."""
    N, C, H, W = x.shape
    P, Q, Rp, Sp, Hp, Wp = _dims(H, W, R, S, st, ph, pw)
    canvas = x.new_zeros((N, C, max(st * Hp, ph + H), max(st * Wp, pw + W)))
    canvas[:, :, ph:ph + H, pw:pw + W] = x
    canvas = canvas[:, :, :st * Hp, :st * Wp]
    return canvas.reshape(N, C, Hp, st, Wp, st).permute(0, 2, 4, 3, 5, 1) \
        .reshape(N, Hp, Wp, st * st * C).contiguous()


def weight_ref(w, st, rows, Kpad):
    """wrb'[k][(r'*S'+s')*C' + (dy*st+dx)*C + c] = w[k][c][st*r'+dy][st*s'+dx]
    with zero phantom taps, pad columns and pad rows."""
    K, C, R, S = w.shape
    Rp, Sp = -(-R // st), -(-S // st)
    wp = w.new_zeros((K, C, Rp * st, Sp * st))
    wp[:, :, :R, :S] = w
    m = wp.reshape(K, C, Rp, st, Sp, st).permute(0, 2, 4, 3, 5, 1) \
        .reshape(K, Rp * Sp * st * st * C)
    out = w.new_zeros((rows, Kpad))
    out[:K, :m.shape[1]] = m
    return out


def unpack_ref(dwp, K, C, R, S, st):
    Rp, Sp = -(-R // st), -(-S // st)
    return dwp[:, :Rp * Sp * st * st * C].reshape(K, Rp, Sp, st, st, C) \
        .permute(0, 5, 1, 3, 2, 4).reshape(K, C, Rp * st, Sp * st)[
            :, :, :R, :S].contiguous()


def _pad32(k):
    return (k + 31) // 32 * 32


def _pad128(k):
    return (k + 127) // 128 * 128


# pack cases: (N, C, H, W, R, S, stride, pad)
PACK_CASES = [
    (2, 3, 37, 29, 11, 11, 4, 0),   # non-square image: swapped h/w shows
    (2, 3, 35, 35, 11, 11, 4, 2),   # leading zero rows, unused tail rows
    (2, 4, 21, 21, 9, 9, 2, 4),
]
WEIGHT_CASES = [(96, 3, 11, 11, 4), (16, 4, 7, 5, 2)]


# ------------------------------------------------------ CPU: index maps

@pytest.mark.parametrize("case", PACK_CASES)
def test_pack_map_matches_definition(case):
    N, C, H, W, R, S, st, pd = case
    x = torch.randn(N, C, H, W, dtype=torch.float64)
    got = pack_ref(x, R, S, st, pd, pd)
    P, Q, Rp, Sp, Hp, Wp = _dims(H, W, R, S, st, pd, pd)
    assert got.shape == (N, Hp, Wp, st * st * C)
    want = torch.zeros_like(got)
    for hp in range(Hp):
        for dy in range(st):
            hs = st * hp + dy - pd
            if not 0 <= hs < H:
                continue
            for wp in range(Wp):
                for dx in range(st):
                    ws = st * wp + dx - pd
                    if 0 <= ws < W:
                        o = (dy * st + dx) * C
                        want[:, hp, wp, o:o + C] = x[:, :, hs, ws]
    assert torch.equal(got, want)


@pytest.mark.parametrize("case", WEIGHT_CASES)
def test_weight_map_matches_definition(case):
    K, C, R, S, st = case
    w = torch.randn(K, C, R, S, dtype=torch.float64)
    Rp, Sp = -(-R // st), -(-S // st)
    Cp = st * st * C
    Kpad = _pad32(Rp * Sp * Cp)
    got = weight_ref(w, st, _pad128(K), Kpad)
    want = torch.zeros_like(got)
    for r in range(R):
        for s in range(S):
            col = ((r // st) * Sp + s // st) * Cp + ((r % st) * st + s % st) * C
            want[:K, col:col + C] = w[:, :, r, s]
    assert torch.equal(got, want)
    # the unpack inverts the pack on the real taps and drops the rest
    assert torch.equal(unpack_ref(got[:K], K, C, R, S, st), w)


@pytest.mark.parametrize("case", PACK_CASES + [(2, 4, 21, 19, 7, 5, 2, 0)])
def test_s2d_algebra(case):
    """stride-1 conv over X' with the packed weight == the strided conv,
    and its weight gradient unpacks to the strided conv's."""
    N, C, H, W, R, S, st, pd = case
    K = 8
    x = torch.randn(N, C, H, W, dtype=torch.float64)
    w = torch.randn(K, C, R, S, dtype=torch.float64)
    P, Q, Rp, Sp, Hp, Wp = _dims(H, W, R, S, st, pd, pd)
    Cp = st * st * C
    xs = pack_ref(x, R, S, st, pd, pd).permute(0, 3, 1, 2)
    ws = weight_ref(w, st, K, Rp * Sp * Cp).reshape(K, Rp, Sp, Cp) \
        .permute(0, 3, 1, 2)
    want = F.conv2d(x, w, stride=st, padding=pd)
    got = F.conv2d(xs, ws)
    torch.testing.assert_close(got, want, rtol=0, atol=1e-11)
    dy = torch.randn_like(want)
    dws = torch.nn.grad.conv2d_weight(xs, list(ws.shape), dy)
    dwp = dws.permute(0, 2, 3, 1).reshape(K, Rp * Sp * Cp)
    dw = torch.nn.grad.conv2d_weight(x, list(w.shape), dy, stride=st,
                                     padding=pd)
    torch.testing.assert_close(unpack_ref(dwp, K, C, R, S, st), dw, rtol=0,
                               atol=1e-10)


def test_route_gate(monkeypatch):
    monkeypatch.delenv("COS_S2D", raising=False)
    # AlexNet conv1: 3x227x227, 11x11/4 -> 48ch 3x3 over 57x57, K 432->448
    assert gpu_ops._s2d_geom(256, 3, 11, 11, 55, 55, 4, 4, 1, 1) == \
        (4, 3, 3, 48, 57, 57, 432, 448)
    # GoogLeNet conv1 (7x7/2, C=3): st*st*C = 12
    assert gpu_ops._s2d_geom(2, 3, 7, 7, 8, 8, 2, 2, 1, 1) is None
    # stride 1, C % 8 == 0, groups, dilation, sh != sw, NPQ >= 2^20
    assert gpu_ops._s2d_geom(2, 4, 9, 9, 8, 8, 1, 1, 1, 1) is None
    assert gpu_ops._s2d_geom(2, 8, 9, 9, 8, 8, 2, 2, 1, 1) is None
    assert gpu_ops._s2d_geom(2, 4, 9, 9, 8, 8, 2, 2, 1, 2) is None
    assert gpu_ops._s2d_geom(2, 4, 9, 9, 8, 8, 2, 2, 2, 1) is None
    assert gpu_ops._s2d_geom(2, 4, 9, 9, 8, 8, 2, 4, 1, 1) is None
    assert gpu_ops._s2d_geom(512, 3, 11, 11, 55, 55, 4, 4, 1, 1) is None
    # pad32(R'S'C') <= 128: 3x3/2 over 4 channels -> 2*2*16 = 64
    assert gpu_ops._s2d_geom(2, 4, 3, 3, 8, 8, 2, 2, 1, 1) is None
    monkeypatch.setenv("COS_S2D", "0")
    assert gpu_ops._s2d_geom(256, 3, 11, 11, 55, 55, 4, 4, 1, 1) is None


# ------------------------------------------------------- GPU: kernels

def _sources(x):
    """The same values as an NCHW-contiguous and a channels-last tensor."""
    return [("nchw", x.contiguous()),
            ("nhwc", x.contiguous(memory_format=torch.channels_last))]


def _run_pack(x, R, S, st, pd):
    N, C, H, W = x.shape
    P, Q, Rp, Sp, Hp, Wp = _dims(H, W, R, S, st, pd, pd)
    # poison the destination: the kernel must write every element
    out = torch.full((N, Hp, Wp, st * st * C), float("nan"),
                     dtype=torch.bfloat16, device=x.device)
    ops.native().s2d_pack(x, out, st, pd, pd, Hp, Wp)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("case", PACK_CASES)
def test_pack_kernel(case):
    N, C, H, W, R, S, st, pd = case
    x = bf(torch.randn(N, C, H, W))
    want = pack_ref(x, R, S, st, pd, pd)
    for name, src in _sources(x.to(dev())):
        got = _run_pack(src, R, S, st, pd)
        assert torch.equal(got.cpu(), want), name


@pytest.mark.gpu
def test_pack_kernel_strided_view():
    N, C, H, W, R, S, st, pd = PACK_CASES[0]
    big = bf(torch.randn(N, C * H * W + 100)).to(dev())
    x = big[:, :C * H * W].view(N, C, H, W)
    assert x.stride(0) > C * H * W
    want = pack_ref(x.cpu(), R, S, st, pd, pd)
    assert torch.equal(_run_pack(x, R, S, st, pd).cpu(), want)
    # channel-minor view with a larger batch stride
    big = bf(torch.randn(N, H * W * C + 64)).to(dev())
    xc = big[:, :H * W * C].view(N, H, W, C).permute(0, 3, 1, 2)
    assert xc.stride(1) == 1 and xc.stride(0) > C * H * W
    want = pack_ref(xc.cpu().contiguous(), R, S, st, pd, pd)
    assert torch.equal(_run_pack(xc, R, S, st, pd).cpu(), want)


@pytest.mark.gpu
def test_pack_kernel_width_chunks():
    """A row wider than the kernel's 8192-element LDS slab is packed in
    several chunks (W'*C' = 179*48 = 8592)."""
    x = bf(torch.randn(1, 3, 21, 715))
    want = pack_ref(x, 11, 11, 4, 0, 0)
    assert want.shape[2] * want.shape[3] > 8192
    for name, src in _sources(x.to(dev())):
        assert torch.equal(_run_pack(src, 11, 11, 4, 0).cpu(), want), name


@pytest.mark.gpu
@pytest.mark.parametrize("case", WEIGHT_CASES)
def test_weight_pack_and_dw_unpack_kernels(case):
    K, C, R, S, st = case
    ext = ops.native()
    Rp, Sp = -(-R // st), -(-S // st)
    Kpad = _pad32(Rp * Sp * st * st * C)
    rows = _pad128(K)
    w = bf(torch.randn(K, C, R, S))
    dst = torch.zeros((rows, Kpad), dtype=torch.bfloat16, device=dev())
    ext.s2d_pack_weight(w.to(dev()), dst, K, C, R, S, st, Kpad)
    assert torch.equal(dst.cpu(), weight_ref(w, st, rows, Kpad))

    dwp = torch.randn(K, Kpad)
    want = unpack_ref(dwp, K, C, R, S, st)
    base = torch.randn(K, C, R, S)
    out = base.clone().to(dev())
    ext.dw_unpack_s2d(dwp.to(dev()), out, K, C, R, S, st, Kpad, False)
    assert torch.equal(out.cpu(), want)
    out = base.clone().to(dev())
    ext.dw_unpack_s2d(dwp.to(dev()), out, K, C, R, S, st, Kpad, True)
    assert torch.equal(out.cpu(), base + want)


@pytest.mark.gpu
@pytest.mark.parametrize("case", WEIGHT_CASES)
def test_fused_repack_descriptor(case):
    """The solver's single fused repack launch maintains the same layout
    as the stand-alone pack."""
    K, C, R, S, st = case
    Rp, Sp = -(-R // st), -(-S // st)
    Kpad = _pad32(Rp * Sp * st * st * C)
    rows = _pad128(K)
    w = bf(torch.randn(K, C, R, S))
    src = w.to(dev())
    dst = torch.zeros((rows, Kpad), dtype=torch.bfloat16, device=dev())
    table = torch.tensor([[src.data_ptr(), dst.data_ptr(), 0, K, C, R, S,
                           Kpad, 0, 0, 1, 0, st]],
                         dtype=torch.int64).to(dev())
    ops.native().repack_weights(table, 1, K * C * R * S)
    assert torch.equal(dst.cpu(), weight_ref(w, st, rows, Kpad))


# ------------------------------------------------------ GPU: whole op

def _check_op(N, C, H, W, K, R, S, st, pd, bias=True, relu=False,
              expect_s2d=True):
    x = bf(torch.randn(N, C, H, W)).to(dev())
    wt = bf(torch.randn(K, C, R, S) * 0.1).to(dev()).float()
    b = torch.randn(K).to(dev()).float() if bias else None
    ctx = {}
    y = ops.conv2d_forward(x, wt, b, (st, st), (pd, pd), (1, 1), 1,
                           ctx=ctx, relu=relu)
    assert bool(ctx.get("s2d")) == expect_s2d
    if expect_s2d:
        assert ctx["col"] is None and ctx["xl"] is None
        assert ctx["xs2d"].shape[3] == st * st * C
    x_cpu, w_cpu = x.float().cpu(), wt.cpu()
    b_cpu = b.cpu() if bias else None
    want = reference.conv2d_forward(x_cpu, w_cpu, b_cpu, (st, st),
                                    (pd, pd), (1, 1), 1, relu=relu)
    agree(y, want, rtol=0.05, atol=0.1)

    dy = bf(torch.randn_like(y.float())).to(dev())
    dx, dw, db = ops.conv2d_backward(x, wt, dy, (st, st), (pd, pd), (1, 1),
                                     1, bias=bias, ctx=ctx)
    if expect_s2d:
        assert ctx["col"] is None      # backward built no col matrix either
    rdx, rdw, rdb = reference.conv2d_backward(
        x_cpu, w_cpu, dy.float().cpu(), (st, st), (pd, pd), (1, 1), 1,
        bias=bias)
    agree(dx, rdx, rtol=0.05, atol=0.15)
    agree(dw, rdw, rtol=0.05, atol=0.3)
    if bias:
        agree(db, rdb, rtol=0.05, atol=0.3)
    else:
        assert db is None
    return ctx


OP_CASES = [
    # the pack shapes, Kout 32
    dict(N=2, C=3, H=37, W=29, K=32, R=11, S=11, st=4, pd=0),
    dict(N=2, C=3, H=35, W=35, K=32, R=11, S=11, st=4, pd=2),
    dict(N=2, C=4, H=21, W=21, K=32, R=9, S=9, st=2, pd=4),
    # R != S
    dict(N=2, C=4, H=21, W=19, K=32, R=7, S=5, st=2, pd=0),
    # NPQ=324 and Kout=264 both > 256: the 4-wave forward kernel
    dict(N=4, C=3, H=43, W=43, K=264, R=11, S=11, st=4, pd=0),
    # NPQ=1089 -> split-K 2: dw accumulates with atomics
    dict(N=9, C=3, H=51, W=51, K=32, R=11, S=11, st=4, pd=0),
    dict(N=2, C=3, H=35, W=35, K=32, R=11, S=11, st=4, pd=2, bias=False),
    dict(N=2, C=3, H=37, W=29, K=32, R=11, S=11, st=4, pd=0, relu=True),
]


@pytest.mark.gpu
@pytest.mark.parametrize("case", OP_CASES)
def test_conv_s2d_forward_backward(case, monkeypatch):
    monkeypatch.delenv("COS_S2D", raising=False)
    _check_op(**case)


@pytest.mark.gpu
def test_route_not_taken_when_ineligible(monkeypatch):
    monkeypatch.delenv("COS_S2D", raising=False)
    # st*st*C = 12: not a multiple of 8
    _check_op(N=2, C=3, H=21, W=21, K=32, R=7, S=7, st=2, pd=0,
              expect_s2d=False)


@pytest.mark.gpu
def test_route_off_switch(monkeypatch):
    monkeypatch.setenv("COS_S2D", "0")
    _check_op(N=2, C=3, H=37, W=29, K=32, R=11, S=11, st=4, pd=0,
              expect_s2d=False)


@pytest.mark.gpu
def test_dw_into_arena_bitwise(monkeypatch):
    monkeypatch.delenv("COS_S2D", raising=False)
    N, C, H, W, K, R, st = 2, 3, 37, 29, 32, 11, 4     # NPQ = 70 < 1024
    x = bf(torch.randn(N, C, H, W)).to(dev())
    wt = bf(torch.randn(K, C, R, R) * 0.1).to(dev()).float()
    ctx = {}
    y = ops.conv2d_forward(x, wt, None, (st, st), (0, 0), (1, 1), 1, ctx=ctx)
    assert ctx.get("s2d")
    dy = bf(torch.randn_like(y.float())).to(dev())
    _, dw, _ = ops.conv2d_backward(x, wt, dy, (st, st), (0, 0), (1, 1), 1,
                                   need_dx=False, bias=False, ctx=ctx)
    arena = torch.full((K, C, R, R), float("nan"), device=dev())
    _, dw2, _ = ops.conv2d_backward(x, wt, dy, (st, st), (0, 0), (1, 1), 1,
                                    need_dx=False, bias=False, ctx=ctx,
                                    dw_out=arena)
    assert dw2 is arena
    assert torch.equal(arena, dw)


@pytest.mark.gpu
def test_input_overwritten_in_place_is_repacked(monkeypatch):
    monkeypatch.delenv("COS_S2D", raising=False)
    N, C, H, W, K, R, st = 2, 3, 37, 29, 32, 11, 4
    x = bf(torch.randn(N, C, H, W)).to(dev())
    wt = bf(torch.randn(K, C, R, R) * 0.1).to(dev()).float()
    b = torch.randn(K).to(dev())
    ctx = {}
    ops.conv2d_forward(x, wt, b, (st, st), (0, 0), (1, 1), 1, ctx=ctx)
    x.copy_(bf(torch.randn(N, C, H, W)))
    y = ops.conv2d_forward(x, wt, b, (st, st), (0, 0), (1, 1), 1, ctx=ctx)
    assert ctx.get("s2d")
    want = reference.conv2d_forward(x.float().cpu(), wt.cpu(), b.cpu(),
                                    (st, st), (0, 0), (1, 1), 1)
    agree(y, want, rtol=0.05, atol=0.1)
