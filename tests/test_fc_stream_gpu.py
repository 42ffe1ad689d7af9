"""gemm_fc_kernel + fc_slab_finalize (the weight-streaming InnerProduct
route), at kernel and at layer level, against the
float64 oracle of _fc_stream_cases.py: bit-exact on the exact class, inside
the derived bound on the rounded one.

Every operand is a view inside a NaN-filled allocation (rows beyond M / N,
columns beyond K and the gap up to the leading dimension are NaN), so a read
outside an operand poisons the output.  Outputs and slabs sit in
sentinel-framed buffers; the slabs start as NaN, so a slab element the
kernel leaves unwritten reaches the output."""

import os

import pytest
import torch

import _fc_stream_cases as FC
import _gemm_bounds as GB

pytestmark = pytest.mark.gpu

from caffeonspark_amd import ops
from caffeonspark_amd.ops import gpu as G


def dev():
    return torch.device("cuda:0")


@pytest.fixture(autouse=True, scope="module")
def _native_loaded():
    ops.native()            # loads the extension behind ops.gpu's helpers


_cache = {}


def _case(name, cls):
    """(inputs, oracle) of a case: computed once, shared by both kinds."""
    key = (name, cls)
    if key not in _cache:
        c = FC.FC_CASES[name]
        seed = 900 + 2 * list(FC.FC_CASES).index(name) + \
            FC.CLASSES.index(cls)
        inp = FC.fc_inputs(c, cls, seed)
        orc, peak = FC.fc_oracle(c, inp)
        if cls == "exact":
            assert peak <= 256, "exact-class precondition"
        _cache[key] = (inp, orc)
    return _cache[key]


def _launch(c, inp, kind):
    """One gemm_fc call (+ finalize) on poisoned layouts.  Returns the
    output view on the CPU after checking every frame."""
    M, N, K = c["M"], c["N"], c["K"]
    d = dev()
    a_flat, lda = GB._operand_buf(inp["A"], False, M + 3, 8)
    b_flat, ldb = GB._operand_buf(inp["Bp"], kind == "dx", N + 5, 8)
    c_flat, _, ldc = GB.out_buf(M, N, FC.BF, GB.NAN, ld_x=8)
    _, splits = FC.split_k(K, c["sk"])
    s_flat, _, _ = GB.out_buf(1, splits * M * N, torch.float32, GB.NAN,
                              ld_x=0)
    a_flat, b_flat, c_flat, s_flat = (t.to(d) for t in
                                      (a_flat, b_flat, c_flat, s_flat))
    P = GB.PADEL
    A = a_flat[P:P + (M + 3) * lda].view(M + 3, lda)[:M, :K]
    if kind == "dx":
        B = b_flat[P:P + K * ldb].view(K, ldb)[:, :N]
    else:
        B = b_flat[P:P + (N + 5) * ldb].view(N + 5, ldb)[:N, :K]
    C = c_flat[P:P + M * ldc].view(M, ldc)[:, :N]
    slabs = s_flat[P:P + splits * M * N].view(splits, M, N)
    assert G._fc_aligned(A, B)
    plan = G.fc_gemm_plan(M, N, K, kind, True)
    assert plan[0] == "stream" and plan[1] == (128 if M <= 128 else 256)
    bias = inp["bias"].to(d) if inp["bias"] is not None else None
    G._fc_stream(A, B, C, bias, kind, c["relu"], c["sk"],
                 slabs if splits > 1 else None)
    torch.cuda.synchronize()
    cc, sc = c_flat.cpu(), s_flat.cpu()
    assert GB.outside_untouched(cc, M, N, ldc), "wrote outside the C view"
    assert GB.outside_untouched(sc, 1, splits * M * N, splits * M * N), \
        "wrote outside the slabs"
    if splits > 1:
        assert torch.isfinite(sc[P:P + splits * M * N]).all(), \
            "a slab element was left unwritten"
    return cc[P:P + M * ldc].view(M, ldc)[:, :N]


@pytest.mark.parametrize("cls", FC.CLASSES)
@pytest.mark.parametrize("kind", FC.KINDS)
@pytest.mark.parametrize("name", list(FC.FC_CASES))
def test_fc_stream(name, kind, cls):
    c = FC.FC_CASES[name]
    if kind == "dx" and c["N"] % 8:
        assert G.fc_gemm_plan(c["M"], c["N"], c["K"], "dx")[0] == "legacy"
        return
    inp, orc = _case(name, cls)
    out = _launch(c, inp, kind)
    GB.within({"out": out}, orc, f"{name}/{kind}/{cls}")


@pytest.mark.parametrize("kind", FC.KINDS)
def test_same_bits_every_run(kind):
    c = FC.fcase(256, 264, 1000, 7, True, True)
    inp = FC.fc_inputs(c, "rounded", 77)
    first = _launch(c, inp, kind)
    assert torch.equal(first, _launch(c, inp, kind))


def test_plan_gates():
    p = G.fc_gemm_plan
    assert p(256, 4096, 9216, "fwd")[0] == "stream"
    assert p(256, 1000, 4096, "fwd")[:2] == ("stream", 256)
    assert p(128, 1000, 1024, "fwd")[:2] == ("stream", 128)
    assert p(256, 4096, 1000, "dx")[0] == "stream"
    assert p(257, 16, 64, "fwd")[0] == "legacy"
    assert p(64, 16, 100, "fwd")[0] == "legacy"        # K % 8
    assert p(64, 20, 64, "dx")[0] == "legacy"          # dx: N % 8
    assert p(64, 16, 64, "fwd", False)[0] == "legacy"  # alignment
    # one wave of blocks, every split at least 256 of K, at most 16 slabs
    for M, N, K, kind in ((256, 4096, 9216, "fwd"), (256, 4096, 4096, "fwd"),
                          (256, 1000, 4096, "fwd"), (256, 9216, 4096, "dx"),
                          (256, 4096, 1000, "dx"), (64, 16, 64, "fwd")):
        sk = p(M, N, K, kind)[4]
        assert 1 <= sk <= 16 and -(-N // 128) * sk <= 256
        assert sk == 1 or K // sk >= 256
    os.environ["COS_FC_STREAM"] = "0"
    try:
        assert p(256, 4096, 9216, "fwd")[0] == "legacy"
    finally:
        del os.environ["COS_FC_STREAM"]


def _layer_oracle(x, w, b, relu):
    c = FC.fcase(x.shape[0], w.shape[0], x.shape[1], 1, b is not None, relu)
    inp = dict(A=x.float(), Bp=w.float(), bias=b, cls="rounded")
    return FC.fc_oracle(c, inp)[0]


DECLINED = {
    "m257": dict(M=257, N=16, K=64),
    "k_not_8": dict(M=64, N=16, K=100),
    "misaligned_base": dict(M=64, N=72, K=104, misalign=True),
    "transposed_w": dict(M=64, N=72, K=104, transposed=True),
}


@pytest.mark.parametrize("name", list(DECLINED))
def test_declined_shapes_keep_the_legacy_route(name):
    """What the streaming kernel cannot take runs as before, and right."""
    dc = DECLINED[name]
    M, N, K = dc["M"], dc["N"], dc["K"]
    g = FC.gen(31)
    x = FC.rb(torch.randn((M, K), generator=g) + 0.25)
    w = FC.rb(torch.randn((N, K), generator=g) * 0.5)
    b = torch.randn((N,), generator=g)
    orc = _layer_oracle(x, w, b, True)
    d = dev()
    if dc.get("misalign"):
        # K = 104 keeps the legacy GEMM on its guarded loads
        xd = torch.zeros(M * K + 8, dtype=FC.BF, device=d)[1:1 + M * K] \
            .view(M, K)
        xd.copy_(x)
    else:
        xd = x.to(d).to(FC.BF)
    wd = w.to(d).to(FC.BF)
    if dc.get("transposed"):
        wd = wd.t().contiguous().t()         # [N, K] view of a [K][N] matrix
    assert G.fc_gemm_plan(M, N, K, "fwd", G._fc_aligned(xd, wd))[0] == \
        "legacy"
    y = G.fc_forward(xd, wd, b.to(d), relu=True)
    torch.cuda.synchronize()
    GB.within({"out": y.cpu()}, orc, name)


def test_no_weight_copies():
    """Peak memory over a forward call at N = 200, K = 104 and over a dx
    call stays within the output plus the slab workspace: neither a padded
    nor a transposed copy of W is made."""
    d = dev()
    M, N, K = 64, 200, 104
    g = FC.gen(5)
    x = torch.randn((M, K), generator=g).to(d).to(FC.BF)
    w = torch.randn((N, K), generator=g).to(d).to(FC.BF)
    b = torch.randn((N,), generator=g).to(d)
    dy = torch.randn((M, N), generator=g).to(d).to(FC.BF)
    dw = torch.empty((N, K), dtype=torch.float32, device=d)
    G._zpage(d)
    slack = 4 * 512                          # the allocator's rounding
    sk = G.fc_gemm_plan(M, N, K, "fwd")[4]
    assert G.fc_gemm_plan(M, N, K, "fwd")[0] == "stream"
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    y = G.fc_forward(x, w, b, relu=True)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    assert peak <= y.numel() * 2 + (sk * M * N * 4 if sk > 1 else 0) + slack
    assert torch.cuda.memory_allocated() - base <= y.numel() * 2 + slack

    assert G.fc_gemm_plan(M, K, N, "dx")[0] == "stream"
    sk = G.fc_gemm_plan(M, K, N, "dx")[4]
    G.begin_backward()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    dx, _, _ = G.fc_backward(x, w, dy, need_dx=True, bias=False, dw_out=dw)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    assert peak <= dx.numel() * 2 + (sk * M * K * 4 if sk > 1 else 0) + slack


@pytest.mark.parametrize("M,N,K", [(64, 200, 104), (256, 264, 328)])
def test_layer_stream_against_legacy(M, N, K):
    """fc_forward / fc_backward with COS_FC_STREAM 1 and 0: y, dx and db
    inside the derived bound of the common float64 oracle, dW the same
    bits (its GEMM does not depend on the route)."""
    d = dev()
    g = FC.gen(1000 + M)
    x = FC.rb(torch.randn((M, K), generator=g) + 0.25)
    w = FC.rb(torch.randn((N, K), generator=g) * 0.5)
    b = torch.randn((N,), generator=g)
    dy = FC.rb(torch.randn((M, N), generator=g))
    y_orc = _layer_oracle(x, w, b, True)
    dx_orc = _layer_oracle(dy, w.t().contiguous(), None, False)
    db_want = dy.double().sum(dim=0)
    db_tol = (2 * M + 4) * FC.E32 * dy.double().abs().sum(dim=0)
    xd, wd, dyd = (t.to(d).to(FC.BF) for t in (x, w, dy))
    got = {}
    for env in ("1", "0"):
        os.environ["COS_FC_STREAM"] = env
        try:
            want_route = "stream" if env == "1" else "legacy"
            assert G.fc_gemm_plan(M, N, K, "fwd")[0] == want_route
            assert G.fc_gemm_plan(M, K, N, "dx")[0] == want_route
            G.begin_backward()
            y = G.fc_forward(xd, wd, b.to(d), relu=True)
            dx, dw, db = G.fc_backward(xd, wd, dyd)
            torch.cuda.synchronize()
            got[env] = tuple(t.cpu().clone() for t in (y, dx, dw, db))
        finally:
            del os.environ["COS_FC_STREAM"]
    for env, (y, dx, dw, db) in got.items():
        GB.within({"out": y}, y_orc, f"y stream={env}")
        GB.within({"out": dx}, dx_orc, f"dx stream={env}")
        GB.within({"db": db}, {"db": (db_want, db_tol)}, f"db stream={env}")
    assert torch.equal(got["1"][2], got["0"][2])
