"""The fused LSTM decode-step kernel and the stateful / expose_hidden layer
on the GPU.  The kernel is held to the float64 oracle and derived bounds of
_lstm_step_cases.py; routes and layers to the CPU fp32 layer at the
tolerances of test_lstm_layer_gpu_parity."""

import os

import numpy as np
import pytest
import torch

import _lstm_step_cases as C
from _bf16_bounds import assert_within, violations
from caffeonspark_amd import ops
from caffeonspark_amd.core.blob import Blob
from caffeonspark_amd.core.layers.base import create_layer
from caffeonspark_amd.core.net import Net
from caffeonspark_amd.proto import caffe_pb, text_format

gpu = pytest.mark.gpu
FIXTURE = os.path.join(os.path.dirname(__file__), "golden", "reference",
                       "data", "lrcn_word_to_preds.deploy.prototxt")
# test_lstm_layer_gpu_parity's forward / dx tolerances
FWD = dict(rtol=0.05, atol=0.03)
DX = dict(rtol=0.08, atol=0.05)


def dev():
    return torch.device("cuda:0")


def agree(got, want, rtol, atol):
    torch.testing.assert_close(got.float().cpu(), want.float().cpu(),
                               rtol=rtol, atol=atol)


# ------------------------------------------------- the bounds do not pass
# vacuously (CPU): the kernel's arithmetic fits, mutants do not

@pytest.mark.parametrize("case", C.CASES, ids=str)
def test_step_bounds_hold_for_the_emulation_and_catch_mutants(case):
    inp = C.inputs(*case)
    orc = C.oracle(inp)
    assert not violations(C.emulate(inp), orc)
    N, D, H, Ds = case
    if N > 1:
        # streams with cont = 0 over a non-zero previous state
        assert violations(C.emulate(inp, ignore_cont=True), orc)
    if inp["K"] <= 1024:
        # rounding pre to bf16 costs up to 2^-9 |pre|; the accumulation
        # bound (K+4) e sum|terms| stays below that up to K of about a
        # thousand.  At the LRCN shape (K = 3000) the bound the
        # accumulation is entitled to is itself a bf16 ulp wide, so this
        # mutant is only told apart at the three smaller shapes.
        assert violations(C.emulate(inp, round_pre=True), orc)


# --------------------------------------------------- kernel vs the oracle

def _run_kernel(inp):
    d = dev()

    def g(name):
        return None if inp[name] is None else inp[name].to(d)

    assert ops.gpu_op("lstm_step_ok")(
        inp["x"].shape[0], inp["x"].shape[1], inp["h_prev"].shape[1],
        0 if inp["xs"] is None else inp["xs"].shape[1])
    h, c = ops.gpu_op("lstm_step")(
        g("x"), g("h_prev"), g("c_prev"), g("cont"), g("w_xc"), g("b"),
        g("w_hc"), g("xs"), g("w_xsc"))
    torch.cuda.synchronize()
    return {"c": c, "h": h}


# beyond the four shapes above: full N at the LRCN lengths, whose 96 KB
# panel takes the opt-in (> 64 KB) dynamic LDS path
BIG_PANEL = (16, 1000, 1000, 1000)


@gpu
@pytest.mark.parametrize("case", C.CASES + [BIG_PANEL], ids=str)
def test_step_kernel_within_derived_bounds(case):
    inp = C.inputs(*case)
    out = _run_kernel(inp)
    assert out["h"].dtype == torch.bfloat16
    assert out["c"].dtype == torch.float32
    assert_within(out, C.oracle(inp), f"lstm_step {case}")


# ------------------------------------------------------------ layer level

class _CpuNet:
    phase = caffe_pb.Phase.TEST
    dtype = torch.float32
    device = torch.device("cpu")

    def __init__(self):
        self.generator = torch.Generator().manual_seed(2)


class _GpuNet(_CpuNet):
    dtype = torch.bfloat16

    def __init__(self):
        super().__init__()
        self.device = dev()


def _layer_text(H, static, expose):
    return f'''name: "l" type: "LSTM" bottom: "x" bottom: "cont"
        {'bottom: "xs"' if static else ''}
        {'bottom: "h0" bottom: "c0"' if expose else ''}
        top: "h" {'top: "hT" top: "cT"' if expose else ''}
        recurrent_param {{ num_output: {H}
          {'expose_hidden: true' if expose else ''}
          weight_filler {{ type: "uniform" min: -0.1 max: 0.1 }}
          bias_filler {{ type: "uniform" min: -0.1 max: 0.1 }} }}'''


def _blobs(tensors, device, dtype):
    out = []
    for t in tensors:
        b = Blob(t.shape)
        b.data = t.to(device, dtype)
        out.append(b)
    return out


class _Pair:
    """The same LSTM layer on CPU fp32 and GPU bf16, same weights."""

    def __init__(self, N, D, H, Ds=0, expose=False, stateful=True, T=1):
        lp = text_format.parse(_layer_text(H, Ds > 0, expose),
                               caffe_pb.LayerParameter)
        self.cpu, self.gpu = create_layer(lp, _CpuNet()), \
            create_layer(lp, _GpuNet())
        self.N, self.D, self.H, self.Ds, self.expose = N, D, H, Ds, expose
        ntop = 3 if expose else 1
        self.ctop = [Blob([0]) for _ in range(ntop)]
        self.gtop = [Blob([0]) for _ in range(ntop)]
        z = self.inputs(torch.Generator().manual_seed(0), T)
        self.cpu.setup(_blobs(z, self.cpu.device, torch.float32), self.ctop)
        self.gpu.setup(_blobs(z, dev(), torch.bfloat16), self.gtop)
        for cb, gb in zip(self.cpu.blobs, self.gpu.blobs):
            gb.data.copy_(cb.data.to(dev()))
        self.cpu.stateful = self.gpu.stateful = stateful and not expose

    def inputs(self, g, T=1, cont=None):
        N = self.N
        ins = [torch.randn(T, N, self.D, generator=g),
               torch.ones(T, N) if cont is None else cont]
        if self.Ds:
            ins.append(torch.randn(N, self.Ds, generator=g))
        if self.expose:
            ins += [torch.randn(1, N, self.H, generator=g) * 0.5,
                    torch.randn(1, N, self.H, generator=g) * 0.5]
        return ins

    def forward(self, ins):
        self.cbot = _blobs(ins, self.cpu.device, torch.float32)
        self.gbot = _blobs(ins, dev(), torch.bfloat16)
        self.cpu.forward(self.cbot, self.ctop)
        self.gpu.forward(self.gbot, self.gtop)


def _cont_pattern(t, N):
    cont = torch.ones(1, N)
    if t == 0:
        cont[:] = 0
    elif t == 3 and N > 1:
        cont[0, 1] = 0              # stream 1 restarts
    return cont


ROUTES = [
    # N, D, H, Ds, env, route
    (1, 8, 8, 0, {}, "fused"),
    (3, 520, 24, 0, {}, "fused"),
    (16, 64, 136, 8, {}, "fused"),
    (16, 2048, 1024, 1024, {}, "fused"),             # panel = 128 KB budget
    (16, 2056, 1024, 1024, {}, "gemm"),              # panel beyond it
    (17, 64, 136, 8, {}, "gemm"),                    # N > MAXN
    (4, 12, 16, 0, {}, "gemm"),                      # D % 8 != 0
    (4, 64, 16, 8, {"COS_LSTM_STEP": "0"}, "gemm"),  # switched off
    (4, 64, 16, 8, {"COS_LSTM_STEP_MAXN": "2"}, "gemm"),
]


@gpu
@pytest.mark.parametrize("N,D,H,Ds,env,route", ROUTES)
def test_step_routes_and_agreement_with_cpu(N, D, H, Ds, env, route,
                                            monkeypatch):
    for k in ("COS_LSTM_STEP", "COS_LSTM_STEP_MAXN"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    p = _Pair(N, D, H, Ds)
    g = torch.Generator().manual_seed(5)
    for t in range(3):
        p.forward(p.inputs(g, cont=_cont_pattern(t, N)))
        assert p.gpu.step_route == route
        assert p.cpu.step_route == "gemm"
        agree(p.gtop[0].data, p.ctop[0].data, **FWD)


@gpu
def test_six_stateful_steps_and_tops_stay():
    p = _Pair(4, 64, 24, 8)
    e = _Pair(4, 64, 24, 8, expose=True)
    for cb, eb in zip(p.gpu.blobs, e.gpu.blobs):
        eb.data.copy_(cb.data)
    g = torch.Generator().manual_seed(6)
    N, H = 4, 24
    h = torch.zeros(1, N, H, device=dev(), dtype=torch.bfloat16)
    c = torch.zeros(1, N, H, device=dev())
    kept = []                        # (tensor handed out, its value then)
    for t in range(6):
        ins = p.inputs(g, cont=_cont_pattern(t, N))
        p.forward(ins)
        assert p.gpu.step_route == "fused"
        agree(p.gtop[0].data, p.ctop[0].data, **FWD)
        assert p.gtop[0].data.dtype == torch.bfloat16
        assert p.gpu._state[1].dtype == torch.float32
        # exposed stepping, fed its own h_T / c_T, is the same computation
        ebot = [b for b in p.gbot] + _blobs([h], dev(), torch.bfloat16) \
            + _blobs([c], dev(), torch.float32)
        e.gpu.forward(ebot, e.gtop)
        assert e.gpu.step_route == "fused"
        assert torch.equal(e.gtop[0].data, p.gtop[0].data), f"step {t}"
        h, c = e.gtop[1].data, e.gtop[2].data
        assert c.dtype == torch.float32
        assert torch.equal(c[0], p.gpu._state[1])
        # tops of steps t-1 and t-2 still hold what they held
        for earlier in kept[-2:]:
            for top, val in earlier:
                assert torch.equal(top, val)
        kept.append([(x, x.clone()) for x in (p.gtop[0].data, h, c)])


@gpu
def test_expose_hidden_forward_backward_gpu_vs_cpu(monkeypatch):
    monkeypatch.delenv("COS_LSTM_STEP", raising=False)
    T, N, D, H = 5, 4, 12, 16
    p = _Pair(N, D, H, expose=True, T=T)
    g = torch.Generator().manual_seed(8)
    cont = torch.ones(T, N)
    cont[0, 0] = 0
    cont[3, 2] = 0
    p.forward(p.inputs(g, T, cont))
    assert p.gpu.step_route == "gemm"
    for gt, ct in zip(p.gtop, p.ctop):
        agree(gt.data, ct.data, **FWD)
    assert p.gtop[2].data.dtype == torch.float32
    diffs = [torch.randn(T, N, H, generator=g),
             torch.randn(1, N, H, generator=g),
             torch.randn(1, N, H, generator=g)]
    for i, d in enumerate(diffs):
        p.ctop[i].diff = d.clone()
        p.gtop[i].diff = d.to(dev(), p.gtop[i].data.dtype)
    for layer in (p.cpu, p.gpu):
        for b in layer.blobs:
            b.zero_diff()
    prop = [True, False, True, True]
    p.cpu.backward(p.ctop, prop, p.cbot)
    p.gpu.backward(p.gtop, prop, p.gbot)
    for i in (0, 2, 3):              # dx, d h_0, d c_0
        agree(p.gbot[i].diff, p.cbot[i].diff, **DX)
    for i, (cb, gb) in enumerate(zip(p.cpu.blobs, p.gpu.blobs)):
        rel = (cb.diff.float() - gb.diff.float().cpu()).norm() / \
            cb.diff.float().norm().clamp_min(1e-4)
        assert rel < 0.1, f"param {i} relL2={rel:.3f}"


@gpu
def test_stateful_and_fused_backward_raise():
    p = _Pair(2, 8, 8)
    p.forward(p.inputs(torch.Generator().manual_seed(1)))
    p.gtop[0].diff = torch.ones_like(p.gtop[0].data)
    with pytest.raises(RuntimeError, match="stateful"):
        p.gpu.backward(p.gtop, [True, False], p.gbot)
    e = _Pair(2, 8, 8, expose=True)
    e.forward(e.inputs(torch.Generator().manual_seed(1)))
    assert e.gpu.step_route == "fused"
    for t in e.gtop:
        t.diff = torch.ones_like(t.data)
    with pytest.raises(RuntimeError, match="COS_LSTM_STEP=0"):
        e.gpu.backward(e.gtop, [True, False, True, True], e.gbot)


@gpu
def test_train_phase_exposed_step_keeps_its_backward():
    """An expose_hidden T=1 step of a TRAIN-phase net stays on the per-step
    ops, so its backward has a cache to read."""
    e = _Pair(2, 8, 8, expose=True)
    e.gpu.phase = caffe_pb.Phase.TRAIN
    e.forward(e.inputs(torch.Generator().manual_seed(1)))
    assert e.gpu.step_route == "gemm"
    for tops in (e.ctop, e.gtop):
        for t in tops:
            t.diff = torch.ones_like(t.data)
    prop = [True, False, True, True]
    e.cpu.backward(e.ctop, prop, e.cbot)
    e.gpu.backward(e.gtop, prop, e.gbot)
    for i in (0, 2, 3):
        agree(e.gbot[i].diff, e.cbot[i].diff, **DX)


# --------------------------------------------------------------- deploy net

@gpu
def test_deploy_net_steps_on_gpu_vs_cpu():
    """lrcn_word_to_preds.deploy.prototxt, 2 streams, 3 tokens: probs per
    step against the CPU fp32 net.  Tokens are not compared across dtypes
    (an arg-max may flip)."""
    param = text_format.parse_file(FIXTURE, caffe_pb.NetParameter)
    state = caffe_pb.NetState(phase=caffe_pb.Phase.TEST)
    cpu = Net(param, state)
    gnet = Net(param, state, device=dev(), dtype=torch.bfloat16)
    rng = np.random.RandomState(3)
    for cl, gl in zip(cpu.layers, gnet.layers):
        for cb, gb in zip(cl.blobs, gl.blobs):
            w = torch.from_numpy(rng.uniform(
                -0.05, 0.05, size=tuple(cb.shape)).astype(np.float32))
            cb.data.copy_(w)
            gb.data.copy_(w.to(dev()))
    cpu.set_recurrent_stateful(True)
    gnet.set_recurrent_stateful(True)
    N = 2
    feats = torch.from_numpy(rng.uniform(-1, 1, (N, 1000)).astype(np.float32))
    for t in range(3):
        cont = torch.full((1, N), 0.0 if t == 0 else 1.0)
        words = torch.from_numpy(
            rng.randint(0, 8801, size=(1, N)).astype(np.float32))
        for net in (cpu, gnet):
            d, dt = net.device, net.dtype
            net.blob_by_name("cont_sentence").data = cont.to(d, dt)
            # ids stay fp32: bf16 cannot hold a 4-digit index
            net.blob_by_name("input_sentence").data = words.to(d)
            net.blob_by_name("image_features").data = feats.to(d, dt)
            net.forward()
        for name in ("lstm1", "lstm2"):
            assert gnet.layer_by_name(name).step_route == "fused"
            agree(gnet.blob_by_name(name).data, cpu.blob_by_name(name).data,
                  **FWD)
        agree(gnet.blob_by_name("probs").data, cpu.blob_by_name("probs").data,
              **FWD)
