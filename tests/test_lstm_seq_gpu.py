"""The two whole-sequence LSTM routes (csrc/lstm_persist.hip and the
per-step driver of csrc/lstm_seq.hip) on the GPU, held step by step to the
float64 oracle and derived bounds of _lstm_seq_cases.py.  Every shape runs
on the route it is eligible for, and the route that ran is asserted: a
silent fallback fails the case instead of passing it on the other route."""

import pytest
import torch

import _lstm_seq_cases as C
from _bf16_bounds import assert_within
from caffeonspark_amd import ops
from caffeonspark_amd.core.blob import Blob
from caffeonspark_amd.core.layers.base import create_layer
from caffeonspark_amd.proto import caffe_pb, text_format

gpu = pytest.mark.gpu


def dev():
    return torch.device("cuda:0")


def _set_route(monkeypatch, forced_loop):
    monkeypatch.delenv("COS_LSTM_PERSIST", raising=False)
    if forced_loop:
        monkeypatch.setenv("COS_LSTM_PERSIST", "0")


def _settle(route):
    """A watchdog abort of the persistent kernel fails this test, not the
    one after it."""
    from caffeonspark_amd.ops import gpu as g

    torch.cuda.synchronize()
    if route == "persist":
        g._persist_check_pending(force=True)


@gpu
@pytest.mark.parametrize("run", C.RUNS, ids=C.run_id)
def test_seq_routes_within_derived_bounds(run, monkeypatch):
    shape, route, forced = run
    route = C.run_route(route, forced)
    _set_route(monkeypatch, forced)
    inp = C.inputs(*shape)
    d = dev()
    w, cont = inp["w_hc"].to(d), inp["cont"].to(d)

    fctx, bctx = {}, {}
    h, cache = ops.gpu_op("lstm_seq_forward")(inp["xg"].to(d), w, cont, fctx)
    _settle(fctx["route"])
    dxg, dwhc = ops.gpu_op("lstm_seq_backward")(inp["dy"].to(d), w, cache,
                                                bctx)
    _settle(bctx["route"])
    assert (fctx["route"], bctx["route"]) == (route, route)

    _, h_c, c, act, h_in = cache[:5]
    assert h_c is h
    out = {"h": h, "c": c, "act": act, "h_in": h_in, "dxg": dxg,
           "dwhc": dwhc}
    for name in ("h", "h_in", "dxg"):
        assert out[name].dtype == torch.bfloat16, name
    for name in ("c", "act", "dwhc"):
        assert out[name].dtype == torch.float32, name
    out = {k: v.cpu() for k, v in out.items()}
    assert_within(out, C.oracle(inp, out, route), f"lstm_seq {C.run_id(run)}")


class _GpuNet:
    phase = caffe_pb.Phase.TRAIN
    dtype = torch.bfloat16

    def __init__(self):
        self.device = dev()
        self.generator = torch.Generator().manual_seed(2)


@gpu
@pytest.mark.parametrize("forced,route", [(False, "persist"), (True, "loop")])
def test_layer_keeps_the_sequence_route(forced, route, monkeypatch):
    _set_route(monkeypatch, forced)
    T, N, D, H = 3, 4, 8, 24
    lp = text_format.parse(f'''name: "l" type: "LSTM" bottom: "x"
        bottom: "cont" top: "h"
        recurrent_param {{ num_output: {H}
          weight_filler {{ type: "uniform" min: -0.1 max: 0.1 }}
          bias_filler {{ type: "uniform" min: -0.1 max: 0.1 }} }}''',
                           caffe_pb.LayerParameter)
    layer = create_layer(lp, _GpuNet())
    cont = torch.ones(T, N)
    cont[0] = 0
    bottom = []
    for t in (torch.randn(T, N, D), cont):
        b = Blob(t.shape)
        b.data = t.to(dev(), torch.bfloat16)
        bottom.append(b)
    top = [Blob([0])]
    layer.setup(bottom, top)
    assert layer.seq_route is None
    layer.forward(bottom, top)
    assert layer.seq_route == route
    _settle(route)
    layer.seq_route = None
    top[0].diff = torch.ones_like(top[0].data)
    for b in layer.blobs:
        b.zero_diff()
    layer.backward(top, [True, False], bottom)
    assert layer.seq_route == route
    _settle(route)
    assert not torch.isnan(bottom[0].diff.float()).any()
