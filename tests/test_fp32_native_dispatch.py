"""Routing of the fp32 GPU path between the native `<op>_f32` entries and
the reference impls, exercised on the CPU: the GPU test and the extension
load are patched out, and fake `_f32` entries return a sentinel."""

import pytest
import torch

from caffeonspark_amd import ops
from caffeonspark_amd.ops import dispatcher

_SENTINEL = object()


class _Fake:
    def __init__(self):
        self.calls = 0

    def __call__(self, *a, **k):
        self.calls += 1
        return _SENTINEL


@pytest.fixture
def fakes(monkeypatch):
    monkeypatch.setattr(ops, "_args_on_gpu", lambda args: True)
    monkeypatch.setattr(ops, "native", lambda: None)
    f = {"conv2d_forward_f32": _Fake(), "fc_forward_f32": _Fake()}
    for name, fn in f.items():
        monkeypatch.setitem(dispatcher.gpu_impls, name, fn)
    try:
        yield f
    finally:
        ops.set_active_gpu_mode(None)


def _fc_args(dtype=torch.float32):
    return torch.ones(2, 3, dtype=dtype), torch.ones(4, 3, dtype=dtype), None


def _conv_args():
    return (torch.ones(1, 2, 4, 4), torch.ones(3, 2, 3, 3), None, (1, 1),
            (0, 0), (1, 1), 1)


def test_native_set_is_the_four_gemm_ops():
    assert ops._FP32_NATIVE_ON_GPU == {"conv2d_forward", "conv2d_backward",
                                       "fc_forward", "fc_backward"}
    assert ops._FP32_NATIVE_ON_GPU <= ops._FP32_REF_ON_GPU


def test_fp32_mode_native_selected(fakes, monkeypatch):
    monkeypatch.setenv("COS_FP32_NATIVE", "1")
    ops.set_active_gpu_mode("fp32")
    assert ops.fc_forward(*_fc_args()) is _SENTINEL
    assert ops.conv2d_forward(*_conv_args()) is _SENTINEL
    assert fakes["fc_forward_f32"].calls == 1
    assert fakes["conv2d_forward_f32"].calls == 1


def test_fp32_mode_library_selected(fakes, monkeypatch):
    monkeypatch.setenv("COS_FP32_NATIVE", "0")
    ops.set_active_gpu_mode("fp32")
    y = ops.fc_forward(*_fc_args())
    assert torch.equal(y, torch.full((2, 4), 3.0))
    y = ops.conv2d_forward(*_conv_args())
    assert torch.equal(y, torch.full((1, 3, 2, 2), 18.0))
    assert all(f.calls == 0 for f in fakes.values())


def test_env_is_read_per_call(fakes, monkeypatch):
    ops.set_active_gpu_mode("fp32")
    monkeypatch.setenv("COS_FP32_NATIVE", "1")
    assert ops.fc_forward(*_fc_args()) is _SENTINEL
    monkeypatch.setenv("COS_FP32_NATIVE", "0")
    assert ops.fc_forward(*_fc_args()) is not _SENTINEL
    monkeypatch.setenv("COS_FP32_NATIVE", "1")
    assert ops.fc_forward(*_fc_args()) is _SENTINEL


def test_bf16_mode_never_consults_f32_entry(fakes, monkeypatch):
    monkeypatch.setenv("COS_FP32_NATIVE", "1")
    bf16_fc = _Fake()
    monkeypatch.setitem(dispatcher.gpu_impls, "fc_forward", bf16_fc)
    ops.set_active_gpu_mode("bf16")
    assert ops.fc_forward(*_fc_args()) is _SENTINEL
    assert bf16_fc.calls == 1
    assert fakes["fc_forward_f32"].calls == 0


def test_other_ops_stay_on_reference(fakes, monkeypatch):
    monkeypatch.setenv("COS_FP32_NATIVE", "1")
    relu32 = _Fake()
    monkeypatch.setitem(dispatcher.gpu_impls, "relu_forward_f32", relu32)
    ops.set_active_gpu_mode("fp32")
    y = ops.relu_forward(torch.tensor([-1.0, 2.0]))
    assert torch.equal(y, torch.tensor([0.0, 2.0]))
    assert relu32.calls == 0


def test_sniff_route(fakes, monkeypatch):
    monkeypatch.setenv("COS_FP32_NATIVE", "1")
    ops.set_active_gpu_mode(None)
    assert ops.fc_forward(*_fc_args()) is _SENTINEL
    assert fakes["fc_forward_f32"].calls == 1
    # a bf16 tensor sends the call to the bf16 entry, not the _f32 one
    bf16_fc = _Fake()
    monkeypatch.setitem(dispatcher.gpu_impls, "fc_forward", bf16_fc)
    assert ops.fc_forward(*_fc_args(torch.bfloat16)) is _SENTINEL
    assert bf16_fc.calls == 1
    assert fakes["fc_forward_f32"].calls == 1


def test_unregistered_f32_entry_falls_through(fakes, monkeypatch):
    monkeypatch.setenv("COS_FP32_NATIVE", "1")
    monkeypatch.delitem(dispatcher.gpu_impls, "fc_forward_f32")
    ops.set_active_gpu_mode("fp32")
    y = ops.fc_forward(*_fc_args())
    assert torch.equal(y, torch.full((2, 4), 3.0))
