"""_dwc_ok (ops/gpu.py), the gate of the direct depthwise kernels, as a truth
table, and a depthwise + pointwise pair built from prototxt through Net on
the CPU path against autograd.  CPU only."""

import pytest
import torch
import torch.nn.functional as F

from caffeonspark_amd.core.net import Net
from caffeonspark_amd.ops import gpu as G
from caffeonspark_amd.proto import caffe_pb, text_format

# (C, Kout, G, Cg, R, S, aligned, COS_DWC) -> taken
GATE = {
    "mobilenet_3x3": ((32, 32, 32, 1, 3, 3, True, None), True),
    "7x7": ((8, 8, 8, 1, 7, 7, True, None), True),
    "3x5_env_1": ((16, 16, 16, 1, 3, 5, True, "1"), True),
    "multiplier_2": ((8, 16, 8, 1, 3, 3, True, None), False),
    "c12": ((12, 12, 12, 1, 3, 3, True, None), False),
    "c6_deconv_case": ((6, 6, 6, 1, 4, 4, True, None), False),
    "r9": ((8, 8, 8, 1, 9, 3, True, None), False),
    "s9": ((8, 8, 8, 1, 3, 9, True, None), False),
    "two_groups": ((16, 16, 2, 8, 3, 3, True, None), False),
    "dense": ((8, 8, 1, 8, 3, 3, True, None), False),
    "unaligned_stride": ((8, 8, 8, 1, 3, 3, False, None), False),
    "cos_dwc_0": ((32, 32, 32, 1, 3, 3, True, "0"), False),
}


@pytest.mark.parametrize("name", list(GATE))
def test_dwc_gate(name, monkeypatch):
    (*args, env), want = GATE[name]
    if env is None:
        monkeypatch.delenv("COS_DWC", raising=False)
    else:
        monkeypatch.setenv("COS_DWC", env)
    assert G._dwc_ok(*args) is want


NET = """
layer { name: "data" type: "DummyData" top: "data"
        dummy_data_param { shape { dim: 2 dim: 8 dim: 6 dim: 6 }
                           data_filler { type: "gaussian" std: 1.0 } } }
layer { name: "lab" type: "DummyData" top: "lab"
        dummy_data_param { shape { dim: 2 } } }
layer { name: "dw" type: "Convolution" bottom: "data" top: "dw"
        convolution_param { num_output: 8 group: 8 kernel_size: 3 pad: 1
          weight_filler { type: "gaussian" std: 0.3 }
          bias_filler { type: "constant" value: 0.1 } } }
layer { name: "pw" type: "Convolution" bottom: "dw" top: "pw"
        convolution_param { num_output: 4 kernel_size: 1
          weight_filler { type: "gaussian" std: 0.3 } } }
layer { name: "gap" type: "Pooling" bottom: "pw" top: "gap"
        pooling_param { pool: AVE global_pooling: true } }
layer { name: "loss" type: "SoftmaxWithLoss" bottom: "gap" bottom: "lab"
        top: "loss" }
"""


def test_depthwise_pointwise_net_cpu():
    param = text_format.parse(NET, caffe_pb.NetParameter)
    net = Net(param, caffe_pb.NetState(phase=caffe_pb.Phase.TRAIN), seed=3)
    loss = net.forward()
    net.backward()
    dw, pw = net.layer_by_name("dw"), net.layer_by_name("pw")
    assert list(dw.blobs[0].data.shape) == [8, 1, 3, 3]
    x = net.blob_by_name("data").data.double()
    lab = net.blob_by_name("lab").data.long()
    w = dw.blobs[0].data.double().requires_grad_(True)
    h = F.conv2d(x, w, dw.blobs[1].data.double(), padding=1, groups=8)
    z = F.conv2d(h, pw.blobs[0].data.double(), pw.blobs[1].data.double())
    ref = F.cross_entropy(z.mean(dim=(2, 3)), lab)
    ref.backward()
    assert abs(loss - ref.item()) < 1e-5
    torch.testing.assert_close(dw.blobs[0].diff.double(), w.grad,
                               rtol=1e-4, atol=1e-6)
