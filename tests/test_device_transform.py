"""Device-side DataTransformer, CPU part: `transform_device` on the CPU
device runs the torch reference op behind `ops.data_transform`, so the
plumbing (packing, table, shared random draws, feed path, flag) is checked
here against the host transformer, bit for bit."""

import numpy as np
import pytest
import torch

import _xform_cases as xc
from caffeonspark_amd.api.config import Config
from caffeonspark_amd.data.transformer import DataTransformer
from caffeonspark_amd.proto import caffe_pb

CPU = torch.device("cpu")


@pytest.mark.parametrize("planar", [True, False])
@pytest.mark.parametrize("c", [1, 3])
def test_matches_host_transform(tmp_path, c, planar):
    imgs = xc.images(c, [(xc.H, xc.W)] * 4)
    raw = [xc.planar_of(im) for im in imgs] if planar else imgs
    for mean, scale, crop, phase in xc.MATRIX:
        host = xc.transformer(tmp_path, c, mean, scale, crop, phase)
        dev = xc.transformer(tmp_path, c, mean, scale, crop, phase)
        want = host.transform(imgs)
        got = dev.transform_device(raw, CPU, torch.float32, planar=planar)
        assert got.dtype == torch.float32 and got.shape == want.shape
        assert torch.equal(got, want), (mean, scale, crop, phase)
        # bf16 output is the host result rounded once
        dev16 = xc.transformer(tmp_path, c, mean, scale, crop, phase)
        got16 = dev16.transform_device(raw, CPU, torch.bfloat16,
                                       planar=planar)
        assert torch.equal(got16, want.to(torch.bfloat16))


def test_ragged_batch_matches_transform_one():
    sizes = [(37, 41), (29, 29), (64, 30)]
    imgs = xc.images(3, sizes)
    tp = caffe_pb.TransformationParameter(
        crop_size=xc.CROP, mirror=True, mean_value=[104.5, 117.25, 123.0],
        scale=0.017)
    host = DataTransformer(tp, caffe_pb.Phase.TRAIN, seed=xc.SEED)
    dev = DataTransformer(tp, caffe_pb.Phase.TRAIN, seed=xc.SEED)
    want = torch.from_numpy(np.stack([host.transform_one(im)
                                      for im in imgs]))
    # mixed layouts in one batch as well
    flags = [True, False, True]
    raw = [xc.planar_of(im) if p else im for im, p in zip(imgs, flags)]
    got = dev.transform_device(raw, CPU, torch.float32, planar=flags)
    assert got.shape == (3, 3, xc.CROP, xc.CROP)
    assert torch.equal(got, want)


@pytest.mark.parametrize("crop", [0, xc.CROP])
def test_rng_state_identical_after_either_path(crop):
    imgs = xc.images(3, [(xc.H, xc.W)] * 5)
    tp = caffe_pb.TransformationParameter(crop_size=crop, mirror=True)
    host = DataTransformer(tp, caffe_pb.Phase.TRAIN, seed=xc.SEED)
    dev = DataTransformer(tp, caffe_pb.Phase.TRAIN, seed=xc.SEED)
    host.transform(imgs)
    dev.transform_device(imgs, CPU, torch.float32)
    hs, ds = host.rng.get_state(), dev.rng.get_state()
    assert hs[0] == ds[0] and np.array_equal(hs[1], ds[1])
    assert hs[2:] == ds[2:]
    assert host.rng.randint(1 << 30) == dev.rng.randint(1 << 30)


def test_value_errors(tmp_path):
    tp = caffe_pb.TransformationParameter()
    with pytest.raises(ValueError, match="differ in size"):
        DataTransformer(tp, seed=0).transform_device(
            xc.images(3, [(37, 41), (37, 40)]), CPU, torch.float32)
    tp = caffe_pb.TransformationParameter(crop_size=xc.CROP)
    with pytest.raises(ValueError, match="smaller than crop"):
        DataTransformer(tp, seed=0).transform_device(
            xc.images(3, [(37, 41), (28, 41)]), CPU, torch.float32)
    xf = xc.transformer(tmp_path, 3, "file", 1.0, xc.CROP,
                        caffe_pb.Phase.TRAIN)
    with pytest.raises(ValueError, match="mean file shape"):
        xf.transform_device(xc.images(3, [(37, 41), (37, 42)]), CPU,
                            torch.float32)


def test_reference_op_checks_bounds():
    from caffeonspark_amd import ops
    src = torch.zeros(3 * 8 * 8, dtype=torch.uint8)
    for row in ([0, 8, 8, 1, 5, 0, 0],      # h_off + oh > H
                [0, 8, 8, 1, 0, 5, 0],      # w_off + ow > W
                [1, 8, 8, 1, 0, 0, 0]):     # bytes past the end of src
        with pytest.raises(ValueError):
            ops.data_transform(src, torch.tensor([row]), None, 0, 1.0, 3,
                               4, 4, torch.float32, False)


def test_config_flag():
    assert Config([]).transform_on_device is False
    assert Config(["-transform_on_device"]).transform_on_device is True
    from com.yahoo.ml.caffe.Config import Config as MirrorConfig
    conf = MirrorConfig(None, ["-transform_on_device"])
    assert conf.transform_on_device is True
    # executors re-parse raw_args
    assert Config(conf.raw_args).transform_on_device is True


@pytest.mark.parametrize("c,mean,crop", [(3, "file", xc.CROP),
                                         (1, "value", 0)])
def test_image_source_flag_on_equals_off(tmp_path, c, mean, crop):
    """Raw planar and PNG samples through next_batch, batch 4 over 10
    samples (so the last batch is partial), flag on vs off."""
    tp = xc.transform_param(tmp_path, c, mean, 1.0 / 256, crop, True)
    off = xc.image_source(tp, c, 4, False)
    on = xc.image_source(tp, c, 4, True)
    smps = xc.samples(c, 10)
    xc.feed(off, smps)
    xc.feed(on, smps)
    sizes = []
    while True:
        a = off.next_batch(CPU, torch.float32)
        b = on.next_batch(CPU, torch.float32)
        if a is None:
            assert b is None
            break
        assert a[0].dtype == b[0].dtype == torch.float32
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        sizes.append(a[0].shape[0])
    assert sizes == [4, 4, 2]


def test_float_sample_batch_takes_host_path():
    from caffeonspark_amd.data.lmdb_source import FloatSample
    tp = caffe_pb.TransformationParameter(scale=0.5)
    srcs = [xc.image_source(tp, 1, 2, flag, hw=(4, 4))
            for flag in (False, True)]
    vals = np.arange(16, dtype=np.float32) / 3
    got = []
    for s in srcs:
        xc.feed(s, [FloatSample("a", 1, 1, 4, 4, vals.tobytes()),
                    xc.samples(1, 1, hw=(4, 4))[0]])
        got.append(s.next_batch(CPU, torch.float32))
    assert torch.equal(got[0][0], got[1][0])


_LENET_NET = """
name: "LeNet"
layer {{
  name: "data" type: "MemoryData" top: "data" top: "label"
  include {{ phase: TRAIN }}
  source_class: "com.yahoo.ml.caffe.LMDB"
  memory_data_param {{ source: "{train}" batch_size: 32
                       channels: 1 height: 28 width: 28 }}
  transform_param {{ scale: 0.00390625 mean_value: 128 mirror: true }}
}}
layer {{ name: "conv1" type: "Convolution" bottom: "data" top: "conv1"
  convolution_param {{ num_output: 8 kernel_size: 5
    weight_filler {{ type: "xavier" }} }} }}
layer {{ name: "pool1" type: "Pooling" bottom: "conv1" top: "pool1"
  pooling_param {{ pool: MAX kernel_size: 2 stride: 2 }} }}
layer {{ name: "ip1" type: "InnerProduct" bottom: "pool1" top: "ip1"
  inner_product_param {{ num_output: 10
    weight_filler {{ type: "xavier" }} }} }}
layer {{ name: "loss" type: "SoftmaxWithLoss" bottom: "ip1" bottom: "label"
  top: "loss" }}
"""

_SOLVER = """
net: "{net}"
base_lr: 0.01
momentum: 0.9
lr_policy: "fixed"
display: 0
max_iter: 10
snapshot: 0
snapshot_after_train: false
snapshot_prefix: "{prefix}"
random_seed: 11
"""


def test_lmdb_training_follows_the_host_path(tmp_path, monkeypatch):
    """`-train` from an LMDB of raw Datums, with and without
    -transform_on_device, same seed: identical loss trajectories."""
    from caffeonspark_amd.api import CaffeOnSpark
    from caffeonspark_amd.core.solver import Solver
    from caffeonspark_amd.data.lmdb_io import LmdbWriter
    from caffeonspark_amd.data.processor import CaffeProcessor
    from caffeonspark_amd.tools.seq_value import datum_from_array

    rng = np.random.RandomState(1)
    items = []
    for i in range(400):
        label = rng.randint(0, 10)
        img = rng.randint(80, 150, size=(1, 28, 28)).astype(np.uint8)
        img[0, :, label * 2] = 250
        items.append((f"{i:08d}".encode(),
                      datum_from_array(img, label).SerializeToString()))
    LmdbWriter(str(tmp_path / "train_lmdb")).write(items)
    (tmp_path / "net.prototxt").write_text(
        _LENET_NET.format(train=str(tmp_path / "train_lmdb")))
    (tmp_path / "solver.prototxt").write_text(
        _SOLVER.format(net=str(tmp_path / "net.prototxt"),
                       prefix=str(tmp_path / "lenet")))

    losses = []
    step = Solver._step_one

    def recording_step(self):
        loss = step(self)
        losses.append(float(loss))
        return loss

    monkeypatch.setattr(Solver, "_step_one", recording_step)
    runs = []
    for flags in ([], ["-transform_on_device"]):
        CaffeProcessor.reset_instance()
        losses.clear()
        conf = Config(["-conf", str(tmp_path / "solver.prototxt"),
                       "-train"] + flags, seed=5)
        conf.device = CPU
        conf.dtype = torch.float32
        CaffeOnSpark(conf).train()
        runs.append(list(losses))
        CaffeProcessor.reset_instance()
    assert len(runs[0]) == 10
    assert runs[0] == runs[1]
