"""Device-side DataTransformer on the GPU: the HIP kernel behind
`ops.data_transform` against the host transformer.  The kernel does the
host's arithmetic (one fp32 subtract, one fp32 multiply, one rounding to
the output type), so every comparison is `torch.equal`: a mismatch is a
bug, not rounding."""

import os

import numpy as np
import pytest
import torch

import _xform_cases as xc
from caffeonspark_amd.data.image_source import DeviceBatch, ImageDataSource
from caffeonspark_amd.data.processor import CaffeProcessor
from caffeonspark_amd.proto import caffe_pb

pytestmark = pytest.mark.gpu

N = 5
_host_cache = {}


def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def mean_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("means")


def _host(mean_dir, c, n, case):
    """Host-path result for one matrix case, computed once and shared."""
    key = (c, n) + case
    if key not in _host_cache:
        xf = xc.transformer(mean_dir, c, *case)
        _host_cache[key] = xf.transform(xc.images(c, [(xc.H, xc.W)] * n))
    return _host_cache[key]


def _empty_out(shape, dtype, channels_last):
    out = torch.full(shape, float("nan"), dtype=dtype, device=dev())
    if channels_last:
        out = out.contiguous(memory_format=torch.channels_last)
    return out


@pytest.mark.parametrize("channels_last", [True, False])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("planar", [True, False])
@pytest.mark.parametrize("c", [1, 3])
def test_matrix_equals_host(mean_dir, c, planar, dtype, channels_last):
    """mean x scale x crop x phase at N=5 (odd image start offsets: a
    37x41xC image is 1517*C bytes), plus N=1 for the cropped mean-file
    cases."""
    for n in (N, 1):
        imgs = xc.images(c, [(xc.H, xc.W)] * n)
        raw = [xc.planar_of(im) for im in imgs] if planar else imgs
        for case in xc.MATRIX:
            mean, scale, crop, phase = case
            if n == 1 and not (crop and mean == "file"):
                continue
            want = _host(mean_dir, c, n, case).to(dtype)
            xf = xc.transformer(mean_dir, c, *case)
            out = _empty_out(tuple(want.shape), dtype, channels_last)
            got = xf.transform_device(raw, dev(), dtype, planar=planar,
                                      out=out)
            assert got is out
            assert torch.equal(got.cpu(), want), (n, case)


def test_default_output_format(mean_dir):
    imgs = xc.images(3, [(xc.H, xc.W)] * 2)
    xf = xc.transformer(mean_dir, 3, "none", 1.0, 0, caffe_pb.Phase.TEST)
    a = xf.transform_device(imgs, dev(), torch.bfloat16)
    assert a.is_contiguous(memory_format=torch.channels_last)
    b = xf.transform_device(imgs, dev(), torch.float32)
    assert b.is_contiguous()
    g = xf.transform_device(xc.images(1, [(xc.H, xc.W)] * 2), dev(),
                            torch.bfloat16)
    assert g.is_contiguous()


class _ScriptedRng:
    """Stands in for the transformer's RandomState: hands out a fixed
    sequence of draws, so a test can place crops and mirrors exactly."""

    def __init__(self, values):
        self.values = list(values)

    def randint(self, *bounds):
        return self.values.pop(0)


# (h_off, w_off, mirror) per image; offsets range over [0, 8] x [0, 12]
_DRAWS = [(0, 0, 0), (8, 12, 1), (3, 0, 1), (8, 12, 0), (5, 7, 1)]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("planar", [True, False])
def test_placed_crops_and_mixed_mirror(mean_dir, planar, dtype):
    """w_off at 0 and at its maximum, mirrored and unmirrored images in
    one batch, and a mean-file crop that touches the last row and
    column."""
    imgs = xc.images(3, [(xc.H, xc.W)] * N, seed=9)
    raw = [xc.planar_of(im) for im in imgs] if planar else imgs
    script = [v for d in _DRAWS for v in d]
    host = xc.transformer(mean_dir, 3, "file", 0.017, xc.CROP,
                          caffe_pb.Phase.TRAIN)
    host.rng = _ScriptedRng(script)
    want = host.transform(imgs).to(dtype)
    xf = xc.transformer(mean_dir, 3, "file", 0.017, xc.CROP,
                        caffe_pb.Phase.TRAIN)
    xf.rng = _ScriptedRng(script)
    got = xf.transform_device(raw, dev(), dtype, planar=planar)
    assert not xf.rng.values
    assert torch.equal(got.cpu(), want)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_ragged_mixed_layout_batch(dtype):
    sizes = [(37, 41), (29, 29), (64, 30)]
    imgs = xc.images(3, sizes)
    tp = caffe_pb.TransformationParameter(
        crop_size=xc.CROP, mirror=True, mean_value=[104.5, 117.25, 123.0],
        scale=0.017)
    host = xc.DataTransformer(tp, caffe_pb.Phase.TRAIN, seed=xc.SEED)
    xf = xc.DataTransformer(tp, caffe_pb.Phase.TRAIN, seed=xc.SEED)
    want = torch.from_numpy(np.stack([host.transform_one(im)
                                      for im in imgs])).to(dtype)
    flags = [True, False, True]
    raw = [xc.planar_of(im) if p else im for im, p in zip(imgs, flags)]
    got = xf.transform_device(raw, dev(), dtype, planar=flags)
    assert torch.equal(got.cpu(), want)


@pytest.mark.parametrize("channels_last", [True, False])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("c,hw,crop", [
    (3, (70, 66), 64),      # 12288 outputs per image: two row chunks
    (3, (2, 5500), 0),      # wider than the 5456-column tile at C=3
    (1, (2, 16400), 0),     # wider than the 16384-column tile at C=1
])
def test_more_than_one_block_per_image(mean_dir, c, hw, crop, dtype,
                                       channels_last):
    """Sizes at which one image is split over several blocks, by rows and
    by columns, mirrored and not, with a mean image."""
    imgs = xc.images(c, [hw] * 3, seed=2)
    host = xc.transformer(mean_dir, c, "file", 0.017, crop,
                          caffe_pb.Phase.TRAIN, hw=hw)
    want = host.transform(imgs).to(dtype)
    for planar in (True, False):
        raw = [xc.planar_of(im) for im in imgs] if planar else imgs
        xf = xc.transformer(mean_dir, c, "file", 0.017, crop,
                            caffe_pb.Phase.TRAIN, hw=hw)
        out = _empty_out(tuple(want.shape), dtype, channels_last)
        xf.transform_device(raw, dev(), dtype, planar=planar, out=out)
        assert torch.equal(out.cpu(), want), planar


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_strided_output_slice(mean_dir, dtype):
    """Write into channels 2..4 of an 8-channel channels-last buffer: the
    slice holds the result and every other byte keeps its value."""
    case = ("value", 1.0 / 256, xc.CROP, caffe_pb.Phase.TRAIN)
    want = _host(mean_dir, 3, N, case).to(dtype)
    big = torch.full((N, 8, xc.CROP, xc.CROP), -77.0, dtype=dtype,
                     device=dev()).contiguous(
                         memory_format=torch.channels_last)
    xf = xc.transformer(mean_dir, 3, *case)
    xf.transform_device(xc.images(3, [(xc.H, xc.W)] * N), dev(), dtype,
                        out=big[:, 2:5])
    res = big.cpu()
    assert torch.equal(res[:, 2:5], want)
    assert bool((res[:, :2] == -77.0).all())
    assert bool((res[:, 5:] == -77.0).all())


def test_extension_rejects_bad_rows():
    from caffeonspark_amd import ops
    src = torch.zeros(3 * 8 * 8, dtype=torch.uint8, device=dev())
    for row in ([0, 8, 8, 1, 5, 0, 0],      # h_off + oh > H
                [0, 8, 8, 1, 0, 5, 0],      # w_off + ow > W
                [1, 8, 8, 1, 0, 0, 0]):     # bytes past the end of src
        table = torch.tensor([row])
        with pytest.raises(RuntimeError, match="data_transform"):
            ops.data_transform(src, table.to(dev()), None, 0, 1.0, 3, 4, 4,
                               torch.float32, False, table_host=table)
    # a mean image must have the image's own [C,H,W]
    table = torch.tensor([[0, 8, 8, 1, 0, 0, 0]])
    mean = torch.zeros(3, 8, 9, device=dev())
    with pytest.raises(RuntimeError, match="mean image"):
        ops.data_transform(src, table.to(dev()), mean, 2, 1.0, 3, 4, 4,
                           torch.float32, False, table_host=table)
    # N == 0 returns without a launch
    out = ops.data_transform(src, torch.zeros((0, 7), dtype=torch.int64,
                                              device=dev()), None, 0, 1.0,
                             3, 4, 4, torch.float32, False)
    assert out.shape == (0, 3, 4, 4)


def _lenet_solver():
    from caffeonspark_amd.core import solver_from_prototxt
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    s = solver_from_prototxt(
        os.path.join(root, "caffeonspark_amd", "models",
                     "lenet_memory_solver.prototxt"),
        device=dev(), dtype=torch.bfloat16)
    s.param.display = 0
    return s


def test_feed_path_ring_reuse(mean_dir):
    """12 batches through a 3-slot staging ring, each adopted by a
    MemoryData layer on the default stream through _reset_layer, equal
    the host path's batches for the same seed."""
    assert ImageDataSource.STAGING_SLOTS == 3
    tp = xc.transform_param(mean_dir, 3, "file", 1.0 / 256, xc.CROP, True)
    smps = xc.samples(3, 48)
    off = xc.image_source(tp, 3, 4, False)
    on = xc.image_source(tp, 3, 4, True)
    xc.feed(off, smps)
    xc.feed(on, smps)
    dl = _lenet_solver().net.data_layers()[0]
    for i in range(12):
        want = off.next_batch(dev(), torch.bfloat16)
        batch = on.next_batch(dev(), torch.bfloat16)
        assert isinstance(batch, DeviceBatch) and batch.ready is not None
        CaffeProcessor._reset_layer(dl, batch)
        assert dl._data is batch[0] and dl._label is batch[1]
        assert dl._data.is_contiguous(memory_format=torch.channels_last)
        torch.cuda.synchronize()
        assert torch.equal(dl._data, want[0]), i
        assert torch.equal(dl._label, want[1]), i
    assert on.next_batch(dev(), torch.bfloat16) is None


def test_lenet_step_same_loss():
    tp = caffe_pb.TransformationParameter(scale=0.00390625)
    smps = [s for s in xc.samples(1, 128, hw=(28, 28)) if not s.encoded]
    batches = []
    for flag in (False, True):
        src = xc.image_source(tp, 1, 64, flag, hw=(28, 28))
        xc.feed(src, smps)
        batches.append(src.next_batch(dev(), torch.bfloat16))
    torch.cuda.synchronize()
    assert torch.equal(batches[0][0], batches[1][0])
    a, b = _lenet_solver(), _lenet_solver()
    assert torch.equal(a.flat_w, b.flat_w)
    losses = []
    for s, batch in zip((a, b), batches):
        dl = s.net.data_layers()[0]
        CaffeProcessor._reset_layer(dl, batch)
        losses.append(float(s._step_one()))
    torch.cuda.synchronize()
    assert losses[0] == losses[1]
