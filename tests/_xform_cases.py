"""Shared inputs for the device-transform tests (CPU and GPU files): seeded
images, TransformationParameters with a mean file written on the fly, the
case matrix, and in-memory ImageDataSources."""

import io
import itertools

import numpy as np

from caffeonspark_amd.data.image_source import ImageDataSource, ImageSample
from caffeonspark_amd.data.source import STOP_MARK
from caffeonspark_amd.data.transformer import DataTransformer
from caffeonspark_amd.proto import caffe_pb

H, W, CROP = 37, 41, 29
SEED = 11

MEANS = ("none", "value", "file")
SCALES = (1.0, 1.0 / 256, 0.017)
CROPS = (0, CROP)
PHASES = (caffe_pb.Phase.TRAIN, caffe_pb.Phase.TEST)
# mean x scale x crop x phase; TRAIN mirrors, TEST centre-crops
MATRIX = list(itertools.product(MEANS, SCALES, CROPS, PHASES))


def images(c, sizes, seed=0):
    """HWC uint8 images, one per (h, w) in sizes."""
    rng = np.random.RandomState(seed)
    return [rng.randint(0, 256, (h, w, c)).astype(np.uint8)
            for (h, w) in sizes]


def planar_of(img_hwc):
    return np.ascontiguousarray(img_hwc.transpose(2, 0, 1))


def write_mean_file(path, c, h, w, seed=5):
    if path.exists():           # same seed, same content
        return str(path)
    rng = np.random.RandomState(seed)
    mean = (rng.rand(c, h, w) * 255).astype(np.float32)
    bp = caffe_pb.BlobProto()
    bp.shape = caffe_pb.BlobShape(dim=[1, c, h, w])
    bp.data = [float(v) for v in mean.reshape(-1)]
    with open(path, "wb") as f:
        f.write(bp.SerializeToString())
    return str(path)


def transform_param(tmp_path, c, mean, scale, crop, mirror, hw=(H, W)):
    tp = caffe_pb.TransformationParameter(scale=scale, mirror=mirror,
                                          crop_size=crop)
    if mean == "value":
        tp.mean_value = [104.5, 117.25, 123.0][:c]
    elif mean == "file":
        tp.mean_file = write_mean_file(
            tmp_path / f"mean_{c}_{hw[0]}x{hw[1]}.binaryproto", c, *hw)
    return tp


def transformer(tmp_path, c, mean, scale, crop, phase, hw=(H, W),
                seed=SEED):
    tp = transform_param(tmp_path, c, mean, scale, crop,
                         phase == caffe_pb.Phase.TRAIN, hw)
    return DataTransformer(tp, phase, seed=seed)


def png_bytes(img_hwc_bgr):
    """Encode so that decode_image gives back exactly img_hwc_bgr."""
    from PIL import Image
    if img_hwc_bgr.shape[2] == 1:
        im = Image.fromarray(img_hwc_bgr[:, :, 0], "L")
    else:
        im = Image.fromarray(
            np.ascontiguousarray(img_hwc_bgr[:, :, ::-1]), "RGB")
    buf = io.BytesIO()
    im.save(buf, format="PNG")
    return buf.getvalue()


def samples(c, n, hw=(H, W), seed=3):
    """n ImageSamples, alternately raw planar Datum bytes and PNG."""
    out = []
    for i, img in enumerate(images(c, [hw] * n, seed)):
        if i % 2 == 0:
            out.append(ImageSample(str(i), i % 10, c, hw[0], hw[1], False,
                                   planar_of(img).tobytes()))
        else:
            out.append(ImageSample(str(i), i % 10, c, hw[0], hw[1], True,
                                   png_bytes(img)))
    return out


def image_source(tp, c, batch, on_device, hw=(H, W), seed=SEED,
                 is_train=True):
    class Conf:
        pass
    conf = Conf()
    conf.seed = seed
    conf.transform_on_device = on_device
    lp = caffe_pb.LayerParameter(name="data", type="MemoryData")
    lp.memory_data_param = caffe_pb.MemoryDataParameter(
        batch_size=batch, channels=c, height=hw[0], width=hw[1])
    lp.transform_param = tp
    return ImageDataSource(conf, lp, is_train)


def feed(src, smps):
    for s in smps:
        assert src.offer(s)
    assert src.offer(STOP_MARK)
