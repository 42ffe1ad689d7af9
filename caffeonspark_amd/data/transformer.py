"""DataTransformer: scale / mean-file / mean-value / crop / mirror.

Equivalent of `caffe::DataTransformer<float>` as driven from the JVM in the
reference (JniFloatDataTransformer.cpp:99-104 calls
`Transform(vector<cv::Mat>&, Blob*)`): runs CPU-side in the reader threads,
producing the batch tensor that is fed zero-copy to the data layer.
Image decode uses PIL (the reference used cv::imdecode through a JNI Mat
wrapper).
"""

from __future__ import annotations

import io
from typing import Optional, Sequence

import numpy as np
import torch

from ..proto import caffe_pb


def decode_image(data: bytes, *, color: Optional[bool] = None,
                 resize_hw: Optional[tuple] = None) -> np.ndarray:
    """Decode an encoded image to HWC uint8 BGR (caffe channel order)."""
    from PIL import Image
    img = Image.open(io.BytesIO(data))
    if color is None:
        color = img.mode not in ("L", "1", "I;16")
    img = img.convert("RGB" if color else "L")
    if resize_hw is not None:
        h, w = resize_hw
        img = img.resize((w, h))
    arr = np.asarray(img)
    if arr.ndim == 2:
        arr = arr[:, :, None]
    elif arr.shape[2] == 3:
        arr = arr[:, :, ::-1]  # RGB -> BGR like cv::imdecode
    return arr


class DataTransformer:
    def __init__(self, param: caffe_pb.TransformationParameter,
                 phase: int = caffe_pb.Phase.TRAIN,
                 seed: Optional[int] = None):
        self.param = param
        self.phase = phase
        self.rng = np.random.RandomState(seed)
        self.mean: Optional[np.ndarray] = None
        if param.mean_file:
            bp = caffe_pb.BlobProto.FromString(
                open(param.mean_file, "rb").read())
            shape = [d for d in (bp.shape.dim if bp.has_field("shape") else
                                 [bp.channels, bp.height, bp.width]) if d]
            self.mean = np.asarray(bp.data, dtype=np.float32).reshape(shape)
            if self.mean.ndim == 4:
                self.mean = self.mean[0]
        elif param.mean_value:
            self.mean = np.asarray(list(param.mean_value),
                                   dtype=np.float32).reshape(-1, 1, 1)

    def output_shape(self, c: int, h: int, w: int):
        crop = int(self.param.crop_size)
        if crop:
            return c, crop, crop
        return c, h, w

    def _draw(self, h: int, w: int):
        """Crop offsets and mirror flag for one h x w image, the only random
        part of the transform.  Draw order is h_off, w_off, mirror; offsets
        are drawn only when a crop is set and the image is larger than it,
        mirror only when param.mirror is set in the TRAIN phase.  Returns
        (cropped, h_off, w_off, mirror)."""
        crop = int(self.param.crop_size)
        cropped, h_off, w_off = False, 0, 0
        if crop and (h > crop or w > crop):
            cropped = True
            if self.phase == caffe_pb.Phase.TRAIN:
                h_off = self.rng.randint(0, h - crop + 1)
                w_off = self.rng.randint(0, w - crop + 1)
            else:
                h_off = (h - crop) // 2
                w_off = (w - crop) // 2
        mirror = bool(self.param.mirror
                      and self.phase == caffe_pb.Phase.TRAIN
                      and self.rng.randint(2))
        return cropped, h_off, w_off, mirror

    def transform_one(self, img_hwc: np.ndarray) -> np.ndarray:
        """uint8/float HWC -> float32 CHW transformed."""
        arr = img_hwc.astype(np.float32).transpose(2, 0, 1)  # CHW
        crop = int(self.param.crop_size)
        c, h, w = arr.shape
        if self.mean is not None:
            if self.mean.shape[-1] == 1 or self.mean.shape == (c, 1, 1):
                arr = arr - self.mean.reshape(c, 1, 1)
            else:
                arr = arr - self.mean
        cropped, h_off, w_off, mirror = self._draw(h, w)
        if cropped:
            arr = arr[:, h_off:h_off + crop, w_off:w_off + crop]
        if mirror:
            arr = arr[:, :, ::-1]
        if self.param.scale != 1.0:
            arr = arr * self.param.scale
        return np.ascontiguousarray(arr)

    def transform(self, images: Sequence[np.ndarray],
                  out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Batch of HWC arrays -> [N,C,H,W] float32 tensor."""
        batch = np.stack([self.transform_one(im) for im in images])
        t = torch.from_numpy(batch)
        if out is not None:
            out.copy_(t)
            return out
        return t

    # ------------------------------------------------------- device path
    def mean_mode(self) -> int:
        """0: no mean, 1: per channel, 2: a full [C,H,W] mean image."""
        if self.mean is None:
            return 0
        return 1 if self.mean.shape[-1] == 1 else 2

    def device_mean(self, device) -> Optional[torch.Tensor]:
        """The mean as an fp32 tensor resident on `device` (one copy per
        transformer and device), None without a mean."""
        if self.mean is None:
            return None
        cache = self.__dict__.setdefault("_dev_mean", {})
        key = str(device)
        if key not in cache:
            m = np.array(self.mean, dtype=np.float32)   # a writable copy
            if self.mean_mode() == 1:
                m = m.reshape(-1)
            cache[key] = torch.from_numpy(m).to(device)
        return cache[key]

    def plan_batch(self, shapes: Sequence[tuple], planar):
        """Validate a batch for `ops.data_transform` and draw its random
        parameters.  `shapes` holds one (C, H, W) per image, `planar` one
        flag per image (or one for all): True for CHW bytes, False for HWC.
        Returns (table, (C, oh, ow), total_bytes): table is the int64
        [N,7] array of (byte_offset, H, W, planar, h_off, w_off, mirror)
        rows for images packed back to back in batch order."""
        n = len(shapes)
        if n == 0:
            raise ValueError("transform_device: empty batch")
        if isinstance(planar, (bool, np.bool_, int)):
            planar = [bool(planar)] * n
        crop = int(self.param.crop_size)
        c0, h0, w0 = (int(d) for d in shapes[0])
        mode = self.mean_mode()
        for (c, h, w) in shapes:
            if c != c0:
                raise ValueError(
                    f"images of one batch differ in channels: {c} vs {c0}")
            if crop and (h < crop or w < crop):
                raise ValueError(
                    f"image {h}x{w} is smaller than crop_size {crop}")
            if not crop and (h, w) != (h0, w0):
                raise ValueError(
                    "images of one batch differ in size and no crop_size "
                    f"is set: {h}x{w} vs {h0}x{w0}")
            if mode == 1 and self.mean.size != c:
                raise ValueError(
                    f"{self.mean.size} mean values for {c} channels")
            if mode == 2 and tuple(self.mean.shape) != (c, h, w):
                raise ValueError(
                    f"mean file shape {tuple(self.mean.shape)} does not "
                    f"match the image's {(c, h, w)}")
        table = np.zeros((n, 7), dtype=np.int64)
        off = 0
        for i, (c, h, w) in enumerate(shapes):
            _, h_off, w_off, mirror = self._draw(int(h), int(w))
            table[i] = (off, h, w, int(bool(planar[i])), h_off, w_off,
                        int(mirror))
            off += int(c) * int(h) * int(w)
        oh, ow = (crop, crop) if crop else (h0, w0)
        return table, (c0, oh, ow), off

    def transform_device(self, images: Sequence[np.ndarray], device, dtype,
                         *, planar=False,
                         out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Batch of uint8 arrays -> [N,C,H,W] tensor of `dtype` on `device`,
        transformed there by `ops.data_transform` (the HIP kernel on a GPU,
        the torch reference op on the CPU).  Each image is HWC, or CHW where
        `planar` (a flag, or one flag per image) says so.  Draws the same
        random numbers in the same order as `transform`, and computes the
        same values bit for bit.  The result is channels-last for bf16 with
        C > 1, contiguous otherwise, unless `out` is given."""
        from .. import ops
        device = torch.device(device)
        n = len(images)
        flags = [bool(planar)] * n if isinstance(
            planar, (bool, np.bool_, int)) else [bool(p) for p in planar]
        shapes = []
        for im, pl in zip(images, flags):
            if im.dtype != np.uint8 or im.ndim != 3:
                raise ValueError(
                    "transform_device takes 3-D uint8 images, got "
                    f"{im.dtype} with {im.ndim} dims")
            shapes.append(tuple(im.shape) if pl else
                          (im.shape[2], im.shape[0], im.shape[1]))
        table, (c, oh, ow), total = self.plan_batch(shapes, flags)
        buf = np.empty(total, dtype=np.uint8)
        for im, row in zip(images, table):
            o = int(row[0])
            np.copyto(buf[o:o + im.size].reshape(im.shape), im)
        table_host = torch.from_numpy(table)
        return ops.data_transform(
            torch.from_numpy(buf).to(device), table_host.to(device),
            self.device_mean(device), self.mean_mode(),
            float(self.param.scale), c, oh, ow, dtype,
            c > 1 and dtype == torch.bfloat16, out=out,
            table_host=table_host)
