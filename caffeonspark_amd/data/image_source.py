"""Image source base for MemoryData layers.

Mirrors ImageDataSource.scala: sample tuple
(id, label, channels, height, width, encoded, bytes); next_batch decodes /
resizes / transforms into the (data, label) tensor pair that is fed
zero-copy to the MemoryData layer.

With `-transform_on_device` the transform runs on the device instead: the
raw uint8 bytes of the batch are staged (pinned, on a GPU), copied on a
feed stream of the source's own and transformed there in one
`ops.data_transform` launch; next_batch then returns a DeviceBatch.
"""

from __future__ import annotations

import threading
from typing import List, Optional

import numpy as np
import torch

from ..proto import caffe_pb
from .source import STOP_MARK, DataSource
from .transformer import DataTransformer, decode_image


class ImageSample:
    __slots__ = ("id", "label", "channels", "height", "width", "encoded",
                 "data")

    def __init__(self, id, label, channels, height, width, encoded, data):
        self.id = id
        self.label = float(label)
        self.channels = channels
        self.height = height
        self.width = width
        self.encoded = encoded
        self.data = data


class DeviceBatch(list):
    """A batch whose tensors were produced on a side stream.  `ready` is an
    event recorded after the last kernel that writes them: a consumer makes
    its stream wait on it (and calls record_stream on the tensors) before
    it touches them, as CaffeProcessor._reset_layer does."""

    ready = None


class _StagingSlot:
    """Pinned host buffers for one in-flight batch: raw image bytes, the
    transform table and the labels, plus the event that marks the end of
    their host-to-device copies."""

    def __init__(self, batch: int):
        self.src = None
        self.table = torch.empty((batch, 7), dtype=torch.int64,
                                 pin_memory=True)
        self.label = torch.empty(batch, dtype=torch.float32,
                                 pin_memory=True)
        self.copied = torch.cuda.Event()
        self.in_flight = False

    def reserve(self, nbytes: int) -> None:
        if self.src is None or self.src.numel() < nbytes:
            self.src = torch.empty(max(nbytes, 1), dtype=torch.uint8,
                                   pin_memory=True)


class ImageDataSource(DataSource):
    # pinned staging slots each transform thread cycles through on the
    # -transform_on_device path
    STAGING_SLOTS = 3

    def __init__(self, conf, layer_param, is_train):
        super().__init__(conf, layer_param, is_train)
        p = layer_param.memory_data_param
        self._batch = int(p.batch_size)
        self.channels = int(p.channels)
        self.height = int(p.height)
        self.width = int(p.width)
        self.source_path = p.source
        phase = caffe_pb.Phase.TRAIN if is_train else caffe_pb.Phase.TEST
        self.transformer = DataTransformer(
            layer_param.transform_param, phase,
            seed=getattr(conf, "seed", None))
        self._tls = threading.local()
        self._feed_lock = threading.Lock()
        self._feed_streams: dict = {}

    @property
    def batch_size(self) -> int:
        return self._batch

    def _decode(self, s: ImageSample) -> np.ndarray:
        want_resize = getattr(self.conf, "resize", False)
        if s.encoded:
            resize = None
            if self.height and self.width and (
                    want_resize or not self.transformer.param.crop_size):
                resize = (self.height, self.width)
            return decode_image(s.data, color=(self.channels == 3),
                                resize_hw=resize)
        # raw Datum bytes are CHW (caffe convention); reorder to HWC like
        # the reference does for cv::Mat (LmdbRDD.scala:270-281)
        c = s.channels or self.channels
        h = s.height or self.height
        w = s.width or self.width
        dt = np.float32 if getattr(s, "is_float", False) else np.uint8
        arr = np.frombuffer(s.data, dtype=dt)
        return arr.reshape(c, h, w).transpose(1, 2, 0)

    def next_batch(self, device, dtype) -> Optional[List[torch.Tensor]]:
        if getattr(self, "_drained", False):
            return None
        items = []
        while len(items) < self._batch:
            item = self.take()
            if item is STOP_MARK:
                if not items:
                    return None
                # partial final batch consumed the stop mark: remember so
                # the NEXT call terminates instead of blocking forever
                self._drained = True
                break
            items.append(item)
        # -transform_on_device: uint8 batches are transformed on the device.
        # A batch holding a FloatSample (float_data Datum) has no raw bytes
        # to stage and takes the host path.
        if getattr(self.conf, "transform_on_device", False) and not any(
                getattr(s, "is_float", False) for s in items):
            return self._next_batch_device(items, torch.device(device),
                                           dtype)
        images = [self._decode(item) for item in items]
        labels = [item.label for item in items]
        data = self.transformer.transform(images)
        label = torch.tensor(labels, dtype=torch.float32)
        return [data.to(device, dtype), label.to(device)]

    # ---------------------------------------------------- device transform
    def _raw_images(self, items):
        """Per-sample uint8 arrays and planar flags for the device path:
        raw Datum bytes stay CHW as they are (planar), encoded images are
        decoded to HWC on the host."""
        arrs, planar = [], []
        for s in items:
            if s.encoded:
                arrs.append(self._decode(s))
                planar.append(False)
                continue
            c = s.channels or self.channels
            h = s.height or self.height
            w = s.width or self.width
            a = np.frombuffer(s.data, dtype=np.uint8)
            if a.size != c * h * w:
                raise ValueError(
                    f"sample {s.id!r}: {a.size} bytes for a "
                    f"{c}x{h}x{w} image")
            arrs.append(a.reshape(c, h, w))
            planar.append(True)
        return arrs, planar

    def _staging_slot(self) -> _StagingSlot:
        """Next slot of this thread's ring; waits, on the host, until the
        copies of the batch it last staged have finished."""
        ring = getattr(self._tls, "ring", None)
        if ring is None:
            ring = self._tls.ring = [
                _StagingSlot(self._batch) for _ in range(self.STAGING_SLOTS)]
            self._tls.next = 0
        slot = ring[self._tls.next % len(ring)]
        self._tls.next += 1
        if slot.in_flight:
            slot.copied.synchronize()
            slot.in_flight = False
        return slot

    def _feed_stream(self, device):
        with self._feed_lock:
            st = self._feed_streams.get(device)
            if st is None:
                st = self._feed_streams[device] = torch.cuda.Stream(device)
            return st

    def _next_batch_device(self, items, device, dtype):
        from .. import ops
        xf = self.transformer
        arrs, planar = self._raw_images(items)
        shapes = [a.shape if p else (a.shape[2], a.shape[0], a.shape[1])
                  for a, p in zip(arrs, planar)]
        table, (c, oh, ow), total = xf.plan_batch(shapes, planar)
        n = len(items)
        labels = [item.label for item in items]
        channels_last = c > 1 and dtype == torch.bfloat16
        scale = float(xf.param.scale)

        def pack(buf):
            for a, row in zip(arrs, table):
                o = int(row[0])
                np.copyto(buf[o:o + a.size].reshape(a.shape), a)

        if device.type != "cuda":
            buf = np.empty(total, dtype=np.uint8)
            pack(buf)
            table_host = torch.from_numpy(table)
            data = ops.data_transform(
                torch.from_numpy(buf).to(device), table_host.to(device),
                xf.device_mean(device), xf.mean_mode(), scale, c, oh, ow,
                dtype, channels_last, table_host=table_host)
            label = torch.tensor(labels, dtype=torch.float32)
            return [data, label.to(device)]

        slot = self._staging_slot()
        slot.reserve(total)
        pack(slot.src.numpy())
        slot.table[:n] = torch.from_numpy(table)
        slot.label[:n] = torch.tensor(labels, dtype=torch.float32)
        stream = self._feed_stream(device)
        with torch.cuda.stream(stream):
            mean = xf.device_mean(device)
            src = slot.src[:total].to(device, non_blocking=True)
            tab = slot.table[:n].to(device, non_blocking=True)
            label = slot.label[:n].to(device, non_blocking=True)
            slot.copied.record(stream)
            slot.in_flight = True
            data = ops.data_transform(
                src, tab, mean, xf.mean_mode(), scale, c, oh, ow, dtype,
                channels_last, table_host=slot.table[:n])
            ready = torch.cuda.Event()
            ready.record(stream)
        batch = DeviceBatch([data, label])
        batch.ready = ready
        return batch
