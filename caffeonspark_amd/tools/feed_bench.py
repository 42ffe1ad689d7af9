"""Feed-rate benchmark: how fast `ImageDataSource.next_batch` produces
device-resident training batches, host transform vs `-transform_on_device`.

    python -m caffeonspark_amd.tools.feed_bench

In-memory raw planar 3x256x256 uint8 samples (the standard ImageNet LMDB
record), crop 227, mirror, a mean file, batch 256, bf16 output.  Both
paths run in one process, in alternating timed windows after a warm-up
window each, with 1 and with 4 transform threads; a window is timed on the
host clock around work that ends in a device synchronise.  Prints one JSON
line: images/s per path and thread count, host-to-device bytes per batch
for each path (computed from the shapes), the transform kernel's time from
device events with the bytes/s it implies, and the time of the bare pinned
uint8 host-to-device copy of the same batch.  Needs a GPU: without one it
fails.
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import tempfile
import threading
import time

import numpy as np
import torch

from ..data.image_source import ImageDataSource, ImageSample
from ..proto import caffe_pb

C, H, W, CROP = 3, 256, 256, 227


def _write_mean(path: str) -> None:
    rng = np.random.RandomState(1)
    mean = (rng.rand(C, H, W) * 255).astype(np.float32)
    bp = caffe_pb.BlobProto()
    bp.shape = caffe_pb.BlobShape(dim=[1, C, H, W])
    bp.data = mean.reshape(-1).tolist()
    with open(path, "wb") as f:
        f.write(bp.SerializeToString())


def _samples(n: int):
    rng = np.random.RandomState(0)
    return [ImageSample(str(i), i % 1000, C, H, W, False,
                        rng.randint(0, 256, C * H * W, dtype=np.uint8)
                        .tobytes()) for i in range(n)]


def _source(mean_file: str, batch: int, on_device: bool) -> ImageDataSource:
    class Conf:
        seed = 1
        transform_on_device = on_device

    lp = caffe_pb.LayerParameter(name="data", type="MemoryData")
    lp.memory_data_param = caffe_pb.MemoryDataParameter(
        batch_size=batch, channels=C, height=H, width=W)
    lp.transform_param = caffe_pb.TransformationParameter(
        crop_size=CROP, mirror=True, mean_file=mean_file)
    return ImageDataSource(Conf(), lp, True)


def _sync(device) -> None:
    if device.type == "cuda":
        torch.cuda.synchronize(device)


def run_window(src: ImageDataSource, samples, device, dtype, threads: int,
               batches: int) -> float:
    """`threads` transform threads take `batches` batches each from `src`
    while a feeder thread offers samples; returns images per second."""
    batch = src.batch_size
    total = threads * batches * batch
    src.reset_queue()

    def feeder():
        for i in range(total):
            while not src.offer(samples[i % len(samples)]):
                pass

    def worker():
        for _ in range(batches):
            # the device path runs ahead by at most its staging ring; the
            # synchronise that ends the window waits for the rest
            out = src.next_batch(device, dtype)
            assert out is not None and out[0].shape[0] == batch

    ts = [threading.Thread(target=worker) for _ in range(threads)]
    fd = threading.Thread(target=feeder)
    _sync(device)
    t0 = time.perf_counter()
    fd.start()
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    fd.join()
    _sync(device)
    return total / (time.perf_counter() - t0)


def feed_rates(mean_file: str, samples, device, dtype, batch: int,
               thread_counts, batches: dict, reps: int) -> dict:
    out = {}
    for nt in thread_counts:
        srcs = {"host": _source(mean_file, batch, False),
                "device": _source(mean_file, batch, True)}
        for src in srcs.values():           # warm-up window
            run_window(src, samples, device, dtype, nt, 2)
        rates = {"host": [], "device": []}
        for _ in range(reps):               # alternate the two paths
            for name, src in srcs.items():
                rates[name].append(
                    run_window(src, samples, device, dtype, nt,
                               batches[name]))
        out[str(nt)] = {
            f"{name}_img_s": round(statistics.median(v), 1)
            for name, v in rates.items()}
        out[str(nt)].update({
            f"{name}_img_s_min_max": [round(min(v), 1), round(max(v), 1)]
            for name, v in rates.items()})
    return out


def kernel_and_copy_time(mean_file: str, samples, device, dtype, batch: int,
                         iters: int = 20) -> dict:
    """Device-event times of the transform kernel and of the bare pinned
    uint8 copy for one batch."""
    from .. import ops
    src = _source(mean_file, batch, True)
    xf = src.transformer
    arrs, planar = src._raw_images(samples[:batch])
    table, (c, oh, ow), total = xf.plan_batch([a.shape for a in arrs],
                                              planar)
    pinned = torch.empty(total, dtype=torch.uint8, pin_memory=True)
    buf = pinned.numpy()
    for a, row in zip(arrs, table):
        o = int(row[0])
        buf[o:o + a.size] = a.reshape(-1)
    table_host = torch.from_numpy(table)
    d_src = pinned.to(device)
    d_tab = table_host.to(device)
    mean = xf.device_mean(device)

    def launch():
        return ops.data_transform(d_src, d_tab, mean, xf.mean_mode(), 1.0,
                                  c, oh, ow, dtype, True,
                                  table_host=table_host)

    def timed(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize(device)
        ms = []
        for _ in range(iters):
            e0 = torch.cuda.Event(enable_timing=True)
            e1 = torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return statistics.median(ms)

    k_ms = timed(launch)
    copy_ms = timed(lambda: d_src.copy_(pinned, non_blocking=True))
    elem = batch * c * oh * ow
    out_b = 2 if dtype == torch.bfloat16 else 4
    # bytes the transform needs: cropped source, output, one mean image
    need = elem * (1 + out_b) + mean.numel() * 4
    return {"kernel_ms": round(k_ms, 4),
            "kernel_bytes": need,
            "kernel_gb_s": round(need / (k_ms * 1e-3) / 1e9, 1),
            "uint8_h2d_copy_ms": round(copy_ms, 4),
            "uint8_h2d_copy_gb_s": round(total / (copy_ms * 1e-3) / 1e9, 1)}


def main(argv=None) -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--batches", type=int, default=6,
                    help="host path: batches per thread per timed window")
    ap.add_argument("--device-batches", type=int, default=48,
                    help="device path: batches per thread per timed window")
    ap.add_argument("--reps", type=int, default=3,
                    help="timed windows per path")
    ap.add_argument("--threads", default="1,4")
    ap.add_argument("--samples", type=int, default=512,
                    help="distinct in-memory samples cycled through")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("feed_bench needs a GPU: none is present")
    device = torch.device("cuda:0")
    dtype = torch.bfloat16
    thread_counts = [int(t) for t in args.threads.split(",")]
    samples = _samples(max(args.samples, args.batch))
    with tempfile.TemporaryDirectory() as tmp:
        mean_file = os.path.join(tmp, "mean.binaryproto")
        _write_mean(mean_file)
        rates = feed_rates(mean_file, samples, device, dtype, args.batch,
                           thread_counts,
                           {"host": args.batches,
                            "device": args.device_batches}, args.reps)
        kern = kernel_and_copy_time(mean_file, samples, device, dtype,
                                    args.batch)
    n = args.batch
    result = {
        "bench": "feed", "device": torch.cuda.get_device_name(0),
        "batch": n, "image": [C, H, W], "crop": CROP, "dtype": "bf16",
        "threads": rates,
        "h2d_bytes_per_batch_host": n * C * CROP * CROP * 4 + n * 4,
        "h2d_bytes_per_batch_device": n * C * H * W + n * 7 * 8 + n * 4,
    }
    result.update(kern)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
