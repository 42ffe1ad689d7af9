"""Deconvolution benchmark: the depth-to-space route against the
dcol GEMM + col2im fallback, one layer at a time.

    python -m caffeonspark_amd.tools.deconv_bench

For each shape (N, Ci, Co, H, W, k, s, p) the forward op and the forward +
backward pair are timed on both routes (COS_DECONV_D2S 1 and 0) in one
process: after a warm-up window per route the two alternate in timed
windows, each bracketed by device events and sized to run well over a
fraction of a second.  Inputs are uniform random bf16, identical for both
routes.  Prints one JSON line per shape with the median and min/max time
per call of each route, and next to them what the shapes imply: the GEMM
FLOPs of each route's forward pass, the bytes of the intermediate it writes
and reads back (Z for depth-to-space, the dcol matrix for the fallback) and
the bytes of y.  Needs a GPU: without one it fails.
"""

from __future__ import annotations

import argparse
import json
import os
import statistics

import torch

from .. import ops

# shapes a user would run: an FCN/autoencoder 2x upsampler, an FCN-8s-style
# 8x upsampling head
SHAPES = [
    (32, 64, 64, 56, 56, 4, 2, 1),
    (8, 32, 32, 16, 16, 16, 8, 4),
]


def shape_counts(N, Ci, Co, H, W, k, s, p) -> dict:
    """Bytes and FLOPs the two forward routes need, from the shapes."""
    Ho = s * (H - 1) + k - 2 * p
    Wo = s * (W - 1) + k - 2 * p
    kp = -(-k // s)
    Hp, Wp = H + kp - 1, W + kp - 1
    z = N * Hp * Wp * s * s * Co * 2
    dcol = N * H * W * k * k * Co * 2
    return {
        "y_bytes": N * Co * Ho * Wo * 2,
        "z_bytes": z,
        "dcol_bytes": dcol,
        # 2*M*N*K of each route's forward GEMM
        "d2s_gemm_flops": 2 * (N * Hp * Wp) * (s * s * Co) * (kp * kp * Ci),
        "col2im_gemm_flops": 2 * (N * H * W) * (k * k * Co) * Ci,
        "out_hw": [Ho, Wo],
    }


def _make(shape, device):
    N, Ci, Co, H, W, k, s, p = shape
    g = torch.Generator().manual_seed(1)
    c = shape_counts(*shape)
    Ho, Wo = c["out_hw"]
    x = (torch.rand(N, Ci, H, W, generator=g) * 2 - 1).to(torch.bfloat16) \
        .to(device).contiguous(memory_format=torch.channels_last)
    w = ((torch.rand(Ci, Co, k, k, generator=g) * 2 - 1) * 0.1).to(device)
    b = (torch.rand(Co, generator=g) * 2 - 1).to(device)
    dy = (torch.rand(N, Co, Ho, Wo, generator=g) * 2 - 1) \
        .to(torch.bfloat16).to(device) \
        .contiguous(memory_format=torch.channels_last)
    return x, w, b, dy


def _calls(shape, device):
    N, Ci, Co, H, W, k, s, p = shape
    x, w, b, dy = _make(shape, device)
    args = ((s, s), (p, p), (1, 1), 1)
    from ..ops import gpu as G

    def fwd():
        return ops.deconv2d_forward(x, w, b, *args)

    def fwd_bwd():
        ctx = {}
        ops.deconv2d_forward(x, w, b, *args, ctx=ctx)
        G.begin_backward()
        ops.deconv2d_backward(x, w, dy, *args, ctx=ctx)

    return {"fwd": fwd, "fwd_bwd": fwd_bwd}


def _window(fn, iters: int) -> float:
    """Milliseconds per call over `iters` calls, by device events."""
    e0 = torch.cuda.Event(enable_timing=True)
    e1 = torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def bench_shape(shape, device, window_s: float, reps: int) -> dict:
    out = {"shape": list(shape)}
    out.update(shape_counts(*shape))
    calls = _calls(shape, device)
    routes = {"d2s": "1", "col2im": "0"}
    for what, fn in calls.items():
        iters = {}
        for name, flag in routes.items():      # warm-up + window sizing
            os.environ["COS_DECONV_D2S"] = flag
            _window(fn, 5)
            per = _window(fn, 20)
            iters[name] = max(20, int(window_s * 1e3 / max(per, 1e-3)))
        ms = {name: [] for name in routes}
        for _ in range(reps):                  # alternate the two routes
            for name, flag in routes.items():
                os.environ["COS_DECONV_D2S"] = flag
                ms[name].append(_window(fn, iters[name]))
        for name, v in ms.items():
            out[f"{what}_{name}_ms"] = round(statistics.median(v), 4)
            out[f"{what}_{name}_ms_min_max"] = [round(min(v), 4),
                                                round(max(v), 4)]
            out[f"{what}_{name}_iters"] = iters[name]
    return out


def main(argv=None) -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--window", type=float, default=1.5,
                    help="seconds of device work per timed window")
    ap.add_argument("--reps", type=int, default=5,
                    help="timed windows per route")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("deconv_bench needs a GPU: none is present")
    device = torch.device("cuda:0")
    prev = os.environ.get("COS_DECONV_D2S")
    try:
        for shape in SHAPES:
            res = {"bench": "deconv",
                   "device": torch.cuda.get_device_name(0), "dtype": "bf16"}
            res.update(bench_shape(shape, device, args.window, args.reps))
            print(json.dumps(res), flush=True)
    finally:
        if prev is None:
            os.environ.pop("COS_DECONV_D2S", None)
        else:
            os.environ["COS_DECONV_D2S"] = prev


if __name__ == "__main__":
    main()
