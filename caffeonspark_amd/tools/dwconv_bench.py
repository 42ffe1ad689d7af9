"""Depthwise convolution benchmark: the direct kernels of dwconv.hip against
the per-group GEMM loop, one layer at a time.

    python -m caffeonspark_amd.tools.dwconv_bench

The shapes (N, C, H, W, k, s, p) are the 3x3 depthwise layers of MobileNet-v1
at batch 32 (stride 1: 32@112, 128@56, 256@28, 512@14; stride 2: 64@112) and
one 5x5 layer.  For each the forward op and the forward + backward pair are
timed on both routes (COS_DWC 1 and 0) in one process: after a warm-up window
per route the two alternate in timed windows bracketed by device events.
Inputs are uniform random bf16, identical for both routes.  Prints one JSON
line per shape with the median and min/max time per call of each route and,
computed from the shapes, the least bytes the layer must move (every
activation read or written once, weights and gradients once) with the rate
the direct route's median makes of them.  Needs a GPU: without one it fails.
"""

from __future__ import annotations

import argparse
import json
import os
import statistics

import torch

from .. import ops

SHAPES = [
    (32, 32, 112, 112, 3, 1, 1),
    (32, 128, 56, 56, 3, 1, 1),
    (32, 256, 28, 28, 3, 1, 1),
    (32, 512, 14, 14, 3, 1, 1),
    (32, 64, 112, 112, 3, 2, 1),
    (32, 128, 28, 28, 5, 1, 2),
]

ROUTES = {"dwc": "1", "gemm": "0"}


def shape_counts(N, C, H, W, k, s, p) -> dict:
    """Least bytes of the forward pass and of forward + backward, from the
    shapes: x and y once forward; backward reads dy for dx, dy and x for dW,
    dy for db, and writes dx; weights bf16 in, gradients fp32 out."""
    P = (H + 2 * p - k) // s + 1
    Q = (W + 2 * p - k) // s + 1
    xb, yb = N * C * H * W * 2, N * C * P * Q * 2
    wb = C * k * k * 2
    fwd = xb + yb + wb + C * 4
    bwd = (yb + wb + xb) + (yb + xb + C * k * k * 4) + (yb + C * 4)
    return {"out_hw": [P, Q], "fwd_min_bytes": fwd,
            "fwd_bwd_min_bytes": fwd + bwd,
            "fwd_flops": 2 * N * C * P * Q * k * k}


def _calls(shape, device):
    N, C, H, W, k, s, p = shape
    g = torch.Generator().manual_seed(1)
    P, Q = shape_counts(*shape)["out_hw"]
    cl = dict(memory_format=torch.channels_last)
    x = (torch.rand(N, C, H, W, generator=g) * 2 - 1).to(torch.bfloat16) \
        .to(device).contiguous(**cl)
    w = ((torch.rand(C, 1, k, k, generator=g) * 2 - 1) * 0.3).to(device)
    b = (torch.rand(C, generator=g) * 2 - 1).to(device)
    dy = (torch.rand(N, C, P, Q, generator=g) * 2 - 1).to(torch.bfloat16) \
        .to(device).contiguous(**cl)
    dw = torch.empty(C, 1, k, k, dtype=torch.float32, device=device)
    db = torch.zeros(C, dtype=torch.float32, device=device)
    args = ((s, s), (p, p), (1, 1), C)
    from ..ops import gpu as G

    def fwd():
        return ops.conv2d_forward(x, w, b, *args)

    def fwd_bwd():
        ctx = {}
        ops.conv2d_forward(x, w, b, *args, ctx=ctx)
        G.begin_backward()
        ops.conv2d_backward(x, w, dy, *args, ctx=ctx, dw_out=dw, db_out=db)

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
    for what, fn in calls.items():
        iters = {}
        for name, flag in ROUTES.items():      # warm-up + window sizing
            os.environ["COS_DWC"] = flag
            _window(fn, 3)
            per = _window(fn, 5)
            iters[name] = max(5, int(window_s * 1e3 / max(per, 1e-3)))
        ms = {name: [] for name in ROUTES}
        for _ in range(reps):                  # alternate the two routes
            for name, flag in ROUTES.items():
                os.environ["COS_DWC"] = flag
                ms[name].append(_window(fn, iters[name]))
        for name, v in ms.items():
            out[f"{what}_{name}_ms"] = round(statistics.median(v), 4)
            out[f"{what}_{name}_ms_min_max"] = [round(min(v), 4),
                                                round(max(v), 4)]
            out[f"{what}_{name}_iters"] = iters[name]
        out[f"{what}_dwc_tb_per_s"] = round(
            out[f"{what}_min_bytes"] / (out[f"{what}_dwc_ms"] * 1e-3) / 1e12,
            3)
    return out


def main(argv=None) -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--window", type=float, default=0.5,
                    help="seconds of device work per timed window")
    ap.add_argument("--reps", type=int, default=5,
                    help="timed windows per route")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("dwconv_bench needs a GPU: none is present")
    device = torch.device("cuda:0")
    prev = os.environ.get("COS_DWC")
    try:
        for shape in SHAPES:
            res = {"bench": "dwconv",
                   "device": torch.cuda.get_device_name(0), "dtype": "bf16"}
            res.update(bench_shape(shape, device, args.window, args.reps))
            print(json.dumps(res), flush=True)
    finally:
        if prev is None:
            os.environ.pop("COS_DWC", None)
        else:
            os.environ["COS_DWC"] = prev


if __name__ == "__main__":
    main()
