"""RNN recurrence benchmark: the batch-tile-resident kernel pair of
rnn_seq.hip against the per-step GEMM loop, one shape at a time.

    python -m caffeonspark_amd.tools.rnn_bench

The shapes (T, N, H) are LRCN-class decoders: 20 steps at batch 64 / hidden
1024, batch 128 / hidden 512 and batch 16 / hidden 256.  For each the forward
op and the forward + backward pair (ops.rnn_seq_forward / rnn_seq_backward
only: the input projection, output stage and weight-gradient GEMMs are the
same on both routes) are timed on both routes (COS_RNN_SEQ 1 and 0) in one
process: after a warm-up window per route the two alternate in timed windows
bracketed by device events.  Inputs are uniform random bf16, identical for
both routes; W_hh is scaled to row sums of 0.5 so the state stays away from
saturation.  Prints one JSON line per shape with the median and min/max time
per call of each route and the workgroups the resident kernel launches.
Needs a GPU: without one it fails.
"""

from __future__ import annotations

import argparse
import json
import os
import statistics

import torch

from .. import ops

SHAPES = [(20, 64, 1024), (20, 128, 512), (20, 16, 256)]

ROUTES = {"resident": "1", "loop": "0"}


def _calls(shape, device):
    T, N, H = shape
    g = torch.Generator().manual_seed(1)
    bf = torch.bfloat16

    def rnd(*s):
        return torch.rand(*s, generator=g) * 2 - 1

    xg = rnd(T, N, H).to(bf).to(device)
    w = rnd(H, H)
    w_hh = (w * (0.5 / w.abs().sum(1, keepdim=True))).to(bf).to(device)
    cont = torch.ones(T, N, device=device)
    cont[0] = 0
    dho = rnd(T, N, H).to(bf).to(device)
    routes = []

    def fwd():
        ctx = {}
        out = ops.rnn_seq_forward(xg, w_hh, cont, None, ctx)
        routes.append(ctx["route"])
        return out

    def fwd_bwd():
        _, cache = fwd()
        ctx = {}
        ops.rnn_seq_backward(dho, w_hh, cache, None, ctx)
        routes.append(ctx["route"])

    return {"fwd": fwd, "fwd_bwd": fwd_bwd}, routes


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
    T, N, H = shape
    out = {"shape": list(shape), "resident_workgroups": (N + 15) // 16}
    calls, routes = _calls(shape, device)
    for what, fn in calls.items():
        iters = {}
        for name, flag in ROUTES.items():      # warm-up + window sizing
            os.environ["COS_RNN_SEQ"] = flag
            del routes[:]
            _window(fn, 3)
            if set(routes) != {name}:
                raise RuntimeError(f"{shape}: asked for {name}, ran "
                                   f"{sorted(set(routes))}")
            per = _window(fn, 5)
            iters[name] = max(5, int(window_s * 1e3 / max(per, 1e-3)))
        ms = {name: [] for name in ROUTES}
        for _ in range(reps):                  # alternate the two routes
            for name, flag in ROUTES.items():
                os.environ["COS_RNN_SEQ"] = flag
                ms[name].append(_window(fn, iters[name]))
        for name, v in ms.items():
            out[f"{what}_{name}_ms"] = round(statistics.median(v), 4)
            out[f"{what}_{name}_ms_min_max"] = [round(min(v), 4),
                                                round(max(v), 4)]
            out[f"{what}_{name}_iters"] = iters[name]
    return out


def main(argv=None) -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--window", type=float, default=0.5,
                    help="seconds of device work per timed window")
    ap.add_argument("--reps", type=int, default=5,
                    help="timed windows per route")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("rnn_bench needs a GPU: none is present")
    device = torch.device("cuda:0")
    prev = os.environ.get("COS_RNN_SEQ")
    try:
        for shape in SHAPES:
            res = {"bench": "rnn_seq",
                   "device": torch.cuda.get_device_name(0), "dtype": "bf16"}
            res.update(bench_shape(shape, device, args.window, args.reps))
            print(json.dumps(res), flush=True)
    finally:
        if prev is None:
            os.environ.pop("COS_RNN_SEQ", None)
        else:
            os.environ["COS_RNN_SEQ"] = prev


if __name__ == "__main__":
    main()
