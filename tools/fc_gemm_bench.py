#!/usr/bin/env python3
"""Per-call timing of the InnerProduct GEMMs of one AlexNet training step
(batch 256, bf16): forward, data gradient and weight gradient of fc6, fc7
and fc8, with the helper kernels each route needs.

Each figure is the median of 24 launches timed one by one with device
events; every launch uses the next of several buffer sets (together
> 0.7 GB, beyond the 256 MB Infinity Cache).  A "call" is everything
between the two events, so a route's helpers (zero fill, bias_act_cast or
the slab finalize, the transpose, fc8's padded copy) are inside its figure;
the helper rows time them alone.  W bytes/s = bf16 weight bytes / time, out
bytes/s = output bytes / time (fp32 for dW).

  python tools/fc_gemm_bench.py                  # both routes, the plan
  python tools/fc_gemm_bench.py --route legacy   # runs on older builds too
  python tools/fc_gemm_bench.py --sk 1,2,4,7     # legacy atomics, forced sk
  python tools/fc_gemm_bench.py --stream-sk 2,4,8,16
"""

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

LAUNCHES = 24
WARMUP = 3
ROTATE_BYTES = 0.75e9
M = 256
LAYERS = [("fc6", 4096, 9216), ("fc7", 4096, 4096), ("fc8", 1000, 4096)]
BF = torch.bfloat16


def _pad128(n):
    return (n + 127) // 128 * 128


def _time(fn, nsets):
    us = []
    for i in range(WARMUP + LAUNCHES):
        t0 = torch.cuda.Event(enable_timing=True)
        t1 = torch.cuda.Event(enable_timing=True)
        t0.record()
        fn(i % nsets)
        t1.record()
        t1.synchronize()
        if i >= WARMUP:
            us.append(t0.elapsed_time(t1) * 1e3)
    us.sort()
    return us[len(us) // 2], us[0], us[-1]


def _nsets(per_set):
    return max(2, min(LAUNCHES, int(ROTATE_BYTES // per_set) + 1))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--route", default="both",
                    choices=("both", "legacy", "stream"))
    ap.add_argument("--sk", default="",
                    help="legacy fwd/dx: forced split-K factors, e.g. 1,2,4,7")
    ap.add_argument("--stream-sk", default="",
                    help="stream fwd/dx: forced slab counts")
    ap.add_argument("--out", help="also write the rows as JSON here")
    args = ap.parse_args()

    from caffeonspark_amd import ops
    from caffeonspark_amd.ops import gpu as G
    ext = ops.native()
    dev = torch.device("cuda:0")
    have_stream = hasattr(ext, "gemm_fc")
    routes = [r for r in ("legacy", "stream")
              if args.route in ("both", r) and (r == "legacy" or have_stream)]
    rows = []

    def emit(layer, what, route, plan, t, wbytes, obytes):
        med, lo, hi = t
        r = dict(layer=layer, what=what, route=route, plan=plan, us=med,
                 us_min=lo, us_max=hi,
                 w_tbs=wbytes / med * 1e-6 if wbytes else None,
                 out_tbs=obytes / med * 1e-6 if obytes else None)
        rows.append(r)
        f = lambda v: "-" if v is None else f"{v:.2f}"  # noqa: E731
        print(f"| {layer} | {what} | {route} | {plan} | {med:.1f} "
              f"({lo:.1f}..{hi:.1f}) | {f(r['w_tbs'])} | {f(r['out_tbs'])} |",
              flush=True)

    print("| layer | call | route | plan | us (min..max) | W TB/s | "
          "out TB/s |")
    print("|---|---|---|---|---|---|---|")
    for layer, N, K in LAYERS:
        wbytes = 2 * N * K
        ns = _nsets(wbytes + 2 * M * (N + K) + 4 * M * max(N, K))
        xs = [torch.randn((M, K), device=dev).to(BF) for _ in range(ns)]
        dys = [torch.randn((M, N), device=dev).to(BF) for _ in range(ns)]
        ws = [(0.02 * torch.randn((N, K), device=dev)).to(BF)
              for _ in range(ns)]
        bias = torch.randn((N,), device=dev)
        ys = [torch.empty((M, N), dtype=BF, device=dev) for _ in range(ns)]
        dxs = [torch.empty((M, K), dtype=BF, device=dev) for _ in range(ns)]

        # ------------------------------------------------ legacy fwd / dx
        def legacy_fwd(i, sk):
            w, na = ws[i], N
            if N % 128:
                wp = torch.zeros((_pad128(N), K), dtype=BF, device=dev)
                wp[:N] = w
                w, na = wp[:N], wp.shape[0]
            if sk > 1:
                acc = torch.zeros((M, N), dtype=torch.float32, device=dev)
                ext.gemm(xs[i], w, acc, None, M, N, K, K, K, N, False, False,
                         2, sk, False, 1.0, M, na)
                ext.bias_act_cast(acc, bias, ys[i], True)
            else:
                ext.gemm(xs[i], w, ys[i], bias, M, N, K, K, K, N, False,
                         False, 0, 1, True, 1.0, M, na)

        def legacy_dx(i, sk, wT=None):
            if wT is None:
                wT = G._transpose(ws[i])
            if sk > 1:
                acc = torch.zeros((M, K), dtype=torch.float32, device=dev)
                ext.gemm(dys[i], wT, acc, None, M, K, N, N, N, K, False,
                         False, 2, sk, False, 1.0, M, _pad128(K))
                ext.bias_act_cast(acc, None, dxs[i], False)
            else:
                ext.gemm(dys[i], wT, dxs[i], None, M, K, N, N, N, K, False,
                         False, 0, 1, False, 1.0, M, _pad128(K))

        if "legacy" in routes:
            sk_f = G._splitk_for(2, (N + 127) // 128, K)
            sk_d = G._splitk_for(2, (K + 127) // 128, N)
            forced = [int(v) for v in args.sk.split(",") if v]
            for sk in forced or [sk_f]:
                emit(layer, "fwd", "legacy", f"128x128 atomics sk{sk}",
                     _time(lambda i: legacy_fwd(i, sk), ns), wbytes,
                     2 * M * N)
            for sk in forced or [sk_d]:
                emit(layer, "dx (with transpose)", "legacy",
                     f"128x128 atomics sk{sk}",
                     _time(lambda i: legacy_dx(i, sk), ns), wbytes,
                     2 * M * K)
            wTs = [G._transpose(w) for w in ws[:2]]
            emit(layer, "dx GEMM alone", "legacy",
                 f"128x128 atomics sk{sk_d}",
                 _time(lambda i: legacy_dx(i % 2, sk_d, wTs[i % 2]), ns),
                 wbytes, 2 * M * K)
            del wTs
            emit(layer, "helper: transpose W", "legacy", "-",
                 _time(lambda i: G._transpose(ws[i]), ns), wbytes, wbytes)
            acc = torch.zeros((M, N), dtype=torch.float32, device=dev)
            emit(layer, "helper: zero fill + bias_act_cast", "legacy", "-",
                 _time(lambda i: (acc.zero_(), ext.bias_act_cast(
                     acc, bias, ys[i], True)), ns), 0, 2 * M * N)

        # ------------------------------------------------ stream fwd / dx
        if "stream" in routes:
            for kind, a, outs, n, k in (("fwd", xs, ys, N, K),
                                        ("dx", dys, dxs, K, N)):
                route, bm, bn, depth, sk_p = G.fc_gemm_plan(M, n, k, kind)
                forced = [int(v) for v in args.stream_sk.split(",") if v]
                for sk in forced or [sk_p]:
                    slabs = torch.empty((max(sk, 1), M, n),
                                        dtype=torch.float32, device=dev)
                    b = bias if kind == "fwd" else None
                    emit(layer, kind, route,
                         f"{bm}x{bn} d{depth} slabs sk{sk}",
                         _time(lambda i: G._fc_stream(
                             a[i], ws[i], outs[i], b, kind, kind == "fwd",
                             sk, slabs), ns), wbytes, 2 * M * n)
                    if sk > 1:
                        emit(layer, f"helper: {kind} slab finalize", route,
                             f"sk{sk}", _time(lambda i: ext.fc_slab_finalize(
                                 slabs, sk, b, outs[i], M, n, n,
                                 kind == "fwd"), ns), 0, 2 * M * n)
                    del slabs

        # ------------------------------------------------------------ dW
        del ys, dxs
        nd = _nsets(4 * N * K)
        dws = [torch.empty((N, K), dtype=torch.float32, device=dev)
               for _ in range(nd)]
        emit(layer, "dW", "wide_tt", "128x256 plain store",
             _time(lambda i: ext.gemm(
                 dys[i % ns], xs[i % ns], dws[i], None, N, K, M, N, K, K,
                 True, True, 1, 1, False, 1.0, N, K), nd), 0, 4 * N * K)
        del dws, xs, dys, ws
        torch.cuda.empty_cache()

    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
