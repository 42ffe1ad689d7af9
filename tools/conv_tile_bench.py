#!/usr/bin/env python3
"""Per-shape timing of gemm_conv_fwd at the launches of one AlexNet
training step (batch 256, bf16): every convolution's forward GEMM and the
implicit data gradients of the stride-1 layers.

Each figure is 24 launches timed one by one with device events; operands
are random bf16 values, and every launch uses the next of several buffer
sets (together > 0.7 GB) so that nothing is served from the Infinity
Cache.  FLOPs come from the shapes: useful = 2 M N K, padded = 2 M
ceil(N/BN) BN K with the N tile the build would pick (128 where the build
has no conv_fwd_plan).

  python tools/conv_tile_bench.py                 # one group per launch
  python tools/conv_tile_bench.py --grouped       # all groups, one launch
  python tools/conv_tile_bench.py --sweep         # every configuration id
  python tools/conv_tile_bench.py --sweep --vec 0 # ... element-wise epilogue
  COS_CONV_BN=128 python tools/conv_tile_bench.py # the fixed 128-wide tile

Without --grouped, --sweep and --vec it uses only the 13-argument binding, so it
runs unchanged on a build from before the tile selection.
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
BATCH = 256


def _pad(v, m):
    return -(-v // m) * m


def _fwd(name, h, c, k, r, pad, groups):
    """Forward GEMM of a stride-1 r x r convolution on an h x h image."""
    cg, kg = c // groups, k // groups
    p = h + 2 * pad - r + 1
    kcol = r * r * cg
    return dict(name=name, groups=groups, M=BATCH * p * p, N=kg,
                K=max(64, _pad(kcol, 32)), in_shape=(BATCH, h, h, c),
                ldc=k, gs=(cg, kg, kg),
                geom=[h, h, c, p, p, 1, 1, pad, pad, 1, r, 0, cg, kcol])


def _dx(name, h, c, k, r, pad, groups):
    """Data gradient of the same convolution: a stride-1 convolution of dy
    with the flipped weights, N = the group's input channels."""
    cg, kg = c // groups, k // groups
    p = h + 2 * pad - r + 1
    k2 = r * r * kg
    return dict(name=name, groups=groups, M=BATCH * h * h, N=cg,
                K=max(64, _pad(k2, 32)), in_shape=(BATCH, p, p, k),
                ldc=c, gs=(kg, _pad(cg, 128), cg),
                geom=[p, p, k, h, h, 1, 1, r - 1 - pad, r - 1 - pad, 1, r,
                      0, kg, k2])


# conv1 (3 channels, 11x11 stride 4) runs space-to-depth: 48 channels, 3x3
ROWS = [
    _fwd("conv1 fwd (s2d)", 57, 48, 96, 3, 0, 1),
    _fwd("conv2 fwd", 27, 96, 256, 5, 2, 2),
    _dx("conv2 dx", 27, 96, 256, 5, 2, 2),
    _fwd("conv3 fwd", 13, 256, 384, 3, 1, 1),
    _dx("conv3 dx", 13, 256, 384, 3, 1, 1),
    _fwd("conv4 fwd", 13, 384, 384, 3, 1, 2),
    _dx("conv4 dx", 13, 384, 384, 3, 1, 2),
    _fwd("conv5 fwd", 13, 384, 256, 3, 1, 2),
    _dx("conv5 dx", 13, 384, 256, 3, 1, 2),
]


def _buffers(row, dev):
    """Rotating (x, w, y) sets; w holds every group's rows at the stride
    the layer code uses, pad rows and pad columns zero."""
    g = row["groups"]
    gs_b = row["gs"][1]
    n_in = 1
    for d in row["in_shape"]:
        n_in *= d
    rows_w = (g - 1) * gs_b + _pad(row["N"], 128)
    per_set = 2 * (n_in + rows_w * row["K"] + row["M"] * row["ldc"])
    nsets = max(2, min(LAUNCHES, int(ROTATE_BYTES // per_set) + 1))
    kreal = row["geom"][13]
    sets = []
    for _ in range(nsets):
        x = torch.randn(row["in_shape"], device=dev).to(torch.bfloat16)
        w = torch.zeros((rows_w, row["K"]), dtype=torch.bfloat16, device=dev)
        for gi in range(g):
            w[gi * gs_b:gi * gs_b + row["N"], :kreal] = \
                (0.05 * torch.randn((row["N"], kreal), device=dev)) \
                .to(torch.bfloat16)
        y = torch.empty((row["M"], row["ldc"]), dtype=torch.bfloat16,
                        device=dev)
        sets.append((x, w, y))
    return sets


def _time(ext, row, sets, zpage, grouped, cfg, vec):
    gs_c, gs_b, gs_n = row["gs"]
    extra = ()
    if grouped or cfg >= 0 or vec >= 0:
        extra = (row["groups"] if grouped else 1, gs_c, gs_b, gs_n, cfg, vec)
    us = []
    for i in range(WARMUP + LAUNCHES):
        x, w, y = sets[i % len(sets)]
        t0 = torch.cuda.Event(enable_timing=True)
        t1 = torch.cuda.Event(enable_timing=True)
        t0.record()
        ext.gemm_conv_fwd(x, w, y, None, zpage, row["M"], row["N"],
                          row["K"], row["K"], row["ldc"], False, False,
                          row["geom"], *extra)
        t1.record()
        t1.synchronize()
        if i >= WARMUP:
            us.append(t0.elapsed_time(t1) * 1e3)
    us.sort()
    return us[len(us) // 2], us[0], us[-1]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--grouped", action="store_true",
                    help="one launch for all groups of a layer")
    ap.add_argument("--sweep", action="store_true",
                    help="time every configuration id, not the chosen one")
    ap.add_argument("--vec", type=int, default=-1,
                    help="epilogue: 0 element-wise, 1 16-byte stores, "
                         "-1 the build's choice")
    ap.add_argument("--out", help="also write the rows as JSON here")
    args = ap.parse_args()

    from caffeonspark_amd import ops
    from caffeonspark_amd.ops import gpu as G
    ext = ops.native()
    dev = torch.device("cuda:0")
    zpage = G._zpage(dev)
    plan = getattr(ext, "conv_fwd_plan", None)

    results = []
    print("| use | launches | M | N | K | cfg | BMxBN waves depth | us "
          "(min..max) | useful TF/s | padded TF/s |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    for row in ROWS:
        sets = _buffers(row, dev)
        table = ext.conv_fwd_cfgs() if args.sweep else None
        for cfg in (range(len(table)) if args.sweep else [-1]):
            med, lo, hi = _time(ext, row, sets, zpage, args.grouped, cfg,
                                args.vec)
            launches = 1 if args.grouped else row["groups"]
            gmul = row["groups"] if args.grouped else 1
            bn, shape = 128, "128x128"
            if cfg >= 0 or plan is not None:
                bm, bn, waves, depth = table[cfg] if cfg >= 0 else \
                    plan(row["M"], row["N"], row["K"])
                shape = f"{bm}x{bn} {waves}w d{depth}"
            useful = 2.0 * row["M"] * row["N"] * row["K"] * gmul
            padded = 2.0 * row["M"] * _pad(row["N"], bn) * row["K"] * gmul
            r = dict(name=row["name"], launches=launches, M=row["M"],
                     N=row["N"], K=row["K"], cfg=cfg, tile=shape, us=med,
                     us_min=lo, us_max=hi, useful_tfs=useful / med * 1e-6,
                     padded_tfs=padded / med * 1e-6)
            results.append(r)
            print(f"| {row['name']} | {launches} | {row['M']} | {row['N']} "
                  f"| {row['K']} | {cfg} | {shape} | {med:.1f} "
                  f"({lo:.1f}..{hi:.1f}) | {r['useful_tfs']:.0f} | "
                  f"{r['padded_tfs']:.0f} |", flush=True)
        del sets
        torch.cuda.empty_cache()
    if not args.sweep:
        per_step = sum(r["us"] * r["launches"] for r in results)
        print(f"\nper step (us x launches, summed): {per_step:.0f} us")
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
