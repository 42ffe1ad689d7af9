#!/usr/bin/env python3
"""Per-shape timing of the conv weight gradient at the five layers of one
AlexNet training step (batch 256, bf16): the legacy route against the
grouped slab route (conv_dw_plan in ops/gpu.py).

  legacy  zero fill of dwp + one gemm_conv_dw per group (atomic split-K)
          + dw_unpack_acc / dw_unpack_s2d
  slab    one gemm_conv_dw_grouped + one dw_slab_finalize

Each figure is the median of 24 runs of the whole sequence, timed one by one
with device events; operands are random bf16 values, and every run uses the
next of several buffer sets (together > 0.7 GB, slabs included) so that
nothing is served from the Infinity Cache except what the sequence itself
leaves there.  The routes are timed alternately, --repeats times each (the
spread between repeats is the noise to read the difference against).  The
GEMMs alone, the finalize alone and the legacy unpack alone are timed the
same way.  FLOPs come from the shapes: 2 * Kout * Kcol * NPQ.

  python tools/conv_dw_bench.py                  # the planner's splits
  python tools/conv_dw_bench.py --splits 6,9,12  # force the slab route's
                                                 # splits per group
  python tools/conv_dw_bench.py --layers conv4,conv5
  python tools/conv_dw_bench.py --fin-blocks 0,128,256,512  # finalize grid
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


def _row(name, h, c, k, r, pad, groups, s2d=None):
    """dW of a stride-1 r x r convolution on an h x h NHWC image; s2d =
    (st, C, R) names the original strided layer of a space-to-depth row."""
    cg, kg = c // groups, k // groups
    p = h + 2 * pad - r + 1
    kcol = r * r * cg
    if s2d:
        st, c0, r0 = s2d
        arena, fin = (k, c0, r0, r0), (c0, r0, r0, st)
    else:
        arena, fin = (k, cg, r, r), (cg, r, r, 0)
    return dict(name=name, G=groups, Kg=kg, Cg=cg, NPQ=BATCH * p * p,
                Kcol=kcol, Kpad=_pad(kcol, 32), in_shape=(BATCH, h, h, c),
                Kout=k, arena=arena, fin=fin,
                geom=[h, h, c, p, p, 1, 1, pad, pad, 1, r, 0, cg, kcol])


ROWS = [
    _row("conv1", 57, 48, 96, 3, 0, 1, s2d=(4, 3, 11)),
    _row("conv2", 27, 96, 256, 5, 2, 2),
    _row("conv3", 13, 256, 384, 3, 1, 1),
    _row("conv4", 13, 384, 384, 3, 1, 2),
    _row("conv5", 13, 384, 256, 3, 1, 2),
]


def _buffers(row, dev, max_splits):
    n_in = 1
    for d in row["in_shape"]:
        n_in *= d
    slab = max_splits * row["Kout"] * row["Kpad"] * 4
    per_set = 2 * (n_in + row["NPQ"] * row["Kout"]) + slab
    nsets = max(2, min(LAUNCHES, int(ROTATE_BYTES // per_set) + 1))
    sets = []
    for _ in range(nsets):
        sets.append(dict(
            x=torch.randn(row["in_shape"], device=dev).to(torch.bfloat16),
            dy=(0.05 * torch.randn((row["NPQ"], row["Kout"]), device=dev))
            .to(torch.bfloat16),
            slabs=torch.empty((max_splits, row["Kout"], row["Kpad"]),
                              dtype=torch.float32, device=dev),
            dwp=torch.zeros((row["Kout"], row["Kpad"]), dtype=torch.float32,
                            device=dev),
            arena=torch.empty(row["arena"], dtype=torch.float32,
                              device=dev)))
    return sets


def _timed(fn, sets):
    us = []
    for i in range(WARMUP + LAUNCHES):
        b = sets[i % len(sets)]
        t0 = torch.cuda.Event(enable_timing=True)
        t1 = torch.cuda.Event(enable_timing=True)
        t0.record()
        fn(b)
        t1.record()
        t1.synchronize()
        if i >= WARMUP:
            us.append(t0.elapsed_time(t1) * 1e3)
    us.sort()
    return us[len(us) // 2]


def _steps(ext, G, row, zpage, splits, blocks=0):
    """The launches of both routes as closures over a buffer set."""
    g, kg, cg = row["G"], row["Kg"], row["Cg"]
    kpad, npq, kout = row["Kpad"], row["NPQ"], row["Kout"]
    fc, fr, fs, st = row["fin"]
    sk_old = G._splitk_dw(kg, kpad, npq, True)

    def zero(b):
        b["dwp"].zero_()

    def gemm_old(b):
        for gi in range(g):
            geom = list(row["geom"])
            geom[11] = gi * cg
            ext.gemm_conv_dw(b["dy"][:, gi * kg:], b["x"],
                             b["dwp"][gi * kg:], None, zpage, kg, kpad, npq,
                             kout, kpad, 2 if sk_old > 1 else 1, sk_old, 1.0,
                             geom)

    def unpack(b):
        if st:
            ext.dw_unpack_s2d(b["dwp"], b["arena"], kout, fc, fr, fs, st,
                              kpad, False)
        else:
            ext.dw_unpack_acc(b["dwp"], b["arena"], kout, fc, fr, fs, kpad,
                              False)

    def gemm_new(b):
        ext.gemm_conv_dw_grouped(b["dy"], b["x"], b["slabs"], zpage, kg,
                                 kpad, npq, kout, kpad, splits, 1.0,
                                 row["geom"], g)

    def finalize(b):
        ext.dw_slab_finalize(b["slabs"], splits, b["arena"], kout, fc, fr,
                             fs, st, kpad, False, blocks)

    def legacy(b):
        zero(b)
        gemm_old(b)
        unpack(b)

    def slab(b):
        gemm_new(b)
        finalize(b)

    return dict(legacy=legacy, slab=slab, gemm_old=gemm_old,
                gemm_new=gemm_new, finalize=finalize, unpack=unpack,
                zero=zero), G._split_count(npq, sk_old)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--splits", default="",
                    help="comma list: force the slab route's splits per "
                         "group (default: conv_dw_plan's)")
    ap.add_argument("--layers", default="",
                    help="comma list of layer names (default: all five)")
    ap.add_argument("--fin-blocks", default="",
                    help="comma list: also time the finalize alone at "
                         "these grid sizes (0: its own choice)")
    ap.add_argument("--repeats", type=int, default=2,
                    help="alternated timings of each route")
    ap.add_argument("--out", help="also write the rows as JSON here")
    args = ap.parse_args()

    from caffeonspark_amd import ops
    from caffeonspark_amd.ops import gpu as G
    ext = ops.native()
    dev = torch.device("cuda:0")
    zpage = G._zpage(dev)
    forced = [int(s) for s in args.splits.split(",") if s]
    layers = [s for s in args.layers.split(",") if s]

    results = []
    print("| layer | legacy splits x launches | slab splits | legacy us "
          "(repeats) | slab us (repeats) | GEMMs old | GEMM new | zero | "
          "unpack | finalize | slab TF/s | slab MB |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|")
    for row in ROWS:
        if layers and row["name"] not in layers:
            continue
        plan = G.conv_dw_plan(row["G"], row["Kg"], row["Kpad"],
                              row["NPQ"])[1]
        choices = [G._split_count(row["NPQ"], s) for s in forced] or [plan]
        sets = _buffers(row, dev, max(choices))
        for splits in choices:
            fns, old_splits = _steps(ext, G, row, zpage, splits)
            leg, new = [], []
            for _ in range(args.repeats):
                leg.append(_timed(fns["legacy"], sets))
                new.append(_timed(fns["slab"], sets))
            parts = {k: _timed(fns[k], sets) for k in
                     ("gemm_old", "gemm_new", "zero", "unpack", "finalize")}
            flops = 2.0 * row["Kout"] * row["Kcol"] * row["NPQ"]
            best = min(new)
            mb = splits * row["Kout"] * row["Kpad"] * 4 / 1e6 \
                if splits > 1 else 0.0
            r = dict(name=row["name"], legacy_splits=old_splits,
                     launches=row["G"], splits=splits, planned=plan,
                     legacy_us=leg, slab_us=new, slab_mb=mb,
                     slab_tfs=flops / best * 1e-6, **parts)
            for nb in [int(v) for v in args.fin_blocks.split(",") if v]:
                f2, _ = _steps(ext, G, row, zpage, splits, nb)
                r[f"finalize_blocks_{nb}"] = _timed(f2["finalize"], sets)
            results.append(r)
            print(f"| {row['name']} | {old_splits} x {row['G']} | {splits}"
                  f"{' (plan)' if splits == plan else ''} | "
                  f"{' '.join(f'{v:.1f}' for v in leg)} | "
                  f"{' '.join(f'{v:.1f}' for v in new)} | "
                  f"{parts['gemm_old']:.1f} | {parts['gemm_new']:.1f} | "
                  f"{parts['zero']:.1f} | {parts['unpack']:.1f} | "
                  f"{parts['finalize']:.1f} | {r['slab_tfs']:.0f} | "
                  f"{mb:.1f} |", flush=True)
            fin = {k: v for k, v in r.items()
                   if k.startswith("finalize_blocks_")}
            if fin:
                print("  finalize alone by grid: " + ", ".join(
                    f"{k[16:]} blocks {v:.1f} us" for k, v in fin.items()),
                    flush=True)
        del sets
        torch.cuda.empty_cache()
    planned = [r for r in results if r["splits"] == r["planned"]]
    if planned:
        print(f"\nper step at the planner's splits: legacy "
              f"{sum(min(r['legacy_us']) for r in planned):.0f} us, slab "
              f"{sum(min(r['slab_us']) for r in planned):.0f} us")
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
