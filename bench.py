#!/usr/bin/env python3
"""Flagship benchmark: AlexNet (bvlc_reference / CaffeNet class) training
step, synthetic 227x227 data, bs=256/GPU, bf16 compute — the headline
metric named by BASELINE.json (whole-node images/sec at 1/2/4/8 MI355X).

Single GPU:   python bench.py --gpus 1 --steps 20 --warmup 5
Multi GPU:    python -m torch.distributed.run --nnodes=1 --nproc-per-node N \
                  --master-addr 127.0.0.1 bench.py --gpus N ...

A plain run sets up, warms up, times --steps steps and prints one JSON
line.  --dump-outputs DIR additionally writes what the last timed step
computed (see dump_outputs) so two builds can be compared array by array;
that step then restarts from the initial weights, outside the clock.
--full is where secondary measurements live; there are none today, so it
runs the same single measurement.
"""

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

# arena elements written per dumped sample: 4M fp32 = 16 MB per file, so
# weights + grads + the net outputs stay far below the 64 MB dump budget
DUMP_SAMPLE = 1 << 22


def snapshot_state(solver):
    """Optimizer state a step reads and rewrites (weights, momentum)."""
    return {"iter": solver.iter, "current_step": solver.current_step,
            "w": solver.flat_w.clone(), "m": solver.flat_m.clone(),
            "m2": None if solver.flat_m2 is None else solver.flat_m2.clone()}


def restore_state(solver, snap):
    """Put the solver back to a snapshot, in place (a captured hipGraph
    keeps the arena addresses), and re-cast the bf16 weight shadow."""
    solver.iter = snap["iter"]
    solver.current_step = snap["current_step"]
    solver.flat_w.copy_(snap["w"])
    solver.flat_m.copy_(snap["m"])
    if snap["m2"] is not None:
        solver.flat_m2.copy_(snap["m2"])
    solver.resync_shadow()


def dump_outputs(solver, out_dir):
    """Write what the last step left behind as out_dir/<name>.npy (fp32).

    A training step hands its caller the loss and, through the solver, the
    updated weights and the gradients that produced them:
      out_<blob>.npy   every net output blob (the loss tops) as the last
                       forward computed it
      loss.npy         the weighted loss sum an eager step returns
      weights.npy      the fp32 master weights after the last update
      grads.npy        the gradients of the last backward
    Arenas larger than DUMP_SAMPLE elements are sampled at a fixed, seeded
    set of indices (identical for weights and grads, and from run to run).
    main() restarts the last timed step from the initial optimizer state,
    so these arrays are one step's work on seeded inputs and agree between
    runs to within the rounding of that single step.
    """
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)

    def save(name, t):
        arr = t.detach().float().cpu().numpy().astype(np.float32, copy=False)
        np.save(os.path.join(out_dir, name + ".npy"), arr)

    net = solver.net
    for name in net.output_blob_names():
        save("out_" + name.replace("/", "_"), net.blob_by_name(name).data)
    loss = torch.zeros(1, dtype=torch.float64)
    for (li, ti, w) in net._loss_tops:
        loss += w * net.layer_tops[li][ti].data.double().sum().cpu()
    np.save(os.path.join(out_dir, "loss.npy"), loss.numpy())
    total = solver.flat_w.numel()
    if total > DUMP_SAMPLE:
        g = torch.Generator().manual_seed(20240229)
        idx = torch.randint(0, total, (DUMP_SAMPLE,), generator=g)
        idx = idx.sort().values.to(solver.flat_w.device)
        save("weights", solver.flat_w.index_select(0, idx))
        save("grads", solver.flat_g.index_select(0, idx))
    else:
        save("weights", solver.flat_w)
        save("grads", solver.flat_g)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=0)
    ap.add_argument("--model", type=str, default="alexnet")
    ap.add_argument("--dtype", type=str, default="",
                    choices=["", "bf16", "fp32"],
                    help="compute dtype (default bf16 on GPU; fp32 runs the "
                         "declared rocBLAS/MIOpen fp32 path)")
    ap.add_argument("--graph", type=int, default=-1,
                    help="hipGraph-captured steps when single-process GPU "
                         "(-1 = auto: on for launch-bound sub-ms models)")
    ap.add_argument("--dump-outputs", type=str, default="", metavar="DIR",
                    help="after the timed steps, write the last step's "
                         "outputs to DIR/<name>.npy (rank 0)")
    ap.add_argument("--full", action="store_true",
                    help="also run the secondary measurements (none exist "
                         "today: the plain run is the whole benchmark)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")

    from caffeonspark_amd.core import solver_from_prototxt
    from caffeonspark_amd.parallel import DistributedSync, init_distributed

    ws = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    use_gpu = torch.cuda.is_available()
    if use_gpu:
        torch.cuda.set_device(local_rank)   # before NCCL/RCCL init
    rank = init_distributed()
    if use_gpu:
        dev = torch.device("cuda", local_rank)
        dtype = torch.float32 if args.dtype == "fp32" else torch.bfloat16
    else:
        dev = torch.device("cpu")
        dtype = torch.float32

    if args.batch == 0:
        args.batch = {"alexnet": 256, "googlenet": 128, "cifar10_quick": 100,
                      "lrcn": 64}.get(args.model, 256)
    root = os.path.dirname(os.path.abspath(__file__))
    solver = solver_from_prototxt(
        os.path.join(root, "caffeonspark_amd", "models",
                     f"{args.model}_solver.prototxt"),
        device=dev, dtype=dtype)
    solver.param.display = 0

    sync = None
    if ws > 1:
        sync = DistributedSync(solver)
        sync.broadcast_params()

    # synthetic batch of the named config's shape, resident on device
    n = args.batch
    g = torch.Generator().manual_seed(1234 + rank)
    dl = solver.net.data_layers()[0]
    from caffeonspark_amd.core.layers.data import CoSDataLayer
    if isinstance(dl, CoSDataLayer):
        # LRCN: image + time-major caption tops
        T = int(dl.tops_cfg[2].channels)
        V = 8801
        x = torch.randn(n, 3, 227, 227, generator=g).to(dev, dtype)
        label = torch.zeros(n, 1).to(dev)
        cont = torch.ones(T, n)
        cont[0] = 0
        inp = torch.randint(0, V, (T, n), generator=g).float()
        tgt = torch.randint(0, V, (T, n), generator=g).float()
        dl.batch_size = n
        dl.reset([x, label, cont.to(dev, dtype), inp.to(dev), tgt.to(dev)])
    else:
        classes = {"cifar10_quick": 10}.get(args.model, 1000)
        c, h, w = dl.channels, dl.height, dl.width
        x = torch.randn(n, c, h, w, generator=g).to(dev, dtype)
        y = torch.randint(0, classes, (n,), generator=g).float().to(dev)
        dl.batch_size = n
        dl.reset(x, y)

    def barrier_sync():
        if ws > 1:
            torch.distributed.barrier()
        if use_gpu:
            torch.cuda.synchronize()

    # measured on MI355X: whole-step hipGraph replay wins everywhere at
    # ws=1 after the round-2 kernel work shifted the steps launch-bound
    # (cifar 106k -> 142k round 1; round 2: googlenet +2.2%, alexnet
    # +1.1%, lrcn +0.4%) — auto mode turns it on for single-process runs
    # fp32 runs the rocBLAS/MIOpen reference route: graph capture forces
    # capture-safe MIOpen algorithms (measured 10.2k -> 2.9k img/s), so
    # auto mode keeps fp32 eager
    use_graph = args.graph == 1 or (args.graph == -1
                                    and dtype != torch.float32)
    step = solver.graph_step if (use_graph and ws == 1 and use_gpu) \
        else solver._step_one
    # The split-K GEMMs accumulate with fp32 atomics, so two runs differ in
    # the last bits of a step, and training amplifies that from step to
    # step until weights differ visibly.  For a dump that two runs (or two
    # builds) can be compared by, the LAST timed step starts again from
    # the initial optimizer state: it is the same timed path on the same
    # batch, and what it computes depends on no earlier step.  The clock
    # stops while the state is put back; a run without --dump-outputs
    # never takes this branch.
    snap = snapshot_state(solver) if args.dump_outputs else None
    for _ in range(args.warmup):
        step()
    barrier_sync()
    elapsed = 0.0
    t0 = time.perf_counter()
    for i in range(args.steps):
        if snap is not None and i == args.steps - 1:
            barrier_sync()
            elapsed += time.perf_counter() - t0
            restore_state(solver, snap)
            barrier_sync()
            t0 = time.perf_counter()
        step()
    barrier_sync()
    elapsed += time.perf_counter() - t0

    # max step time over ranks
    if ws > 1:
        t = torch.tensor([elapsed], device=dev if use_gpu else None)
        torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
        elapsed = float(t.item())

    ms_per_step = elapsed / args.steps * 1000.0
    value = (n * ws * args.steps) / elapsed
    if rank == 0 and args.dump_outputs:
        dump_outputs(solver, args.dump_outputs)
    if rank == 0:
        print(json.dumps({
            "metric": "images/sec",
            "value": round(value, 2),
            "unit": "images/sec",
            "n_gpus": ws,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(ms_per_step, 3),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "fp32" if dtype == torch.float32 else "bf16",
            "data": "synthetic",
            "config": {"model": {"alexnet": "alexnet(bvlc_reference/CaffeNet)"
                                 }.get(args.model, args.model),
                       "global_batch": n * ws,
                       "seq_len": 21 if args.model == "lrcn" else None,
                       "parallelism": f"dp{ws}"},
        }), flush=True)
    if ws > 1:
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
