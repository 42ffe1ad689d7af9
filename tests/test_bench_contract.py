"""bench.py driver contract: one JSON line with the required fields."""

import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_json_contract():
    out = subprocess.run(
        [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1",
         "--steps", "2", "--warmup", "1", "--batch", "8",
         "--model", "cifar10_quick"],
        capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-500:]
    line = out.stdout.strip().splitlines()[-1]
    d = json.loads(line)
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup",
                "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
                "dtype", "data", "config"):
        assert key in d, f"missing {key}"
    assert d["metric"] == "images/sec"
    assert d["n_gpus"] == 1
    assert d["data"] == "synthetic"
    assert d["scaling"] == "weak"
    assert d["higher_is_better"] is True
    assert d["value"] > 0
    assert {"model", "global_batch", "parallelism"} <= set(d["config"])


def test_bench_dump_outputs(tmp_path):
    """--dump-outputs DIR: the last timed step's loss, net outputs, weights
    and gradients land as float .npy files within the 64 MB budget, and
    --full is accepted alongside."""
    import numpy as np
    out_dir = tmp_path / "dump"
    out = subprocess.run(
        [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1",
         "--steps", "2", "--warmup", "1", "--batch", "8",
         "--model", "cifar10_quick", "--full",
         "--dump-outputs", str(out_dir)],
        capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-500:]
    d = json.loads(out.stdout.strip().splitlines()[-1])
    assert d["steps"] == 2 and d["ms_per_step"] > 0
    arrays = {p.stem: np.load(p) for p in out_dir.glob("*.npy")}
    assert {"loss", "out_loss", "weights", "grads"} <= set(arrays)
    for name, a in arrays.items():
        assert a.dtype in (np.float32, np.float64), name
        assert np.isfinite(a).all(), name
    assert sum(a.nbytes for a in arrays.values()) <= 64 * 2 ** 20
    # cifar10_quick: 145578 learnable parameters, dumped whole
    assert arrays["weights"].shape == arrays["grads"].shape == (145578,)
    assert np.abs(arrays["grads"]).max() > 0
    # the loss top and the returned weighted loss are the same number
    assert arrays["loss"].shape == (1,)
    assert float(arrays["loss"][0]) == float(arrays["out_loss"])
    # 10-class softmax loss a few steps from init: near ln(10)
    assert 1.0 < float(arrays["loss"][0]) < 4.0


def test_bench_default_args_fast():
    """Driver runs bench.py with no flags: must default to N=1 and finish
    quickly. We only check arg parsing + default batch resolution here."""
    import importlib.util
    spec = importlib.util.spec_from_file_location(
        "bench", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert hasattr(mod, "main")


def test_bench_two_rank_gloo_contract():
    """The driver launches bench.py under torchrun for the multi-GPU
    scaling run; lock the rendezvous + DDP + JSON contract down with a
    2-rank gloo (CPU) run of the smallest config."""
    env = dict(os.environ)
    env["MASTER_ADDR"] = "127.0.0.1"
    # gloo contract even on a GPU box (ROCm reads the HIP/ROCR variants
    # and treats an empty CUDA_VISIBLE_DEVICES as unset)
    env["CUDA_VISIBLE_DEVICES"] = ""
    env["HIP_VISIBLE_DEVICES"] = ""
    env["ROCR_VISIBLE_DEVICES"] = ""
    out = subprocess.run(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
         "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
         "--master-port", "29713", "--no-python", sys.executable,
         os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2",
         "--warmup", "1", "--batch", "8", "--model", "cifar10_quick"],
        capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    assert out.returncode == 0, out.stderr[-800:]
    line = [l for l in out.stdout.splitlines()
            if l.startswith('{"metric"')]
    assert len(line) == 1, out.stdout[-500:]  # rank 0 prints exactly one
    rec = json.loads(line[0])
    assert rec["n_gpus"] == 2
    assert rec["config"]["parallelism"] == "dp2"
