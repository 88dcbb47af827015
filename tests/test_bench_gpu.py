"""bench.py's N > 1 plumbing, rehearsed on the one-GPU box: `python bench.py --gpus 2` must start its
two ranks itself (self_launch -> torch.distributed.run), run the data-parallel step with the reducer attached, and relay
exactly ONE JSON line from rank 0.  With MVLT_BENCH_BACKEND=gloo both ranks share cuda:0 (RCCL refuses two ranks on one
device); the driver's SCALE runs take the default backend (RCCL, one rank per GPU) through the same code."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_two_ranks_self_launch_relays_one_json_line():
    env = dict(os.environ, MVLT_BENCH_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1",
                        "--no-extra", "--no-cpu-baseline"], env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + "\n" + r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, lines
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["steps"] == 3 and out["warmup"] == 1
    assert out["config"]["global_batch"] == 64 and out["config"]["parallelism"] == "dp2"
    assert "gloo all-reduce" in out["config"]["grad_exchange"] and "GLOBAL batch" in out["config"]["grad_exchange"]
    assert out["value"] > 0 and out["ms_per_step"] > 0
    loss = out["config"]["loss"]
    assert loss == loss and 5.0 < loss < 15.0          # ~ln(30522) + ln 2 on random-init weights


def test_bench_one_rank_over_rccl_with_and_without_the_collective():
    """`other_configs.one_rank_rccl` of the default bench line: the step with the gradient reducer over RCCL
    on ONE rank (MVLT_FORCE_DDP=1), and the same without the collective itself (MVLT_DDP_NULL_COLLECTIVE=1) -- exactly one JSON
    line each (RCCL prints a banner on stdout: bench.py re-points file descriptor 1 for the run), a finite loss, and the
    hardware-queue default in place."""
    for extra in ({}, {"MVLT_DDP_NULL_COLLECTIVE": "1"}):
        env = dict(os.environ, MVLT_FORCE_DDP="1", **extra)
        for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "GPU_MAX_HW_QUEUES"):
            env.pop(k, None)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1", "--no-extra",
                            "--no-cpu-baseline"], env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert r.returncode == 0, r.stdout[-2000:] + "\n" + r.stderr[-4000:]
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{"metric"')]
        assert len(lines) == 1, r.stdout[-2000:]
        out = json.loads(lines[0])
        assert out["n_gpus"] == 1 and out["value"] > 0
        loss = out["config"]["loss"]
        assert loss == loss and 5.0 < loss < 15.0


def test_bench_plain_run_times_its_steps_and_dumps_the_same_outputs_every_run(tmp_path):
    """A plain run (no --full): exactly --steps timed steps and the headline keys, none of the figures that --full adds;
    --dump-outputs writes one step's loss and the seeded parameter / gradient samples from fixed inputs as float .npy files, and
    two runs with the same arguments write the same outputs up to rounding (the gradients' float-atomic sums)."""
    import numpy as np
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE"):
        env.pop(k, None)
    dumps = []
    for run in ("a", "b"):
        d = tmp_path / run
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                            "--dump-outputs", str(d)], env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert r.returncode == 0, r.stdout[-2000:] + "\n" + r.stderr[-4000:]
        lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
        assert len(lines) == 1, lines
        out = json.loads(lines[0])
        assert out["steps"] == 3 and out["warmup"] == 1 and out["unit"] == "pairs/s" and out["dtype"] == "bf16"
        assert out["higher_is_better"] is True and out["ms_per_step"] > 0
        assert abs(out["value"] * out["ms_per_step"] - 32e3) < 1e-3 * 32e3          # B=32 pairs per step of ms_per_step
        for k in ("roofline", "roofline_wgrad_group", "value_dense_rows", "value_packed", "other_configs", "cpu_baseline"):
            assert k not in out, k
        assert sorted(os.listdir(d)) == ["grads.npy", "loss.npy", "params.npy"]
        assert sum(os.path.getsize(d / f) for f in os.listdir(d)) <= 64 << 20
        loss, params, grads = (np.load(d / f) for f in ("loss.npy", "params.npy", "grads.npy"))
        assert loss.dtype == np.float64 and loss.shape == (1,) and 5.0 < loss[0] < 15.0   # ~ln(30522) + ln 2 at random init
        assert params.dtype == grads.dtype == np.float32 and params.shape == grads.shape and params.ndim == 1
        assert np.isfinite(params).all() and np.isfinite(grads).all() and np.count_nonzero(grads) > grads.size // 10
        dumps.append((loss, params, grads))
    (la, pa, ga), (lb, pb, gb) = dumps
    rel = lambda x, y: float(np.linalg.norm(x.astype(np.float64) - y) / np.linalg.norm(y.astype(np.float64)))
    # measured between two runs: loss 9e-8, parameters 1e-11 and gradients 2e-11 apart (relative L2)
    assert abs(la[0] - lb[0]) < 1e-5 * abs(lb[0]), (la, lb)
    assert rel(pa, pb) < 1e-8 and rel(ga, gb) < 1e-6, (rel(pa, pb), rel(ga, gb))
