"""bench.py through its self-launch path: `python bench.py --gpus N` without a launcher re-executes itself under
torch.distributed.run (one process per GPU, RCCL); --spawn forces that path for N = 1 so that a 1-GPU box can test it."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


def test_bench_self_launch_path_one_gpu():
    d = _run(["--gpus", "1", "--spawn", "--steps", "2", "--warmup", "1", "--batch", "512", "--no-cpu-baseline", "--full"])
    assert d["n_gpus"] == 1 and d["config"]["rccl_world_size"] == 1           # RCCL process group of one rank was initialised
    assert d["value"] > 0 and d["steps"] == 2 and d["scaling"] == "weak"
    assert d["config"]["joint_noise"] == 0.02 and 0.3 < d["config"]["lanes_resolved_at_lcp_stage0"] < 0.7
    assert d["secondary"]["stage0_only"]["lanes_resolved_at_lcp_stage0"] == 1.0
    r = d["roofline"]
    assert set(r) >= {"bound", "achieved", "peak", "unit", "frac", "traffic", "fp64", "csrc_sha16"}
    # the fp64 fraction is the primary one only when the flop count was taken on the kernels that are built right now
    assert (r["bound"] == "fp64" and r["fp64"]["csrc_sha16"] == r["csrc_sha16"] and r["unit"] == "TFLOP/s" and "hbm" in r) or \
           (r["bound"] == "hbm" and r["fp64"] is None and r["unit"] == "GB/s")
    assert 0 < r["frac"] < 1
    assert d["reps"] >= 2 and (d["timed_seconds"] >= 0.25 or d["reps"] == 25) and len(d["reps_ms_per_step"]) == d["reps"]     # a 2-step region is repeated


def test_bench_cfg5_workload_is_selectable():
    """cfg5's per-GPU share: Atlas-33 on the ground, T = 64 trajectory (a short batch here)."""
    d = _run(["--workload", "atlas33_contact", "--rollout", "8", "--steps", "1", "--warmup", "1", "--batch", "256", "--no-cpu-baseline", "--easy-noise", "0"])
    assert d["config"]["n_dofs"] == 33 and d["config"]["rollout_T"] == 8 and d["value"] > 0
    assert "N(0,0.02^2)" in d["config"]["workload"]


def test_plain_bench_times_exactly_its_steps_and_dumps_its_outputs(tmp_path):
    """A plain run (no --full): ONE timed region of exactly --steps steps, the headline fields and nothing of what --full measures; with
    --dump-outputs the last step's next state, gradients and status of every world as float64 .npy files."""
    d = _run(["--steps", "3", "--warmup", "1", "--batch", "512", "--dump-outputs", str(tmp_path)])
    assert d["steps"] == 3 and d["reps"] == 1 and len(d["reps_ms_per_step"]) == 1 and d["ms_per_step"] > 0
    assert d["metric"] == "worlds*timesteps/sec fwd+bwd" and d["unit"] == "worlds*timesteps/s" and d["higher_is_better"] is True and d["dtype"] == "f64"
    assert abs(d["value"] - 512 / (d["ms_per_step"] * 1e-3)) <= 1e-6 * d["value"]
    assert not {"secondary", "roofline", "cpu_baseline"} & set(d)
    import numpy as np
    n2 = 2 * d["config"]["n_dofs"]
    arrays = {f.stem: np.load(f) for f in tmp_path.glob("*.npy")}
    assert set(arrays) == {"next_state", "grad_state", "grad_action", "status", "shared_action_grad"}
    assert all(a.dtype == np.float64 and np.isfinite(a).all() for a in arrays.values())
    assert arrays["next_state"].shape == arrays["grad_state"].shape == (512, n2) and arrays["status"].shape == (512,)
    assert arrays["grad_action"].shape[0] == 512 and arrays["shared_action_grad"].shape == arrays["grad_action"].shape[1:]
    assert np.allclose(arrays["shared_action_grad"], 3 * arrays["grad_action"].sum(0), rtol=1e-9, atol=1e-12)   # 3 identical cold steps


def test_scale_curve_tool_at_one_gpu():
    """tools/scale_curve.py on the box's one GPU: the plain launch and the launcher path (torch.distributed.run + RCCL, one rank) of the
    same command, the table, and its assertion that the launcher path costs at most a few percent (10 % here: two short
    runs on a shared box - the tool's own default is 3 % with the driver's 20 steps)."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "scale_curve.py"), "--gpus", "1", "2", "--steps", "20", "--warmup", "5",
                        "--tolerance", "0.10"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-2500:])
    rec = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
    assert [r["n_gpus"] for r in rec["launcher"]] in ([1], [1, 2]) and rec["launcher"][0]["rccl_world_size"] == 1
    assert rec["launcher"][0]["efficiency_vs_first"] == 1.0 and abs(rec["launcher_vs_plain_n1"]) <= 0.10
    assert rec["skipped"] in ([2], [])            # a 1-GPU box says so instead of failing
    assert "efficiency" in p.stdout and "RCCL ranks" in p.stdout
