"""bench.py's multi-rank launch path on the CPU (gloo): `python bench.py --gpus 2` without torchrun's environment
starts the two ranks itself (torch.distributed.run as a child process), every rank verifies the process group's
size against --gpus, and rank 0 prints exactly one JSON line with n_gpus 2. The ranks run the shipping FleetNode
loop (the mixed config: per-rank shards of all three models, per-tick command all-gather) with the fp64 oracle
behind the solver interface (tests/cpu_fleet_solver.py), as the other gloo tests do; on the GPU box the same
path runs BatchSolver over RCCL. A --gpus that disagrees with the launched world size exits non-zero."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.join(ROOT, "tests")


def _run(args, env_extra=None, timeout=300):
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "NMPC_BENCH_LAUNCHER"):
        env.pop(k, None)
    env["PYTHONPATH"] = os.pathsep.join([TESTS, ROOT, env.get("PYTHONPATH", "")])
    env["OMP_NUM_THREADS"] = "1"
    env.update(env_extra or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], cwd=ROOT, env=env,
                          capture_output=True, text=True, timeout=timeout)


CPU = ["--device", "cpu", "--test-solver", "cpu_fleet_solver:OracleFleetSolver", "--steps", "2", "--warmup", "1",
       "--closed-loop-warmup", "2", "--no-cpu-baseline"]


def test_gpus2_launches_two_ranks_and_prints_one_line():
    p = _run(["--gpus", "2", "--config", "mixed", "--batch-per-gpu", "6", *CPU])
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, p.stdout
    r = json.loads(lines[0])
    assert r["n_gpus"] == 2 and r["config"]["ranks"] == 2 and r["config"]["backend"] == "gloo"
    assert r["config"]["launcher"] == "bench.py --gpus 2"
    assert r["config"]["batch_per_gpu"] == 6 and r["config"]["global_batch"] == 12
    assert r["config"]["rccl_gather"] is True  # mixed at world > 1: the whole-fleet gather
    assert r["failed_solves"] == 0 and r["value"] > 0
    # value: robots of all ranks x steps / the max-over-ranks timed region (2 steps)
    assert abs(r["value"] - (2 * 6) * 2 / (r["ms_per_step"] * 2e-3)) / r["value"] < 1e-3


def test_world_size_mismatch_exits_nonzero():
    # a "torchrun" environment of one rank with --gpus 2: the check fails before any work
    p = _run(["--gpus", "2", "--config", "metric", "--batch-per-gpu", "2", *CPU],
             env_extra={"RANK": "0", "WORLD_SIZE": "1", "LOCAL_RANK": "0"})
    assert p.returncode == 3 and not p.stdout.strip(), (p.returncode, p.stdout, p.stderr[-2000:])
    assert "process group has 1 rank" in p.stderr


def test_plain_run_is_lean_and_full_is_an_option():
    """A plain run reports the headline fields and leaves what --full adds (roofline, CPU baseline, u0 error) null;
    --full is accepted and keeps the same headline fields."""
    for extra in ([], ["--full"]):
        p = _run(["--config", "metric", "--batch-per-gpu", "3", *CPU, *extra])
        assert p.returncode == 0, p.stderr[-3000:]
        r = json.loads(p.stdout.strip())
        for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
            assert k in r, k
        assert r["steps"] == 2 and r["ms_per_step"] > 0 and r["config"]["full"] is bool(extra)
        assert r["qp_iter"]["robot_ticks"] == 2 * 3  # --steps sets the number of timed steps
        assert r["roofline"] is None and r["cpu_baseline"] is None and r["u0_max_abs_err"] is None  # (CPU device)


def test_dump_outputs_is_reproducible(tmp_path):
    """--dump-outputs DIR writes the last timed step's outputs as float32 .npy files (robots in the last axis), the
    same from run to run with the same arguments; over the byte budget every array keeps the same seeded sample."""
    import numpy as np
    B, dirs = 5, [str(tmp_path / "a"), str(tmp_path / "b")]
    for d in dirs:
        p = _run(["--config", "mixed", "--batch-per-gpu", str(3 * B), *CPU, "--dump-outputs", d])
        assert p.returncode == 0, p.stderr[-3000:]
        assert len([ln for ln in p.stdout.splitlines() if ln.strip()]) == 1
    names = sorted(os.listdir(dirs[0]))
    assert names == sorted(os.listdir(dirs[1]))
    for j, m in enumerate(("diff", "omni4", "tric")):
        for k in ("u0", "cmd", "status", "qp_iter", "xbar", "ubar", "pose", "vel", "traj", "tlen"):
            assert f"f{j}_{m}_{k}.npy" in names
    assert "f2_tric_steer.npy" in names and "f0_diff_steer.npy" not in names
    for n in names:
        a, b = (np.load(os.path.join(d, n)) for d in dirs)
        assert a.dtype == np.float32 and a.shape[-1] == B and np.isfinite(a).all(), n
        assert np.array_equal(a, b), n
    u0 = np.load(os.path.join(dirs[0], "f1_omni4_u0.npy"))
    assert u0.shape == (4, B) and np.abs(u0).max() > 0



def test_dump_outputs_samples_whole_robots_over_the_budget(tmp_path):
    """Over the byte budget dump_outputs keeps the same seeded robots (columns) of every array, run after run."""
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    try:
        import bench
    finally:
        sys.path.remove(ROOT)

    class View:
        def to_tensor(self):
            return Fleet.u0

    class Solver:
        def state(self):
            return View(), View(), None

    class Fleet:  # the attributes step_outputs reads: 3 arrays of 2 x 1000 floats = 24000 bytes
        model, B, solver = "diff", 1000, Solver()
        u0 = torch.arange(2000.0).reshape(2, 1000)
        cmd = status = qp_iter = pose = vel = steer = traj = tlen = None

    outs = []
    for s in ("c", "d"):
        names = bench.dump_outputs(str(tmp_path / s), [Fleet], budget=6000)
        assert names == ["f0_diff_u0", "f0_diff_ubar", "f0_diff_xbar"]
        assert sum(os.path.getsize(str(tmp_path / s / f)) for f in os.listdir(str(tmp_path / s))) <= 6000
        outs.append([np.load(str(tmp_path / s / (n + ".npy"))) for n in names])
    u0, ubar, xbar = outs[0]
    assert 0 < u0.shape[1] < 1000 and np.array_equal(u0[1] - u0[0], np.full(u0.shape[1], 1000.0))
    assert np.array_equal(u0, ubar) and np.array_equal(u0, xbar)
    assert all(np.array_equal(a, b) for a, b in zip(*outs))


def test_single_rank_default():
    p = _run(["--config", "metric", "--batch-per-gpu", "3", *CPU])
    assert p.returncode == 0, p.stderr[-3000:]
    r = json.loads(p.stdout.strip())
    assert r["n_gpus"] == 1 and r["config"]["ranks"] == 1 and r["config"]["backend"] is None
