"""Closed-loop ticks of the team kernel (plain launch) with the model table holding the shared rule
(tests/robot_model_cases.py), written to an npz. Run as a child process of
tests/test_gpu_robot_model.py::test_product_matches_the_row_form_checker, so that each library -- the product's or the
checker build named by NMPC_AMD_LIB -- is the only libnmpc_amd.so in its process.
usage: robot_model_probe.py model N B ticks out"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

from nmpc_nav_control_amd._lib import default_params  # noqa: E402
from nmpc_nav_control_amd.batch import BatchSolver  # noqa: E402
from nmpc_nav_control_amd.scenario import make_fleet  # noqa: E402
from tests import robot_model_cases as mc  # noqa: E402


def main():
    model, N, B, ticks, out = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]), sys.argv[5]
    dev = torch.device("cuda:0")
    t = lambda a, dt=torch.float32: torch.from_numpy(np.ascontiguousarray(a)).to(device=dev, dtype=dt)  # noqa: E731
    os.environ["NMPC_AMD_ROWPAR_MAX"] = "0"  # the team kernel, unsplit, at this batch size
    os.environ["NMPC_AMD_SPLIT_MAX"] = "0"
    s = BatchSolver(model, N, B, params=default_params(model, N), device=dev)
    assert s.plan_ex(B, "run")["kernel"] == "team"
    s.set_robot_model(t(mc.robot_model(model, N, B).T))
    fl = make_fleet(model, B, seed=mc.SEED)
    s.state()[2].copy_from(t(fl["carried"]))
    pose, vel, steer = t(fl["pose"]), t(fl["vel"]), t(fl["steer"])
    path, prog = t(fl["path"]), t(fl["s"])
    steer_arg = steer if model == "tric" else None
    traj = torch.zeros(N + 1, 3, B, device=dev)
    tlen = torch.zeros(B, dtype=torch.int32, device=dev)
    u0 = torch.zeros(s.nu, B, device=dev)
    status = torch.full((B,), -7, dtype=torch.int32, device=dev)
    qp_iter = torch.zeros(B, dtype=torch.int32, device=dev)
    s.fleet_sim_step(path, prog, pose, vel, steer_arg, None, None, traj, tlen, advance=False)
    log = dict(u0=[], status=[], qp_iter=[])
    for _ in range(ticks):
        s.run(pose, vel, traj, steer=steer_arg, traj_len=tlen, u0=u0, status=status, qp_iter=qp_iter)
        torch.cuda.synchronize()
        log["u0"].append(u0.cpu().numpy().copy())
        log["status"].append(status.cpu().numpy().copy())
        log["qp_iter"].append(qp_iter.cpu().numpy().copy())
        s.fleet_sim_step(path, prog, pose, vel, steer_arg, u0, status, traj, tlen, advance=True)
    np.savez(out, lib=os.environ.get("NMPC_AMD_LIB", ""), **{k: np.stack(v) for k, v in log.items()})


if __name__ == "__main__":
    main()
