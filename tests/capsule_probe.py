"""Closed loops of one capsule per model through the controller mirrors, every tick's results written to an npz (run
as a child process of tests/test_gpu_capsule.py::test_staged_capsule_equals_copied: NMPC_AMD_CAPSULE_STAGE is read
once per process, so the staged solve -- the kernel copies its own I/O block from and to host-mapped memory -- and the
copied one need a process each). usage: capsule_probe.py out.npz

NMPCNavControlDiff at N = 80 (the shipped horizon) and NMPCNavControlTric at N = 20, 8 ticks each: reference lists
shorter than N + 1 on three ticks of four, a NaN robot pose on tick NAN_POSE_TICK (the shim rejects the stage-0 bounds
before any launch), a NaN reference pose on tick NAN_REF_TICK (the launch's solve fails); either way the iterate is
kept and the next tick recovers; a reset_mpc() before tick RESET_TICK."""
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(HERE), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

TICKS, NAN_POSE_TICK, NAN_REF_TICK, RESET_TICK = 8, 1, 3, 5
FAIL_TICKS = (NAN_POSE_TICK, NAN_REF_TICK)
CASES = (("diff", 80), ("tric", 20))
W_DIFF = [10, 10, 5, 0, 0, 0, 0, 1, 1]
FIELDS = ("status", "qp_iter", "inf_norm_res", "u0", "cmd", "xs", "us")


def path(t0, n):
    """n reference poses ahead of time t0 on a gentle arc (theta crosses +-pi: the unwrap)."""
    from nmpc_nav_control_amd.controller import Pose
    s = 0.02 * (t0 + np.arange(1, n + 1))
    th = (3.0 + 0.8 * s + np.pi) % (2 * np.pi) - np.pi
    return [Pose(0.3 * np.cos(0.8 * si), 0.3 * np.sin(0.8 * si), thi) for si, thi in zip(s, th)]


def main():
    from nmpc_nav_control_amd.controller import (CmdVelDiff, CmdVelTric, NMPCNavControlDiff, NMPCNavControlTric, Pose,
                                                 Vel)
    from oracle.oracle import Oracle
    out = {}
    for model, N in CASES:
        if model == "diff":
            ctl, Cmd = NMPCNavControlDiff(1 / 40, 0.270, 0.1, 1.0, 1.0, W_DIFF, N=N), CmdVelDiff
        else:
            d2r = np.pi / 180
            ctl = NMPCNavControlTric(1 / 40, 0.270, 0.1, 0.5, 1.0, 1.0, -45 * d2r, 45 * d2r, 15 * d2r, W_DIFF, N=N)
            Cmd = CmdVelTric
        o = Oracle(model, N, rule="acados")  # (the plant's RK4 only)
        pose, vel, steer = np.array([0.05, -0.02, 2.9]), np.array([0.1, 0.0, 0.05]), 0.0
        for tick in range(TICKS):
            if tick == RESET_TICK:
                ctl.reset_mpc()
            if model == "tric":
                ctl.setSteeringWheelAngle(steer)
            cmd = Cmd()
            p_in = np.full(3, np.nan) if tick == NAN_POSE_TICK else pose
            refs = path(tick, N - 2 + tick % 4)
            if tick == NAN_REF_TICK:
                refs[N // 2].x = float("nan")
            carried = ctl.x0[5:7].copy()
            try:
                ctl.run(Pose(*p_in), Vel(*vel), refs, cmd)
                status = ctl.status
            except RuntimeError as e:  # (the wrapper's exception carries the solve's status)
                status = int(re.search(r"status (-?\d+)", str(e)).group(1))
            xs, us = ctl.iterate()
            got = [cmd.v, cmd.w] if model == "diff" else [cmd.v, cmd.alpha]
            res = dict(status=np.int32(status), qp_iter=np.int32(ctl.qp_iter()),
                       inf_norm_res=np.float64(ctl._capsule.contents.nlp_out.contents.inf_norm_res),
                       u0=ctl._out_get(0, "u", ctl.nu), cmd=np.array(got), xs=xs, us=us)
            for k in FIELDS:
                out[f"{model}__t{tick}__{k}"] = res[k]
            if status != 0:
                continue  # (the plant stands still on a failed tick)
            wheels = ctl.directKinematrics(vel[0], vel[2]) if model == "diff" else (vel[0], steer)
            xn = o.rk4(np.concatenate([pose, wheels, carried]), us[0], 1 / 40)[0]
            pose = xn[:3]
            if model == "diff":
                vel = np.array([0.5 * (xn[3] + xn[4]), 0.0, (xn[4] - xn[3]) / 0.270])
            else:
                vel, steer = np.array([xn[3], 0.0, 0.0]), xn[4]
    np.savez(sys.argv[1], **out)


if __name__ == "__main__":
    main()
