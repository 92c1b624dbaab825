"""The shared rule of the per-robot parameter tests: robot i of the seeded fleet gets its own bounds and weights, and
the CPU side is one fp64 Oracle per robot with exactly those values.

Robot i of ``make_fleet(model, B, seed=SEED)`` gets, on the model's default parameters:
  * speed scale SPEED[i % 5] on lbx / ubx (the speed reference states; tric's steering box is not a speed),
  * input scale INPUT[i % 3] on lbu / ubu,
  * pose-weight scale POSE_W[(i // 2) % 3] on W[0:3] and W_e[0:3],
  * input-weight scale INPUT_W[(i // 3) % 3] on the R entries W[NX:],
  * tric: the steering box times 0.6 on one side (even i: the upper side, odd i: the lower side).
Each bounded state's box is then widened to hold 1.05 |carried_i| + 0.02, so that it holds the robot's starting
reference state (without it robots 0, 5 and 10 are infeasible from the first tick).
The values are rounded to fp32 once, so the device table and the oracles hold the same numbers.
"""
import numpy as np

from nmpc_nav_control_amd.scenario import make_fleet
from oracle.oracle import Oracle

SEED = 20250824
SPEED = (0.35, 0.5, 0.7, 1.0, 1.3)
INPUT = (0.5, 1.0, 2.0)
POSE_W = (0.5, 1.0, 4.0)
INPUT_W = (0.25, 1.0, 3.0)
FIELDS = ("lbx", "ubx", "lbu", "ubu", "W", "W_e")


def handle_params(model, N, B):
    """The default parameter set for every robot: dict field -> float64 [B][n] (fp32 values)."""
    o = Oracle(model, N, rule="batched")
    n = dict(lbx=o.nbx, ubx=o.nbx, lbu=o.nbu, ubu=o.nbu, W=o.ny, W_e=o.nx)
    return {k: np.tile(np.array(getattr(o.prm, k)[:n[k]], np.float64), (B, 1)).astype(np.float32).astype(np.float64)
            for k in FIELDS}


def robot_params(model, N, B, seed=SEED):
    """dict field -> float64 [B][n] by the rule above."""
    fl = make_fleet(model, B, seed=seed)
    P = handle_params(model, N, B)
    nx = P["W_e"].shape[1]
    for i in range(B):
        ns = 1 if model == "tric" else P["lbx"].shape[1]
        P["lbx"][i, :ns] *= SPEED[i % 5]
        P["ubx"][i, :ns] *= SPEED[i % 5]
        P["lbu"][i] *= INPUT[i % 3]
        P["ubu"][i] *= INPUT[i % 3]
        P["W"][i, :3] *= POSE_W[(i // 2) % 3]
        P["W_e"][i, :3] *= POSE_W[(i // 2) % 3]
        P["W"][i, nx:] *= INPUT_W[(i // 3) % 3]
        if model == "tric":
            P["ubx" if i % 2 == 0 else "lbx"][i, 1] *= 0.6
        m = 1.05 * np.abs(fl["carried"][:, i].astype(np.float64)) + 0.02
        P["ubx"][i] = np.maximum(P["ubx"][i], m)
        P["lbx"][i] = np.minimum(P["lbx"][i], -m)
    return {k: v.astype(np.float32).astype(np.float64) for k, v in P.items()}


def oracle_for(model, N, P, i, **more):
    return Oracle(model, N, rule="batched", **{k: P[k][i] for k in FIELDS}, **more)


def oracles(model, N, P, **more):
    return [oracle_for(model, N, P, i, **more) for i in range(P["W"].shape[0])]


def set_speed_limit(o, lim):
    """nmpc_model_params_set_limits' v_max alone on one oracle: its speed reference states in [-lim, lim]."""
    for j in range(1 if o.model == "tric" else o.nbx):
        o.prm.lbx[j], o.prm.ubx[j] = -lim, lim


class OracleFleet:
    """One oracle per robot over a shared fp64 state (the iterate, the carried refs), ticked like Oracle.batch_tick."""

    def __init__(self, os_, carried):
        self.os = os_
        B, o = len(os_), os_[0]
        self.xbar = np.zeros((B, o.N + 1, o.nx))
        self.ubar = np.zeros((B, o.N, o.nu))
        for i in range(B):
            self.xbar[i], self.ubar[i] = o.iterate_create()
        self.carried = np.ascontiguousarray(carried, np.float64).copy()  # [B][nbx]

    def tick(self, pose, vel, steer, traj, tlen, only=None):
        """pose / vel [B][3], steer [B] or None, traj [B][N+1][3], tlen int32 [B]; only: the robots that solve.
        Returns cmd [B][3], u0 [B][nu], status [B], qp_iter [B] (a robot that does not solve: zeros, status 0)."""
        B, o = len(self.os), self.os[0]
        cmd, u0 = np.zeros((B, 3)), np.zeros((B, o.nu))
        st, it = np.zeros(B, np.int32), np.zeros(B, np.int32)
        for i in (range(B) if only is None else only):
            sl = slice(i, i + 1)
            _, c, u, s, q = self.os[i].batch_tick(pose[sl], vel[sl], None if steer is None else steer[sl], traj[sl],
                                                  tlen[sl], None, self.carried[sl], self.xbar[sl], self.ubar[sl])
            cmd[i], u0[i], st[i], it[i] = c[0], u[0], s[0], q[0]
        return cmd, u0, st, it
