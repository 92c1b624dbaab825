"""The shared cases of the speed map tests: the two maps, and the rule in the fp64 oracle's closed loop.

Map A: a 16 x 16 grid of 0.25 m cells with its low corner at (-2, -2); the cell (cx, cy) holds, by
(cx // 2 + cy // 2) % 3, +inf (no limit), 0.4 or 0.15 m/s: half-metre zones in a diagonal pattern that the seeded fleet
``make_fleet(model, B, seed=SEED)`` drives through. Map B, for the writer tests: 13 x 7 cells (a row / column swap
shows), seeded values, one NaN cell, one +inf cell and ``outside`` = 0.3.

The closed loop is tests/stage_bound_cases.py's (``default_fleet``, ``solve_spliced``, the plant of ``cpu_closed_loop``)
with the stage-1..N speed rows of every robot's box taken from tests/speed_map_ref.py:limits on the robot's own fp64
iterate, rounded to fp32 as the device reads it. A robot counts as reset until its first successful solve.
"""
import numpy as np

from nmpc_nav_control_amd.scenario import refs_for
from tests import speed_map_ref as sr
from tests import stage_bound_cases as sc
from tests.helpers import plant_measure

SEED = sc.SEED
SLOPE, V_FLOOR = 0.8, 0.05


def map_a():
    cx, cy = np.meshgrid(np.arange(16), np.arange(16))  # [cy][cx]
    v = np.array([np.inf, 0.4, 0.15], np.float32)[(cx // 2 + cy // 2) % 3]
    return sr.Map(-2.0, -2.0, 0.25, v)


def map_b(at=(0.0, 0.0)):
    """13 x 7 cells of 0.25 m, low corner at + (-1.25, -0.75): x0, y0 and res are dyadic, so a position can be put
    exactly on a cell edge and (X - x0) / res is exact there"""
    v = np.random.default_rng(13).uniform(0.1, 0.9, (7, 13)).astype(np.float32)
    v[2, 9] = np.nan
    v[5, 3] = np.inf
    return sr.Map(at[0] - 1.25, at[1] - 0.75, 0.25, v, outside=0.3)


def map_c(at):
    """for the cycle tests: 64 x 64 cells of 0.25 m centred on `at`, seeded limits in [0.1, 0.9), 0.3 off the grid"""
    v = np.random.default_rng(17).uniform(0.1, 0.9, (64, 64)).astype(np.float32)
    return sr.Map(at[0] - 8.0, at[1] - 8.0, 0.25, v, outside=0.3)


def box_of(model, o, lim):
    """one robot's box [N+1 or N][n] (fp32 values in float64) with the speed rows of stages 1..N at -+lim [N+1]"""
    P = {k: v.astype(np.float32).astype(np.float64) for k, v in sc.uniform_box(o).items()}
    ns = sc.speed_rows(model, o.nbx)
    P["ubx"][1:, :ns] = np.asarray(lim, np.float64)[1:, None]
    P["lbx"][1:, :ns] = -np.asarray(lim, np.float64)[1:, None]
    return P


def rule_limits(model, o, m, xbar, pose, fresh, carried, variant="rule"):
    """one robot's lim [N+1] float32 from its fp64 iterate xbar [N+1][nx] (pose [3] at every stage while fresh);
    variant "abrupt": z_0, the cell of the robot's stage-0 position, at every stage"""
    pos = np.asarray(xbar, np.float32)[:, :2, None].copy()  # [N+1][2][1]
    if fresh:
        pos[:] = np.asarray(pose, np.float32)[None, :2, None]
    cap, a = np.float32(o.prm.ubx[0]), np.float32(o.prm.ubu[0])
    if variant == "abrupt":
        z0 = np.fmin(cap, np.fmax(np.float32(V_FLOOR), m.cell(pos[0, 0].astype(np.float64), pos[0, 1].astype(np.float64))))
        return np.full(pos.shape[0], z0[0], np.float32)
    car = np.asarray(carried, np.float32).reshape(-1, 1)
    return sr.limits(m, pos, cap, a, o.prm.dt, car, sc.speed_rows(model, o.nbx), slope=SLOPE, v_floor=V_FLOOR)[:, 0]


def cell_limit(o, m, pose):
    """z of the cell a robot stands in: fminf(cap, fmaxf(v_floor, m)) at its fp32 pose"""
    p = np.asarray(pose, np.float32).astype(np.float64)
    return float(np.fmin(np.float32(o.prm.ubx[0]), np.fmax(np.float32(V_FLOOR), m.cell(p[0:1], p[1:2])))[0])


def closed_loop(model, N, B, ticks, variant="rule", hook=None):
    """variant "rule", "abrupt" or "none" (no map: the default box). Per tick and robot: status, iters, lim1 (the
    stage-1 limit the solve ran with; inf for "none"), zone (the limit of the cell the robot stands in at the tick's
    pose), speed (the largest carried speed after the solve: the speed the tick commands), and g, one ramp step."""
    fl, F = sc.default_fleet(model, N, B, SEED)
    o, m = F.os[0], map_a()
    pose, vel = fl["pose"].T.astype(np.float64).copy(), fl["vel"].T.astype(np.float64).copy()
    steer, s = fl["steer"].astype(np.float64).copy(), fl["s"].astype(np.float64).copy()
    fresh = np.ones(B, bool)
    keys = ("status", "iters", "lim1", "speed", "zone")
    log = {k: np.zeros((ticks, B), np.int32 if k in ("status", "iters") else np.float64) for k in keys}
    log["g"] = float((np.float32(SLOPE) * np.float32(o.prm.ubu[0])) * np.float32(o.prm.dt))
    for t in range(ticks):
        for i in range(B):
            traj, s[i] = refs_for(fl["path"], i, pose[i], s[i], N, o.prm.dt_ctrl)
            x0, yref, We = o.prepare(pose[i], vel[i], steer[i], traj, F.carried[i])
            box, lim1 = None, np.inf
            log["zone"][t, i] = cell_limit(o, m, pose[i])
            if variant != "none":
                lim = rule_limits(model, o, m, F.xbar[i], pose[i], fresh[i], F.carried[i], variant)
                box, lim1 = box_of(model, o, lim), float(lim[1])
            if hook:
                hook(t, i, o, (F.xbar[i].copy(), F.ubar[i].copy(), x0, yref, We), box)
            st, it, xb, ub = sc.solve_spliced(o, F.xbar[i], F.ubar[i], x0, yref, We, box)
            log["status"][t, i], log["iters"][t, i], log["lim1"][t, i] = st, it, lim1
            if st == 0:
                fresh[i] = False
                F.xbar[i], F.ubar[i] = xb, ub
                _, F.carried[i] = o.post(x0, ub[0])
                xn, _, _ = o.rk4(x0, ub[0], o.prm.dt_ctrl)
                pose[i] = xn[:3]
                vel[i], steer[i] = plant_measure(model, xn, o.prm.p)
            log["speed"][t, i] = sc.speed_of(model, F.carried[i:i + 1])[0]
    return log
