"""The saturated QPs of the solve kernels' tests: inputs only. The reference is tests/stage_bound_cases.py's
(``solve_spliced`` / ``StageFleet``: one fp64 ``oc_qp_ipm`` per robot on the tick's QP with the per-stage box spliced
in, oracle rule "batched"). Every bound is rounded to fp32 once, so the device table and the reference hold the same
numbers.

Family A, the static-plant loop. ``make_fleet(model, B, seed=SEED)`` with the default parameters: pose, velocity,
steering angle and the reference list stay those of tick 0 for all T ticks (the plant is never advanced) while the
carried reference states run on, as ``run()`` leaves them. Before each tick, robots with i % 4 != 3 get on the speed
rows of stages k = 1..N
    lim_k = max(min(ZONE, default ubx), c - k g),  c = the largest |carried| over the robot's speed reference states
    (fp32), g = fp32(fp32(0.8) fp32(a_max)) fp32(dt)
which is ``speed_map_ref.limits`` on a map of one uniform cell; the rows hold [-lim_k, lim_k]. Tric's steering rows,
the input rows and the robots with i % 4 == 3 keep the default box. The start of the horizon lies on the limit by
construction (lim_1 = c - g and the carried speed is what stage 1 of the iterate was), and ZONE is below the fleet's
speeds, so the limit stays active on most stages tick after tick.

Family B, the iterate exactly on the bound (solve mode: one QP on packed data). From family A's state after its last
tick, the iterate, x0, yref and We rounded to fp32. For K in KS(N) = (1, N/2 - 3, N) the speed rows of stages 1..K
hold [-m_k, m_k], m_k = the iterate's own largest |speed state| at stage k, floored at FLOOR; all other rows keep the
defaults. Then ubx - xbar or lbx - xbar is exactly 0 on the row that attains m_k, in fp32 and in fp64 alike. Variant
"above" has m_k one fp32 ulp larger, "below" one ulp smaller (the iterate is just outside).

Family C, saturated inputs: family B's exact K = N/2 - 3 case on another iterate. At every stage ubar is the input
bound with the sign of family A's own input, each state stage is rolled out with the oracle's RK4 and the result is
rounded to fp32; m_k is taken from that iterate. The roll-out starts START_GAP outside x0 on every speed reference
state (stage 0 of the iterate is x0 with those states moved away from zero by START_GAP), not at x0 itself. A speed
reference state is the integral of its input, so a state rolled out from x0 under an input held on one bound is the
farthest the QP can reach: with the limit exactly there, the feasible set of that row is the single point du = 0 and
has no interior. The fp64 reference then stalls at mu = 2e-7 with step lengths falling to 1e-90 and runs into
qp_iter_max on 6 of 16 (diff, N = 20), 2 (omni4), 3 (tric) and 4 (diff, N = 40) robots, more than may be removed. With
the start moved, dx0 = -START_GAP on those rows opens the same gap below every pinned limit while ubx - xbar and
ubu - ubar (or the lower sides) stay exactly 0, and the reference solves all 16 robots of every case in at most 21
iterations.

A robot of family B or C that the reference itself does not solve (status != 0, or qp_iter_max reached) is listed in
DROPPED by index; at most MAX_DROPPED per case. No robot of family A is left out.
"""
import functools

import numpy as np

from nmpc_nav_control_amd.scenario import make_fleet, refs_for
from oracle.oracle import Oracle
from tests import stage_bound_cases as sc

F32 = np.float32
SEED = sc.SEED
B = 16
T = 40
ZONE = 0.3
SLOPE = 0.8
FLOOR = 0.05
START_GAP = 0.02
VARIANTS = ("exact", "above", "below")
MAX_DROPPED = 2
QP_ITER_MAX = 50

# (model, N, family, K, variant) -> the robots the fp64 reference does not solve, removed from the case: none
DROPPED = {}


def f32(a):
    return np.asarray(a, np.float64).astype(F32).astype(np.float64)


def ks(N):
    return (1, N // 2 - 3, N)


def gain(o):
    """g, the limit's slope per stage: fp32(fp32(SLOPE) fp32(a_max)) fp32(dt), an fp32 value"""
    return (F32(SLOPE) * F32(o.prm.ubu[0])) * F32(o.prm.dt)


def limited(i):
    return i % 4 != 3


def zone_limits(model, N, carried):
    """lim [B][N+1] fp32 of the rule, from carried [B][nbx] (rounded to fp32 here)"""
    o = Oracle(model, N, rule="batched")
    ns = sc.speed_rows(model, o.nbx)
    c = np.abs(np.asarray(carried, np.float64).astype(F32))[:, :ns].max(axis=1)
    z = np.fmin(F32(min(o.prm.ubx[j] for j in range(ns))), F32(ZONE))
    k = np.arange(N + 1, dtype=F32)
    lim = np.fmax(z, c[:, None] - k[None, :] * gain(o))
    assert lim.dtype == F32
    return lim


def zone_profile(model, N, carried, mistake=None):
    """The rule's table for one tick: dict lbx / ubx [B][N+1][nbx], lbu / ubu [B][N][nbu], fp32 values in float64.
    mistake: None, "ignore" (the default box everywhere) or "next" (stage k holds stage k + 1's limit)."""
    n = len(carried)
    P = sc.default_profile(model, N, n)
    if mistake == "ignore":
        return P
    lim = zone_limits(model, N, carried).astype(np.float64)
    if mistake == "next":
        lim = lim[:, np.minimum(np.arange(N + 1) + 1, N)]
    ns = sc.speed_rows(model, P["ubx"].shape[2])
    for i in range(n):
        if limited(i):
            P["ubx"][i, 1:, :ns] = lim[i, 1:, None]
            P["lbx"][i, 1:, :ns] = -lim[i, 1:, None]
    return P


def static_inputs(model, N, n=B):
    """tick 0's measurements and reference lists of the seeded fleet, fp32 values: (pose [n][3], vel [n][3], steer [n]
    or None, traj [n][N+1][3], tlen [n]) as StageFleet.tick takes them, and the fleet"""
    fl = make_fleet(model, n, seed=SEED)
    o = Oracle(model, N, rule="batched")
    pose, vel = fl["pose"].T.astype(np.float64), fl["vel"].T.astype(np.float64)
    traj, tlen = np.zeros((n, N + 1, 3)), np.zeros(n, np.int32)
    for i in range(n):
        tr, _ = refs_for(fl["path"], i, pose[i], fl["s"][i], N, o.prm.dt_ctrl)
        tlen[i] = len(tr)
        traj[i, :len(tr)] = f32(tr)
    steer = fl["steer"].astype(np.float64) if model == "tric" else None
    return (np.ascontiguousarray(pose), np.ascontiguousarray(vel), steer, traj, tlen), fl


@functools.lru_cache(maxsize=None)
def static_loop(model, N, ticks=T, n=B):
    """Family A on the CPU, c from the reference's own carried states. Per tick the state before it (xbar, ubar,
    carried) and its table, statuses, iteration counts and u0; the inputs; the fleet after the last tick."""
    inp, fl = static_inputs(model, N, n)
    F = sc.StageFleet([Oracle(model, N, rule="batched") for _ in range(n)], fl["carried"].T)
    log = dict(inp=inp, pre=[], P=[], status=[], iters=[], u0=[])
    for _ in range(ticks):
        P = zone_profile(model, N, F.carried)
        log["pre"].append((F.xbar.copy(), F.ubar.copy(), F.carried.copy()))
        log["P"].append(P)
        _, u0, st, it = F.tick(*inp, P=P)
        log["status"].append(st)
        log["iters"].append(it)
        log["u0"].append(u0)
    log["fleet"] = F
    return log


def on_limit(model, xbar, P, tol=1e-6):
    """[B] the number of stages 1..N at which a speed state of the iterate is within tol of its limit"""
    o = Oracle(model, xbar.shape[1] - 1, rule="batched")
    ix, _ = sc.idx(o)
    ns = sc.speed_rows(model, o.nbx)
    v = np.abs(xbar[:, 1:, ix[:ns]])
    return (np.abs(v - P["ubx"][:, 1:, :ns]) <= tol).any(axis=2).sum(axis=1)


def speed_states(o, xbar):
    """|speed states| of an iterate: xbar [..][N+1][nx] -> [..][N+1][ns]"""
    ix, _ = sc.idx(o)
    return np.abs(xbar[..., ix[:sc.speed_rows(o.model, o.nbx)]])


def ulp_step(m, variant):
    m = np.asarray(m, F32)
    if variant == "above":
        return np.nextafter(m, F32(np.inf))
    if variant == "below":
        return np.nextafter(m, F32(0))
    assert variant == "exact"
    return m


def pinned_profile(model, N, xbar, K, variant="exact", mistake=None):
    """Family B's table on the fp32 iterate xbar [n][N+1][nx]: stages 1..K of the speed rows at +-m_k.
    mistake as zone_profile's."""
    o = Oracle(model, N, rule="batched")
    P = sc.default_profile(model, N, len(xbar))
    if mistake == "ignore":
        return P
    ns = sc.speed_rows(model, o.nbx)
    v = speed_states(o, xbar).max(axis=2)
    assert np.array_equal(v, f32(v))  # (the iterate holds fp32 values, so m_k is the iterate's own number)
    m = ulp_step(np.fmax(v.astype(F32), F32(FLOOR)), variant).astype(np.float64)
    src = np.arange(N + 1) + (1 if mistake == "next" else 0)
    for k in range(1, K + 1):
        # ("next": stage k holds what the rule gives stage k + 1, which past K is the default box)
        if src[k] <= K:
            P["ubx"][:, k, :ns] = m[:, src[k], None]
            P["lbx"][:, k, :ns] = -m[:, src[k], None]
        else:
            P["ubx"][:, k, :ns] = P["ubx"][:, N, :ns]
            P["lbx"][:, k, :ns] = P["lbx"][:, N, :ns]
    return P


def saturated_iterate(o, x0, ubar, lbu, ubu):
    """Family C's iterate of one robot: ubar on the bound with its own sign at every stage, the states re-rolled from x0
    with the oracle's RK4; fp32 values"""
    _, iu = sc.idx(o)
    ub = np.array(ubar, np.float64)
    for j, col in enumerate(iu):
        ub[:, col] = np.where(ubar[:, col] < 0, lbu[:, j], ubu[:, j])
    ix, _ = sc.idx(o)
    ns = sc.speed_rows(o.model, o.nbx)
    xb = np.zeros((o.N + 1, o.nx))
    xb[0] = x0
    xb[0, ix[:ns]] += np.where(x0[ix[:ns]] < 0, -START_GAP, START_GAP)
    for k in range(o.N):
        xb[k + 1], _, _ = o.rk4(xb[k], ub[k])
    return f32(xb), f32(ub)


class SolveCase:
    """One solve-mode case: packed QP data of the kept robots (fp32 values in float64) and the table."""

    def __init__(self, model, N, family, K, variant, keep, xbar, ubar, x0, yref, We):
        self.model, self.N, self.family, self.K, self.variant = model, N, family, K, variant
        self.keep = keep
        self.xbar, self.ubar, self.x0, self.yref, self.We = xbar, ubar, x0, yref, We
        self.P = pinned_profile(model, N, xbar, K, variant)

    @property
    def name(self):
        return f"{self.family}-K{self.K}-{self.variant}"

    def profile(self, mistake=None):
        return pinned_profile(self.model, self.N, self.xbar, self.K, self.variant, mistake)

    def box(self, i, P=None):
        P = self.P if P is None else P
        return {k: P[k][i] for k in sc.FIELDS}


def _solve_data(model, N, saturate):
    """family A's state after its last tick as packed solve-mode data, every robot"""
    L = static_loop(model, N)
    F, (pose, vel, steer, traj, tlen) = L["fleet"], L["inp"]
    n = len(F.os)
    D = sc.default_profile(model, N, n)
    xs, us, x0s, ys, ws = [], [], [], [], []
    for i, o in enumerate(F.os):
        x0, yref, We = o.prepare(pose[i], vel[i], 0.0 if steer is None else steer[i], traj[i][:int(tlen[i])],
                                 F.carried[i])
        x0, yref, We = f32(x0), f32(yref), f32(We)
        xb, ub = f32(F.xbar[i]), f32(F.ubar[i])
        if saturate:
            xb, ub = saturated_iterate(o, x0, ub, D["lbu"][i], D["ubu"][i])
        for lst, a in zip((xs, us, x0s, ys, ws), (xb, ub, x0, yref, We)):
            lst.append(a)
    return tuple(np.stack(a) for a in (xs, us, x0s, ys, ws))


@functools.lru_cache(maxsize=None)
def solve_cases(model, N, with_dropped=False):
    """The family B and C cases of (model, N): B for every K of ks(N) and every variant, C once. with_dropped: every
    robot, for the CPU test that checks the DROPPED list."""
    out = []
    for family in ("B", "C"):
        data = _solve_data(model, N, family == "C")
        for K in (ks(N) if family == "B" else ks(N)[1:2]):
            for variant in (VARIANTS if family == "B" else VARIANTS[:1]):
                gone = () if with_dropped else DROPPED.get((model, N, family, K, variant), ())
                assert len(gone) <= MAX_DROPPED
                keep = np.array([i for i in range(B) if i not in gone])
                out.append(SolveCase(model, N, family, K, variant, keep, *[a[keep] for a in data]))
    return out


# ---- the recorded failure (tests/golden/make_saturated_fixture.md) ----------------------------------------------------
def recorded():
    """the stored history of the robot whose solve failed under the seeded speed map: dict of float64 / int arrays,
    per tick t = 0..tick: traj [N+1][3], vlim [N+1], carried [nbx], xbar [N+1][nx], ubar [N][nu] (before the solve),
    status, qp_iter, qp_res, u0, cmd (the device's results), reset; pose, vel per tick (constant)."""
    import os
    d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "saturated_diff_N40_r459.npz"))
    N = int(d["N"])
    o = Oracle("diff", N, rule="batched")
    out = {k: (np.asarray(d[k], np.float64) if d[k].dtype == np.float32 else np.asarray(d[k])) for k in d.files}
    T1 = len(out["status"])
    out["xbar"] = out["xbar"].reshape(T1, N + 1, o.nx)
    out["ubar"] = out["ubar"].reshape(T1, N, o.nu)
    out["N"], out["tick"], out["robot"] = N, int(d["tick"]), int(d["robot"])
    return out


def limits_profile(model, N, vlim):
    """what set_stage_limits(v_max = vlim) leaves in a fresh stage table: vlim [n][N+1] -> the speed rows of every
    stage at [-vlim_k, vlim_k], every other row the default box"""
    vlim = np.asarray(vlim, np.float64)
    P = sc.default_profile(model, N, len(vlim))
    ns = sc.speed_rows(model, P["ubx"].shape[2])
    P["ubx"][:, :, :ns] = vlim[:, :, None]
    P["lbx"][:, :, :ns] = -vlim[:, :, None]
    return P
