"""GPU tests of nmpc_batch_node_tick (csrc/node_gate.hip, k_node_order in schedule.hip, the solve kernels' active
count) against tests/node_ref.py, the fp64 restatement of NMPCNavControlROS::mainCycle's branches.

Tolerances: mode, event and the solve count are exact (node_ref refuses cases within 1e-9 of a threshold); path_u and
err are held to test_gpu_path_nearest.py's bars (d_gpu in [d_ref - 1e-12, d_ref + 1e-9] m, |U_gpu - U_ref| <= 1e-9
where the answer is separated and well conditioned, err equal to the oracle's at U_gpu to 1e-12); the reference poses
of path robots are bit-equal to nmpc_path_discretize from the same path_u; a solving robot's outputs and resident
state are bit-equal to nmpc_batch_run's on the same references, and a non-solving robot's state to a snapshot.
"""
import functools
import math

import numpy as np
import pytest
import torch

from nmpc_nav_control_amd._lib import default_params
from nmpc_nav_control_amd.batch import BatchSolver, NodeParams
from nmpc_nav_control_amd.path import discretize
from tests import node_ref as nr
from tests.path_cases import _line
from tests.path_nearest_ref import dist_at, near_err, nearest_one
from tests.test_gpu_path_nearest import follow_case, wrap_diff

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
N = 8
S = 4  # segment records per robot
NU = {"diff": 2, "omni4": 4, "tric": 2}


def dev(a, dtype=None):
    t = torch.from_numpy(np.array(a, order="C")).to(DEV)
    return t if dtype is None else t.to(dtype)


def params(**kw):
    return dict(nr.DEFAULT, **kw)


class Fleet:
    """Host arrays of B robots: mode [B], pose / goal [B][3] (fp32), vel [B][3], segs [B][S][16] (NaN past nseg),
    nseg, path_u, reset [B]."""

    def __init__(self, B):
        self.B = B
        self.mode = np.zeros(B, np.uint8)
        self.pose = np.zeros((B, 3), np.float32)
        self.vel = np.zeros((B, 3), np.float32)
        self.goal = np.full((B, 3), np.nan, np.float32)
        self.segs = np.full((B, S, 16), np.nan)
        self.nseg = np.ones(B, np.int32)
        self.path_u = np.zeros(B)
        self.reset = np.zeros(B, np.uint8)

    def set_path(self, i, recs, path_u=0.0):
        self.segs[i] = np.nan
        if len(recs):
            self.segs[i, :len(recs)] = recs
        self.nseg[i] = len(recs)
        self.path_u[i] = path_u

    def tile(self, k):
        f = Fleet(self.B * k)
        for name in ("mode", "pose", "vel", "goal", "segs", "nseg", "path_u", "reset"):
            a = getattr(self, name)
            setattr(f, name, np.concatenate([a] * k, 0))
        return f

    def ref(self, p, omni4=False):
        """node_ref of every robot (a NaN pose never reaches the path oracle: such robots are goal robots here)"""
        return [nr.node_ref(p, self.mode[i], self.pose[i].astype(np.float64), N,
                            goal=self.goal[i].astype(np.float64), segs=self.segs[i], nseg=self.nseg[i],
                            path_u=self.path_u[i], omni4=omni4) for i in range(self.B)]


class Tick:
    """Device copies of a fleet and the outputs of one node tick."""

    def __init__(self, f, model="diff", goal=True, paths=True):
        B = f.B
        self.B, self.f = B, f
        z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=DEV)  # noqa: E731
        self.mode, self.pose, self.vel = dev(f.mode), dev(f.pose.T), dev(f.vel.T)
        self.goal = dev(f.goal.T) if goal else None
        self.segs, self.nseg, self.path_u = (dev(f.segs), dev(f.nseg), dev(f.path_u)) if paths else (None, None, None)
        self.reset = dev(f.reset)
        self.steer = z(B) if model == "tric" else None
        self.event, self.err = z(B, dt=torch.uint8), z(2, B, dt=torch.float64)
        self.traj, self.n = torch.full((N + 1, 3, B), 7.0, device=DEV), z(1, dt=torch.int32)
        self.cmd, self.u0, self.qp_res = z(3, B) + 5, z(NU[model], B) + 5, z(3, B) + 5
        self.status, self.qp_iter = z(B, dt=torch.int32) + 5, z(B, dt=torch.int32) + 5

    def run(self, solver, p):
        solver.node_tick(NodeParams(**p), self.mode, self.pose, self.vel, goal=self.goal, segs=self.segs,
                         nseg=self.nseg, path_u=self.path_u, steer=self.steer, reset=self.reset, event=self.event,
                         err=self.err, traj_out=self.traj, n_solved=self.n, cmd=self.cmd, u0=self.u0,
                         status=self.status, qp_iter=self.qp_iter, qp_res=self.qp_res)
        torch.cuda.synchronize()

    def outs(self):
        return dict(cmd=self.cmd, u0=self.u0, status=self.status, qp_iter=self.qp_iter, qp_res=self.qp_res)

    def solved(self):
        ev = self.event.cpu().numpy()
        return (ev == nr.EV_SOLVED) | (ev == nr.EV_SOLVE_FAILED)


def check_gate(t, ref, p, omni4=False):
    """mode, event, count, path_u, err and the reference poses of one tick against node_ref"""
    f, B = t.f, t.B
    status = t.status.cpu().numpy()
    ref = [nr.after_solve(r, status[i]) for i, r in enumerate(ref)]
    mode, ev = t.mode.cpu().numpy(), t.event.cpu().numpy()
    assert [int(v) for v in mode] == [r.mode for r in ref]
    assert [int(v) for v in ev] == [r.event for r in ref]
    solves = np.array([r.solves for r in ref])
    assert int(t.n.cpu()) == solves.sum()
    U, err, traj = t.path_u.cpu().numpy(), t.err.cpu().numpy(), t.traj.cpu().numpy()
    searched = np.array([int(f.mode[i]) == nr.FOLLOW_PATH and f.nseg[i] >= 1 for i in range(B)])
    assert (U[~searched] == f.path_u[~searched]).all() and np.isnan(err[:, ~searched]).all()
    check = np.flatnonzero(searched)
    if B > 300:  # a tiled fleet (mixed_fleet): every tile bit-equal to the first, which goes to the oracle
        for a in (U, err[0], err[1]):
            a = a.reshape(B // 205, 205)
            assert np.array_equal(a, np.broadcast_to(a[0], a.shape), equal_nan=True)
        check = check[check < 205]
    for i in check:
        pose = f.pose[i].astype(np.float64)
        n = int(f.nseg[i])
        Ur, dr, gap, cond = nearest_one(f.segs[i], n, pose[:2], (f.path_u[i], math.nan))
        d = dist_at(f.segs[i:i + 1], f.nseg[i:i + 1], U[i:i + 1], pose[None, :2])[0]
        assert dr - 1e-12 <= d <= dr + 1e-9, (i, d - dr)
        if gap >= 1e-6 and cond >= 0.05:
            assert abs(U[i] - Ur) <= 1e-9, (i, U[i] - Ur)
        assert U[i] >= f.path_u[i]
        _, ee = near_err(f.segs[i], n, U[i], pose, omni4)
        assert abs(err[0, i] - ee[0]) <= 1e-12 and wrap_diff(err[1, i], ee[1]) <= 1e-12, i
    # reference poses: NaN for the robots that do not solve, the goal repeated, or the discretizer's from path_u
    assert np.isnan(traj[:, :, ~solves]).all()
    for i in np.flatnonzero(solves):
        if ref[i].traj_len == 1:
            assert (traj[:, :, i] == f.goal[i][None, :]).all(), i
    pr = np.flatnonzero(solves & searched)
    if len(pr):
        want = discretize(dev(f.segs[pr]), dev(f.nseg[pr]), dev(U[pr]), p["sample_period"], N + 1,
                          bool(p["is_holonomic"]))
        torch.cuda.synchronize()
        assert np.array_equal(want.cpu().numpy(), traj[:, :, pr])
    return ref


# ---- 1. branch table -------------------------------------------------------------------------------------------------
LINE = [_line((0, 0), (2, 0), 0.5)]


@functools.lru_cache(maxsize=None)
def branch_fleet():
    """37 hand-built robots covering every row of the semantics list (two full gate waves and a partial one)"""
    f = Fleet(37)
    rows = [
        (nr.IDLE, (0, 0, 0), None, None),
        (nr.ERROR, (0, 0, 0), None, None),
        (nr.BREAK, (0.2, 0.1, 0), None, None),
        (9, (0, 0, 0), None, None),                        # out-of-range mode bytes
        (255, (0, 0, 0), None, None),
        (nr.GOTO_POSE, (0, 0, 0), (2.5, 0, 0), None),      # too far (guard on)
        (nr.GOTO_POSE, (0, 0, 0), (1.9, 0, 0.4), None),    # just inside the guard
        (nr.GOTO_POSE, (0.003, 0.004, 0.5 * nr.DEG), (0, 0, 0), None),  # arrived
        (nr.GOTO_POSE, (0.003, 0.004, 2 * nr.DEG), (0, 0, 0), None),    # heading still off
        (nr.GOTO_POSE, (0.03, 0, 0), (0, 0, 0), None),     # 3 cm: not yet
        (nr.GOTO_POSE, (0.003, 0.004, 0.0), (0, 0, 1.0), None),  # ang = -1 rad: arrived only under the signed rule
        (nr.GOTO_POSE, (0.003, 0.004, 1.0), (0, 0, 0.0), None),  # ang = +1 rad: never
        (nr.GOTO_POSE, (1.0, -1.0, 0.3), (1.4, -0.8, 0.5), None),
        (nr.FOLLOW_PATH, (0.5, 0.1, 0.2), None, []),       # nseg = 0
        (nr.FOLLOW_PATH, (0.5, 0.1, 0.2), None, LINE),     # on the path
        (nr.FOLLOW_PATH, (0.5, 0.6, 0.2), None, LINE),     # position threshold alone
        (nr.FOLLOW_PATH, (0.5, 0.1, 1.2), None, LINE),     # orientation threshold alone
        (nr.FOLLOW_PATH, (0.5, 0.6, 1.2), None, LINE),     # both
        (nr.FOLLOW_PATH, (1.994, 0.0, 0.0), None, LINE),   # 6 mm before the end: arrived
        (nr.FOLLOW_PATH, (1.994, 0.0, -1.0), None, LINE),  # and with ang = -1 rad: arrived only under the signed rule
        (nr.FOLLOW_PATH, (1.9, 0.0, 0.0), None, LINE),     # 10 cm before the end: padded poses, still solving
        (nr.FOLLOW_PATH, (0.5, 0.1, 0.2), None, LINE, 0.4),  # the search starts at path_u
        (nr.FOLLOW_PATH, (0.5, 0.1, -3.0), None, [_line((0, 0), (2, 0), -0.5)]),  # driven backwards: heading + pi
        (nr.FOLLOW_PATH, (0.45, 0.2, 1.4), None,
         [_line((0, 0), (0.5, 0), 0.8), _line((0.5, 0), (0.5, 0.5), 0.2), _line((0.5, 0.5), (2, 0.5), 1.2)]),
    ]
    segs, nseg, pose, vel, _ = follow_case(13, 41, max_segs=S)  # seeded paths for the rest
    for k in range(13):
        rows.append((nr.FOLLOW_PATH, pose[k], None, list(segs[k, :nseg[k]])))
    assert len(rows) == f.B
    for i, row in enumerate(rows):
        f.mode[i], f.pose[i] = row[0], row[1]
        if row[2] is not None:
            f.goal[i] = row[2]
        if row[3] is not None:
            f.set_path(i, row[3], row[4] if len(row) > 4 else 0.0)
    f.vel[:, 0] = 0.1
    f.reset[::3] = 1
    return f


@pytest.mark.parametrize("over", [{}, {"enable_safe_conditions": 0}, {"max_pos_err": math.inf},
                                  {"max_ori_err": math.inf}, {"final_ori_signed": 0}],
                         ids=["default", "safe_off", "pos_inf", "ori_inf", "abs_angle"])
def test_branch_table(built, over):
    f, p = branch_fleet(), params(**over)
    ref = f.ref(p)
    t = Tick(f)
    t.run(BatchSolver("diff", N, f.B, device=DEV), p)
    ref = check_gate(t, ref, p)
    ev = [r.event for r in ref]
    if not over:
        assert {nr.EV_NONE, nr.EV_SOLVED, nr.EV_ARRIVED, nr.EV_GOAL_TOO_FAR, nr.EV_OFF_PATH, nr.EV_BREAK} <= set(ev)
        assert ev[5] == nr.EV_GOAL_TOO_FAR and ev[10] == ev[19] == nr.EV_ARRIVED
        assert ev[15] == ev[16] == ev[17] == nr.EV_OFF_PATH and ev[13] == nr.EV_NONE and ref[13].mode == nr.IDLE
    expect = {"enable_safe_conditions": {5: nr.EV_SOLVED, 15: nr.EV_SOLVED, 16: nr.EV_SOLVED, 17: nr.EV_SOLVED},
              "max_pos_err": {15: nr.EV_SOLVED, 16: nr.EV_OFF_PATH, 17: nr.EV_OFF_PATH},
              "max_ori_err": {15: nr.EV_OFF_PATH, 16: nr.EV_SOLVED, 17: nr.EV_OFF_PATH},
              "final_ori_signed": {10: nr.EV_SOLVED, 19: nr.EV_SOLVED, 7: nr.EV_ARRIVED}}
    for k in over:
        for i, e in expect[k].items():
            assert ev[i] == e, (k, i)
    # the pending reset: consumed by the robots that solved, kept by the others
    solves = np.array([r.solves for r in ref])
    assert (t.reset.cpu().numpy() == np.where(solves, 0, f.reset)).all()


# ---- 2 / 3. solving robots are unchanged solves, the others are untouched -------------------------------------------
@functools.lru_cache(maxsize=None)
def mixed_fleet(B, seed=3):
    """A seeded mixed fleet (about 60 % of the robots solve); above 300 robots a block of 205 repeated"""
    if B > 300:
        assert B % 205 == 0
        return mixed_fleet(205, seed).tile(B // 205)
    rng = np.random.default_rng(seed)
    segs, nseg, pose, vel, normal = follow_case(B, seed + 100, max_segs=S)
    f = Fleet(B)
    f.pose[:], f.vel[:] = pose, vel
    kinds = rng.choice(["idle", "error", "break", "bad", "goto", "goto_here", "goto_far", "follow", "follow_off",
                        "follow_end", "follow_empty"], B,
                       p=[0.1, 0.04, 0.04, 0.02, 0.3, 0.04, 0.03, 0.3, 0.05, 0.05, 0.03])
    kinds[:4] = ["goto", "idle", "follow", "goto"]  # (every fleet has both solving kinds, B = 5 included)
    for i, k in enumerate(kinds):
        x, y, th = (float(v) for v in f.pose[i])
        if k.startswith("goto"):
            f.mode[i] = nr.GOTO_POSE
            r = {"goto": rng.uniform(0.1, 1.5), "goto_here": 0.0, "goto_far": 2.5}[k]
            a = rng.uniform(-math.pi, math.pi)
            f.goal[i] = (x + r * math.cos(a), y + r * math.sin(a), th + (0.3 if k == "goto_here" else rng.uniform(-1, 1)))
        elif k.startswith("follow"):
            f.mode[i] = nr.FOLLOW_PATH
            f.set_path(i, segs[i, :nseg[i]])
            if k == "follow_off":
                f.pose[i, :2] += 3.0 * normal[i]
            elif k == "follow_end":
                en, _ = near_err(segs[i], int(nseg[i]), float(nseg[i]), (0.0, 0.0, 0.0))
                f.pose[i] = (en[0], en[1], en[2] - 0.1)
            elif k == "follow_empty":
                f.nseg[i] = 0
        else:
            f.mode[i] = {"idle": nr.IDLE, "error": nr.ERROR, "break": nr.BREAK, "bad": 200}[k]
    f.reset[:] = rng.uniform(size=B) < 0.3
    return f


@functools.lru_cache(maxsize=None)
def mixed_ref(B, omni4):
    f = mixed_fleet(B)
    if B > 300:
        return mixed_ref(205, omni4) * (B // 205)
    return f.ref(params(), omni4)


def warm_up(solvers, f, model, ticks=2):
    """the same plain run ticks on every handle, so that iterates, carried refs, warm flags and keys are non-trivial"""
    B = f.B
    rng = np.random.default_rng(9)
    off = rng.uniform(-0.5, 0.5, (B, 3)).astype(np.float32)
    traj = dev(np.broadcast_to((f.pose + off).T[None], (N + 1, 3, B)))
    steer = torch.zeros(B, device=DEV) if model == "tric" else None
    for s in solvers:
        for _ in range(ticks):
            s.run(dev(f.pose.T), dev(f.vel.T), traj, steer=steer)
    torch.cuda.synchronize()


def state_of(s):
    return [v.to_tensor() for v in s.state()] + [s.warm_state()[0].to_tensor()]


FORMS = {"split": (5, {"NMPC_AMD_ROWPAR_MAX": "0"}, "team"), "rowpar": (70, {}, "rowpar"),
         "team": (70, {"NMPC_AMD_ROWPAR_MAX": "0", "NMPC_AMD_SPLIT_MAX": "0"}, "team"), "dense": (4100, {}, "team")}


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("model", ["diff", "omni4", "tric"])
def test_solvers_match_run_and_the_rest_is_untouched(built, monkeypatch, model, form):
    B, env, kernel = FORMS[form]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    f, p = mixed_fleet(B), params()
    ref = mixed_ref(B, model == "omni4")
    A, R = (BatchSolver(model, N, B, device=DEV) for _ in range(2))
    assert A.plan_ex(B, "run")["kernel"] == kernel
    warm_up((A, R), f, model)
    before = state_of(A)
    for a, b in zip(before, state_of(R)):
        assert torch.equal(a, b)
    t = Tick(f, model)
    t.run(A, p)
    ref = check_gate(t, ref, p, model == "omni4")
    solves = np.array([r.solves for r in ref])
    assert 0 < solves.sum() < B and (t.solved() == solves).all()
    # handle R: nmpc_batch_run at the same B on the references node_ref predicts, the pending resets applied
    traj = np.broadcast_to(f.pose.T[None], (N + 1, 3, B)).copy()
    tlen = np.ones(B, np.int32)
    gt = t.traj.cpu().numpy()
    for i in np.flatnonzero(solves):
        tlen[i] = ref[i].traj_len
        traj[:, :, i] = f.goal[i][None, :] if tlen[i] == 1 else gt[:, :, i]  # (gt: checked against the discretizer)
    o = Tick(f, model)
    R.run(o.pose, o.vel, dev(traj), steer=o.steer, traj_len=dev(tlen), reset=dev(f.reset), **o.outs())
    torch.cuda.synchronize()
    sv, ns = dev(np.flatnonzero(solves)), dev(np.flatnonzero(~solves))
    for k, a in t.outs().items():
        assert torch.equal(a[..., sv], o.outs()[k][..., sv]), k
        assert (a[..., ns] == 0).all(), k
    after = state_of(A)
    for k, (a, b, c) in enumerate(zip(after, state_of(R), before)):
        assert torch.equal(a[:, sv], b[:, sv]), k     # solving robots: the state nmpc_batch_run leaves
        assert torch.equal(a[:, ns], c[:, ns]), k     # the others: the snapshot
    assert not torch.equal(after[0][:, sv], before[0][:, sv])
    reset = t.reset.cpu().numpy()
    assert (reset[solves] == 0).all() and (reset[~solves] == f.reset[~solves]).all()


# ---- 4. placement changes nothing -----------------------------------------------------------------------------------
def test_placement_changes_nothing(built, monkeypatch):
    B = 70
    monkeypatch.setenv("NMPC_AMD_ROWPAR_MAX", "0")
    monkeypatch.setenv("NMPC_AMD_SPLIT_MAX", "0")
    f, p = mixed_fleet(B), params()
    ticks = []
    for sched in ("off", "sorted"):
        s = BatchSolver("diff", N, B, device=DEV)
        s.set_schedule(sched)
        warm_up((s,), f, "diff")
        t = Tick(f)
        for _ in range(3):  # two warm-up node ticks, then the compared one: the placement keys differ by now
            t.reset[:] = dev(f.reset)
            t.run(s, p)
        ticks.append((t, state_of(s)))
    (a, sa), (b, sb) = ticks
    assert int(a.n.cpu()) > 4 and len(set(a.qp_iter.cpu().numpy().tolist())) > 2
    for k in a.outs():
        assert torch.equal(a.outs()[k], b.outs()[k]), k
    for x, y in ((a.mode, b.mode), (a.event, b.event), (a.path_u, b.path_u), (a.n, b.n), (a.reset, b.reset)):
        assert torch.equal(x, y)
    assert torch.equal(torch.nan_to_num(a.err, nan=-9.0), torch.nan_to_num(b.err, nan=-9.0))
    assert torch.equal(torch.nan_to_num(a.traj, nan=-9.0), torch.nan_to_num(b.traj, nan=-9.0))
    for x, y in zip(sa, sb):
        assert torch.equal(x, y)


# ---- 5. edges -------------------------------------------------------------------------------------------------------
def small_fleet(B, active):
    """B goal robots 0.5 m from their goals, of which only `active` are in GOTO_POSE (the rest Idle)"""
    f = Fleet(B)
    f.pose[:, 0] = np.arange(B)
    f.goal[:] = f.pose + np.array([0.4, 0.3, 0.2], np.float32)
    f.mode[list(active)] = nr.GOTO_POSE
    return f


def test_all_idle(built):
    f = small_fleet(9, [])
    s = BatchSolver("diff", N, 9, device=DEV)
    warm_up((s,), f, "diff")
    before = state_of(s)
    t = Tick(f)
    t.run(s, params())
    assert int(t.n.cpu()) == 0 and (t.event == nr.EV_NONE).all() and (t.mode == nr.IDLE).all()
    for a, b in zip(state_of(s), before):
        assert torch.equal(a, b)
    for k, a in t.outs().items():
        assert (a == 0).all(), k
    assert torch.isnan(t.traj).all()


@pytest.mark.parametrize("active", [[4], [0, 3, 5, 8], [1, 2, 4, 6, 7], list(range(9))])
def test_active_counts(built, active):
    """1, 4, 5 and 9 of 9 robots solve, each exactly as in a plain run of the whole fleet"""
    B = 9
    f = small_fleet(B, active)
    A, R = (BatchSolver("diff", N, B, device=DEV) for _ in range(2))
    warm_up((A, R), f, "diff")
    before = state_of(A)
    t = Tick(f)
    t.run(A, params())
    check_gate(t, f.ref(params()), params())
    assert int(t.n.cpu()) == len(active)
    o = Tick(f)
    R.run(o.pose, o.vel, dev(np.broadcast_to(f.goal.T[None], (N + 1, 3, B))),
          traj_len=torch.ones(B, dtype=torch.int32, device=DEV), **o.outs())
    torch.cuda.synchronize()
    sv = dev(np.array(active))
    ns = dev(np.setdiff1d(np.arange(B), active))
    for k, a in t.outs().items():
        assert torch.equal(a[..., sv], o.outs()[k][..., sv]) and (a[..., ns] == 0).all(), k
    for a, b, c in zip(state_of(A), state_of(R), before):
        assert torch.equal(a[:, sv], b[:, sv]) and torch.equal(a[:, ns], c[:, ns])


def test_one_robot(built):
    for mode, n in ((nr.GOTO_POSE, 1), (nr.IDLE, 0)):
        f = small_fleet(1, [0] if mode == nr.GOTO_POSE else [])
        t = Tick(f)
        t.run(BatchSolver("diff", N, 1, device=DEV), params())
        check_gate(t, f.ref(params()), params())
        assert int(t.n.cpu()) == n and int(t.status.cpu()[0]) == 0
        assert bool((t.cmd != 0).any()) == bool(n)


def test_missing_inputs_are_an_error(built):
    f = small_fleet(5, [0, 2])
    f.mode[3] = nr.FOLLOW_PATH
    f.set_path(3, LINE)
    t = Tick(f, goal=False, paths=False)
    t.run(BatchSolver("diff", N, 5, device=DEV), params())
    assert t.mode.cpu().tolist() == [nr.ERROR, nr.IDLE, nr.ERROR, nr.ERROR, nr.IDLE]
    assert (t.event == nr.EV_NONE).all() and int(t.n.cpu()) == 0 and (t.cmd == 0).all()


def test_nan_pose_fails_alone(built):
    B = 9
    f = small_fleet(B, range(B))
    f.mode[6] = nr.IDLE
    g = small_fleet(B, range(B))
    g.mode[6] = nr.IDLE
    g.pose[2, 1] = np.nan
    runs = []
    for fl in (f, g):
        s = BatchSolver("diff", N, B, device=DEV)
        warm_up((s,), f, "diff")
        t = Tick(fl)
        t.run(s, params())
        runs.append((t, state_of(s)))
    (a, sa), (b, sb) = runs
    assert int(b.status.cpu()[2]) == 1 and int(b.event.cpu()[2]) == nr.EV_SOLVE_FAILED
    assert int(b.mode.cpu()[2]) == nr.ERROR and (b.cmd[:, 2] == 0).all() and int(b.n.cpu()) == B - 1
    keep = dev(np.setdiff1d(np.arange(B), [2]))
    for k in a.outs():
        assert torch.equal(a.outs()[k][..., keep], b.outs()[k][..., keep]), k
    assert torch.equal(a.mode[keep], b.mode[keep]) and torch.equal(a.event[keep], b.event[keep])
    for x, y in zip(sa, sb):
        assert torch.equal(x[:, keep], y[:, keep])
    assert (a.status == 0).all()


def test_argument_errors_with_a_handle(built):
    s = BatchSolver("diff", N, 4, device=DEV)
    f = small_fleet(4, [0])
    t = Tick(f)
    with pytest.raises(ValueError, match="capacity"):
        Tick(small_fleet(5, [0])).run(s, params())
    with pytest.raises(RuntimeError, match="sample_period"):
        t.run(s, params(sample_period=math.nan))
    with pytest.raises(TypeError):
        t.mode = t.mode.to(torch.int32)
        t.run(s, params())


# ---- 6. closed loop -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["diff", "omni4"])
def test_closed_loop(built, model):
    """16 goal robots, 16 path robots and 16 Idle ones, 40 ticks on the harness plant (nmpc_fleet_sim_step): at every
    tick mode and event equal node_ref on that tick's device poses, robots of both moving kinds arrive inside the
    window, and an arrived robot's resident state stays frozen."""
    B, T = 48, 40
    omni4 = model == "omni4"
    # arrival within 5 cm and (signed) 0.2 rad; omni4 follows the paths' holonomic heading, 1.2 rad off the tangent
    p = params(final_pos_err=0.05, final_ori_err=0.2, is_holonomic=1 if omni4 else 0)
    f = Fleet(B)
    rng = np.random.default_rng(11)
    for i in range(B):
        x, y, th = rng.uniform(-2, 2), rng.uniform(-2, 2), rng.uniform(-math.pi, math.pi)
        hold = th + 1.2 if omni4 else th  # the heading the robot holds
        f.pose[i] = (x, y, hold)
        k = i % 16
        c, s_ = math.cos(th), math.sin(th)
        if i < 16:
            f.mode[i] = nr.GOTO_POSE
            r = 0.052 + 0.006 * k
            f.goal[i] = (x + r * c, y + r * s_, hold - 0.05)
        elif i < 32:
            f.mode[i] = nr.FOLLOW_PATH
            L = 0.055 + 0.004 * k
            f.set_path(i, [_line((x, y), (x + L * c, y + L * s_), 0.5, hold, hold)])
    f.reset[:] = 1
    prm = default_params(model, N)
    if omni4:
        # omni4 has no terminal-weight hack: with the shipped pose weights a robot 10 cm from its goal pulls with
        # 1 cm/s^2 and covers 2 mm in 27 ticks, so nothing would arrive inside the window
        for k in range(3):
            prm.W[k] *= 100.0
            prm.W_e[k] *= 100.0
    s = BatchSolver(model, N, B, params=prm, device=DEV)
    t = Tick(f, model)
    hp = torch.zeros(6, B, device=DEV)
    hp[5] = -1.0  # (the harness's own references are not used)
    hs, htraj, hlen = torch.zeros(B, device=DEV), torch.zeros(N + 1, 3, B, device=DEV), torch.zeros(
        B, dtype=torch.int32, device=DEV)
    arrived_at, frozen = {}, {}
    for tick in range(T):
        f.mode, f.path_u = t.mode.cpu().numpy().copy(), t.path_u.cpu().numpy().copy()
        f.pose = t.pose.cpu().numpy().T.copy()
        ref = f.ref(p, omni4)
        t.run(s, p)
        status = t.status.cpu().numpy()
        ref = [nr.after_solve(r, status[i]) for i, r in enumerate(ref)]
        mode, ev = t.mode.cpu().numpy(), t.event.cpu().numpy()
        assert [int(v) for v in mode] == [r.mode for r in ref], tick
        assert [int(v) for v in ev] == [r.event for r in ref], tick
        st = [x.cpu().numpy() for x in state_of(s)]
        for i in range(B):
            if ev[i] == nr.EV_ARRIVED:
                arrived_at[i] = tick
                frozen[i] = [x[:, i].copy() for x in st]
            elif i in frozen:
                assert mode[i] == nr.IDLE and ev[i] == nr.EV_NONE
                for x, y in zip(st, frozen[i]):
                    assert np.array_equal(x[:, i], y), (tick, i)
        s.fleet_sim_step(hp, hs, t.pose, t.vel, None, t.u0, t.status, htraj, hlen, advance=True)
    print("arrivals (robot: tick):", arrived_at, "final modes:", t.mode.cpu().tolist())
    goal_arr = [i for i in arrived_at if i < 16]
    path_arr = [i for i in arrived_at if 16 <= i < 32]
    assert len(goal_arr) >= 2 and len(path_arr) >= 2
    assert max(arrived_at[i] for i in goal_arr) > 0 and max(arrived_at[i] for i in path_arr) > 0
    assert (t.mode[32:] == nr.IDLE).all()
