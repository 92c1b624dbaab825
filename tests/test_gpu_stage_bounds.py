"""GPU tests of the stage table (csrc/robot_tables.hip, stage_box in csrc/sqp_steps.hpp) against one fp64 solve per
robot on the QP with the profile's bounds spliced in (tests/stage_bound_cases.py).

Tolerance of the oracle comparisons: test_gpu_parity.py's, |u0 - u0_oracle|_inf and |cmd - cmd_oracle|_inf <= 1e-3 with
every status 0. One stage of the ramp is 0.02 of bound, which is 0.8 in u0 where stage 1 is active, so a library that
ignores the table or reads the neighbouring stage cannot pass. Everything else here is exact (torch.equal).
"""
import functools

import numpy as np
import pytest
import torch

from nmpc_nav_control_amd.batch import BatchSolver
from oracle.oracle import Oracle, path_discretize
from tests import node_ref as nr
from tests import queue_cases as qc
from tests import robot_param_cases as rc
from tests import stage_bound_cases as sc
from tests.path_cases import random_paths
from tests.test_gpu_node import N as NODE_N
from tests.test_gpu_node import Tick, mixed_fleet
from tests.test_gpu_node import params as node_params
from tests.test_gpu_queue import QTick
from tests.table_harness import CASES, FORMS, MODELS, TOL_U, Loop, make_solver, state_of, t, table_args

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
T0 = sc.T0


def upload(solver, P, mask=None, fields=sc.FIELDS):
    """a profile dict [B][stages][n] into the solver's stage table ([stages][n][B] on the device)"""
    solver.set_stage_bounds(**{k: t(P[k].transpose(1, 2, 0)) for k in fields}, mask=mask)


def cm_of(loop):
    return sc.speed_of(loop.model, loop.carried().cpu().numpy().T)


def table_bytes(solver):
    torch.cuda.synchronize()
    return solver.stage_bounds().to_tensor()


def check_tick(loop, fleet, inp, tick, P):
    """one tick's u0 / cmd / status against the spliced reference on the same inputs; no robot is left out"""
    cmd_o, u0_o, st_o, it_o = fleet.tick(*inp, P=P)
    st = loop.out["status"].cpu().numpy()
    eu = np.abs(loop.out["u0"].cpu().numpy().T - u0_o).max()
    ec = np.abs(loop.out["cmd"].cpu().numpy().T - cmd_o).max()
    print(f"tick {tick}: oracle status {st_o.tolist()} iters <= {it_o.max()}; device status {st.tolist()} iters "
          f"{loop.out['qp_iter'].cpu().numpy().tolist()}; |du0| {eu:.2e} |dcmd| {ec:.2e}")
    assert (st_o == 0).all(), (tick, st_o)
    assert (st == 0).all(), (tick, st)
    assert eu <= TOL_U, (tick, eu)
    assert ec <= TOL_U, (tick, ec)


# ---- 1. the ramp in closed loop, in every launch form ----------------------------------------------------------------
def ramp_closed_loop(monkeypatch, model, form, N, advance, T=12):
    B = 12
    solver = make_solver(monkeypatch, model, N, B, form)
    plan = solver.plan_ex(B, "run")
    assert FORMS[form][2](plan), plan
    loop = Loop(solver, model, B)
    _, fleet = sc.default_fleet(model, N, B)
    P, cm = None, None
    for tick in range(T):
        if tick == T0:
            assert solver.stage_bounds() is None  # (the table is off until the first writer)
            cm = cm_of(loop)
        if tick >= T0:
            if advance == "shift" and tick > T0:
                solver.shift_stage_bounds(1, B=B)
                P = sc.shifted(P, 1)
            else:
                P = sc.profile(model, N, cm, tick)
                upload(solver, P)
        inp = loop.host_inputs()
        loop.run()
        check_tick(loop, fleet, inp, tick, P)
        loop.advance()


@pytest.mark.parametrize("model,form,advance", [(m, f, ("shift", "upload")[k % 2]) for k, (m, f) in enumerate(CASES)])
def test_ramp_closed_loop(built, monkeypatch, model, form, advance):
    ramp_closed_loop(monkeypatch, model, form, 20, advance)


TEAM_FORMS = [("diff", f) for f in ("team_split_launch", "team_plain", "rec_split", "mehrotra")] + \
    [("omni4", "team_plain"), ("tric", "team_plain")]


@pytest.mark.parametrize("N", [21, 22])
@pytest.mark.parametrize("model,form", TEAM_FORMS)
def test_ramp_closed_loop_rotation_remainders(built, monkeypatch, model, form, N):
    """N + 1 = 22 and 23: with N = 20 the team kernel's three-row rotation of P0 ends on each of its remainders. (The
    CPU conditions of the rule hold for these N as well: every oracle status is asserted 0 on every tick.)"""
    ramp_closed_loop(monkeypatch, model, form, N, "upload" if N == 21 else "shift", T=8)


# ---- 2. the ramp succeeds where the abrupt drop fails ----------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
def test_ramp_succeeds_where_the_abrupt_drop_fails(built, model):
    """test_abrupt_drop_fails_those_robots_alone's scenario with the ramp in place of the drop: every solve succeeds,
    the even robots brake into their targets, and the odd robots are bit-identical to a handle without a table."""
    N, B, T = 20, 12, 24
    ramp, ref = (BatchSolver(model, N, B, device=DEV) for _ in range(2))
    a, b = Loop(ramp, model, B), Loop(ref, model, B)
    ev, od = torch.arange(0, B, 2, device=DEV), torch.arange(1, B, 2, device=DEV)
    cm = None
    for tick in range(T):
        if tick == T0:
            cm = cm_of(a)
        if tick >= T0:
            upload(ramp, sc.profile(model, N, cm, tick))
        a.run()
        b.run()
        assert (a.out["status"] == 0).all(), (tick, a.out["status"])
        assert (a.out["cmd"].abs().sum(dim=0) > 0).all(), tick
        for k in a.out:
            assert torch.equal(a.out[k][..., od], b.out[k][..., od]), (tick, k)
        for k, (x, y) in enumerate(zip(state_of(ramp), state_of(ref))):
            assert torch.equal(x[:, od], y[:, od]), (tick, k)
        if tick == 8:
            assert (a.out["u0"][:, ev] != b.out["u0"][:, ev]).any(dim=0).sum() >= len(ev) - 1
        a.advance()
        b.advance()
    speed = cm_of(a)
    print("speed", speed[0::2].tolist(), "target", (0.3 * cm[0::2]).tolist())
    assert (speed[0::2] <= 0.3 * cm[0::2] * 1.001).all()


# ---- 3. a uniform profile changes nothing ----------------------------------------------------------------------------
def uniform_pair(monkeypatch, model, N, B, form, source):
    """two solvers of one form, the second with a stage table that holds the launch's own box at every stage (source:
    "handle", or "robot": a per-robot table on both)"""
    off, on = (make_solver(monkeypatch, model, N, B, form) for _ in range(2))
    if source == "robot":
        for s in (off, on):
            s.set_robot_params(**table_args(rc.robot_params(model, N, B)))
    on.shift_stage_bounds(0)  # (the first writer fills the table from what the launches used until now)
    assert off.stage_bounds() is None and on.stage_bounds() is not None
    return off, on


@pytest.mark.parametrize("source", ["handle", "robot"])
@pytest.mark.parametrize("model,form", CASES)
def test_uniform_profile_is_bit_identical_run(built, monkeypatch, model, form, source):
    N, B = 20, 15
    off, on = uniform_pair(monkeypatch, model, N, B, form, source)
    assert FORMS[form][2](on.plan_ex(B, "run"))
    a, b = Loop(off, model, B), Loop(on, model, B)
    for tick in range(3):
        a.run()
        b.run()
        for k in a.out:
            assert torch.equal(a.out[k], b.out[k]), (tick, k)
        for k, (x, y) in enumerate(zip(state_of(off), state_of(on))):
            assert torch.equal(x, y), (tick, k)
        a.advance()
        b.advance()
    assert (a.out["status"] == 0).all()


@functools.lru_cache(maxsize=None)
def solve_data(model="diff", N=20, B=12, tick=5):
    """the ramp loop's solve inputs of one tick per robot: (xbar, ubar, x0, yref, We) and the robot's box"""
    kept = []

    def hook(tk, i, o, args, box):
        if tk == tick:
            kept.append((args, box))

    sc.cpu_closed_loop(model, N, B, tick + 1, "ramp", hook=hook)
    return kept


def packed(kept):
    xbar = t(np.stack([a[0] for a, _ in kept]).reshape(len(kept), -1).T)
    ubar = t(np.stack([a[1] for a, _ in kept]).reshape(len(kept), -1).T)
    x0 = t(np.stack([a[2] for a, _ in kept]).T)
    yref = t(np.stack([a[3] for a, _ in kept]).transpose(1, 2, 0))
    We = np.stack([a[4] for a, _ in kept])
    P = {k: np.stack([b[k] for _, b in kept]) for k in sc.FIELDS}
    return xbar, ubar, x0, yref, We, P


@pytest.mark.parametrize("source", ["handle", "robot"])
@pytest.mark.parametrize("form", list(FORMS))
def test_uniform_profile_is_bit_identical_solve(built, monkeypatch, form, source):
    model, N, B = "diff", 20, 12
    xbar, ubar, x0, yref, _, _ = packed(solve_data())
    off, on = uniform_pair(monkeypatch, model, N, B, form, source)
    assert FORMS[form][2](on.plan_ex(B, "solve"))
    outs = []
    for s in (off, on):
        s.state()[0].copy_from(xbar)
        s.state()[1].copy_from(ubar)
        o = dict(u0=torch.zeros(s.nu, B, device=DEV), x1=torch.zeros(s.nx, B, device=DEV),
                 status=torch.full((B,), -7, dtype=torch.int32, device=DEV),
                 qp_iter=torch.zeros(B, dtype=torch.int32, device=DEV), qp_res=torch.zeros(3, B, device=DEV))
        for _ in range(2):
            s.solve(x0, yref, **o)
        torch.cuda.synchronize()
        outs.append(o)
    for k in outs[0]:
        assert torch.equal(outs[0][k], outs[1][k]), k
    for k, (x, y) in enumerate(zip(state_of(off), state_of(on))):
        assert torch.equal(x, y), k
    assert (outs[0]["status"] == 0).all()


@pytest.mark.parametrize("form", ["seg", "team_plain"])
@pytest.mark.parametrize("model", MODELS)
def test_both_tables(built, monkeypatch, model, form):
    """the per-robot table and the stage table on: W and W_e from the robot's column, the box from the stage table
    (here the default box at every stage, which is not the robot table's)"""
    N, B = 20, 12
    solver = make_solver(monkeypatch, model, N, B, form)
    R = rc.robot_params(model, N, B)
    solver.set_robot_params(**table_args(R))
    dflt = Oracle(model, N, rule="batched")
    P = {k: np.tile(v, (B, 1, 1)) for k, v in sc.uniform_box(dflt).items()}
    P = {k: v.astype(np.float32).astype(np.float64) for k, v in P.items()}
    assert any((P[k][:, 0] != R[k]).any() for k in sc.FIELDS)
    upload(solver, P)
    loop = Loop(solver, model, B)
    fleet = sc.StageFleet(rc.oracles(model, N, R), loop.fl["carried"].T)
    for tick in range(3):
        inp = loop.host_inputs()
        loop.run()
        check_tick(loop, fleet, inp, tick, P)
        loop.advance()


# ---- 4. shift ----------------------------------------------------------------------------------------------------------
def random_profile(model, N, B, seed):
    o = Oracle(model, N, rule="batched")
    rng = np.random.default_rng(seed)
    P = dict(lbx=-rng.uniform(0.1, 2, (B, N + 1, o.nbx)), ubx=rng.uniform(0.1, 2, (B, N + 1, o.nbx)),
             lbu=-rng.uniform(0.1, 2, (B, N, o.nbu)), ubu=rng.uniform(0.1, 2, (B, N, o.nbu)))
    return {k: v.astype(np.float32).astype(np.float64) for k, v in P.items()}


@pytest.mark.parametrize("n", [0, 1, 3, "N+5"])
@pytest.mark.parametrize("model", ["diff", "omni4"])
def test_shift(built, model, n):
    """shift(n) against a second handle given the shifted arrays directly, byte for byte; the masked robots and the
    robots past B keep their rows, and the last stage is repeated"""
    N, B, cap = 7, 300, 320  # (two blocks of the writers' robots, the second one partial)
    n = N + 5 if n == "N+5" else n
    P = random_profile(model, N, B, seed=17 + n)
    mask = np.arange(B) % 3 != 1
    a, b = (BatchSolver(model, N, cap, device=DEV) for _ in range(2))
    upload(a, P)
    a.shift_stage_bounds(n, mask=t(mask, torch.uint8), B=B)
    Q = sc.shifted(P, n)
    want = {k: np.where(mask[:, None, None], Q[k], P[k]) for k in P}
    for k in want:
        last = want[k].shape[1] - 1
        assert (want[k][mask][:, max(last - n, 0):] == P[k][mask][:, last:]).all()  # the last stage, repeated
    upload(b, want)
    assert torch.equal(table_bytes(a), table_bytes(b))
    assert table_bytes(a).numel() == (N + 1) * (2 * a.nbx + 2 * a.nbu) * cap * 4
    # the same through the mask of the writer, and field by field
    c = BatchSolver(model, N, cap, device=DEV)
    upload(c, P)
    for k in sc.FIELDS:
        upload(c, Q, mask=t(mask, torch.uint8), fields=(k,))
    assert torch.equal(table_bytes(a), table_bytes(c))


def test_stage_limits_writer(built):
    """the per-stage set_limits against set_stage_bounds with the mapped rows (tric: the steering rows their own)"""
    N, B = 6, 9
    rng = np.random.default_rng(3)
    for model in MODELS:
        a, b = (BatchSolver(model, N, B, device=DEV) for _ in range(2))
        o = Oracle(model, N, rule="batched")
        P = {k: np.tile(v, (B, 1, 1)) for k, v in sc.uniform_box(o).items()}
        v, acc = rng.uniform(0.2, 1, (N + 1, B)), rng.uniform(0.2, 1, (N, B))
        ns, na = (1, 1) if model == "tric" else (o.nbx, o.nbu)
        P["ubx"][:, :, :ns], P["lbx"][:, :, :ns] = v.T[:, :, None], -v.T[:, :, None]
        P["ubu"][:, :, :na], P["lbu"][:, :, :na] = acc.T[:, :, None], -acc.T[:, :, None]
        kw = dict(v_max=t(v), a_max=t(acc))
        if model == "tric":
            lo, hi, da = -rng.uniform(0.2, 1, (N + 1, B)), rng.uniform(0.2, 1, (N + 1, B)), rng.uniform(0.1, 1, (N, B))
            P["lbx"][:, :, 1], P["ubx"][:, :, 1] = lo.T, hi.T
            P["lbu"][:, :, 1], P["ubu"][:, :, 1] = -da.T, da.T
            kw.update(alpha_min=t(lo), alpha_max=t(hi), dalpha_max=t(da))
        a.set_stage_limits(**kw)
        upload(b, {k: x.astype(np.float32).astype(np.float64) for k, x in P.items()})
        assert torch.equal(table_bytes(a), table_bytes(b)), model


# ---- 5. NaN and crossed bounds ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ["state_N", "input_0"])
@pytest.mark.parametrize("form", ["seg", "serial", "team_split_launch", "team_plain"])
def test_nan_and_crossed_bounds_fail_alone(built, monkeypatch, form, entry):
    """A NaN in a used entry (a state bound at stage N / an input bound at stage 0): status 1 and a stop command on
    that robot alone, its iterate and carried refs kept. NaN in the unused state rows of stage 0 of every robot changes
    nothing. lb > ub at one stage: a nonzero status on that robot alone."""
    model, N, B = "diff", 20, 12
    off, ref, bad = (make_solver(monkeypatch, model, N, B, form) for _ in range(3))
    o = Oracle(model, N, rule="batched")
    P = {k: np.tile(v, (B, 1, 1)) for k, v in sc.uniform_box(o).items()}
    P["lbx"][:, 0], P["ubx"][:, 0] = np.nan, np.nan
    upload(ref, P)
    if entry == "state_N":
        P["ubx"][2, N, 1] = np.nan
    else:
        P["lbu"][2, 0, 0] = np.nan
    P["lbu"][7, 4, 1], P["ubu"][7, 4, 1] = 0.5, -0.5
    upload(bad, P)
    loops = [Loop(s, model, B) for s in (off, ref, bad)]
    for lp in loops:
        lp.run()
        lp.advance()
    before = state_of(bad)
    for lp in loops:
        lp.run()
    c, a, b = loops
    for k in a.out:
        assert torch.equal(c.out[k], a.out[k]), k  # NaN in the unused entries
    st = b.out["status"].cpu().numpy()
    assert st[2] == 1 and st[7] != 0, st
    keep = torch.tensor([i for i in range(B) if i not in (2, 7)], device=DEV)
    assert (st[keep.cpu().numpy()] == 0).all() and (a.out["status"] == 0).all()
    for k in a.out:
        assert torch.equal(a.out[k][..., keep], b.out[k][..., keep]), k
    for k, (x, y) in enumerate(zip(state_of(ref), state_of(bad))):
        assert torch.equal(x[:, keep], y[:, keep]), k
    assert (b.out["cmd"][:, [2, 7]] == 0).all()
    for k, (x, y) in enumerate(zip(state_of(bad)[:3], before[:3])):
        assert torch.equal(x[:, [2, 7]], y[:, [2, 7]]), k


# ---- 6. solve mode -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("caller_We", [False, True])
@pytest.mark.parametrize("entry", ["solve", "solve_iterate"])
@pytest.mark.parametrize("form", ["seg", "team_plain"])
def test_solve_mode(built, monkeypatch, form, entry, caller_We):
    """nmpc_batch_solve and _solve_iterate on the packed QP data of the ramp loop's tick 5; a caller's We still wins"""
    model, N, B = "diff", 20, 12
    kept = solve_data()
    xbar, ubar, x0, yref, We_run, P = packed(kept)
    solver = make_solver(monkeypatch, model, N, B, form)
    assert solver.plan_ex(B, "solve")["kernel"] == ("rowpar" if form == "seg" else "team")
    upload(solver, P)
    o = Oracle(model, N, rule="batched")
    We = We_run if caller_We else np.tile(np.array(o.prm.W_e[:o.nx]), (B, 1))
    assert np.abs(We_run - np.array(o.prm.W_e[:o.nx])).max() > 1.0  # (the two cases solve different QPs)
    u0 = torch.zeros(solver.nu, B, device=DEV)
    status = torch.full((B,), -7, dtype=torch.int32, device=DEV)
    We_arg = t(We.T) if caller_We else None
    if entry == "solve":
        solver.state()[0].copy_from(xbar)
        solver.state()[1].copy_from(ubar)
        solver.solve(x0, yref, We=We_arg, u0=u0, status=status)
    else:
        xb, ub = xbar.clone(), ubar.clone()
        solver.solve_iterate(x0, yref, xb, ub, We=We_arg, status=status)
        u0 = ub[:solver.nu]
    torch.cuda.synchronize()
    assert (status == 0).all(), status
    far = 0.0
    for i, ((xb_i, ub_i, x0_i, yref_i, _), box) in enumerate(kept):
        st, _, _, un = sc.solve_spliced(o, xb_i, ub_i, x0_i, yref_i, We[i], box)
        assert st == 0, i
        assert np.abs(u0[:, i].cpu().numpy() - un[0]).max() <= TOL_U, i
        _, _, _, ud = o.sqp_rti(xb_i, ub_i, x0_i, yref_i, We[i])
        far = max(far, np.abs(ud[0] - un[0]).max())
    assert far > 100 * TOL_U  # (the profile matters in these QPs)


# ---- 7. node ticks and path ticks --------------------------------------------------------------------------------------
def node_setup(B, seed=5):
    """the mixed fleet's solver: seeded carried refs, the rule's profile on them, and the oracles"""
    model, N = "diff", NODE_N
    solver = BatchSolver(model, N, B, device=DEV)
    carried = np.random.default_rng(seed).uniform(0.1, 0.5, (B, 1)).repeat(2, axis=1).astype(np.float32)
    solver.state()[2].copy_from(t(carried.T))
    P = sc.profile(model, N, sc.speed_of(model, carried), T0)
    upload(solver, P)
    _, fleet = sc.default_fleet(model, N, B)
    fleet.carried[:] = carried
    return solver, P, fleet


def check_node(tk, f, solver, P, fleet, before, tab):
    B, N = tk.B, NODE_N
    solved = tk.solved()
    assert 0 < solved.sum() < B
    sv, ns = np.flatnonzero(solved), np.flatnonzero(~solved)
    assert torch.equal(table_bytes(solver), tab)
    for k, (x, y) in enumerate(zip(state_of(solver), before)):
        assert torch.equal(x[:, ns], y[:, ns]), k
    for k, a in tk.outs().items():
        assert (a[..., ns] == 0).all(), k
    traj = np.ascontiguousarray(tk.traj.cpu().numpy().transpose(2, 0, 1), np.float64)
    tlen = np.full(B, N + 1, np.int32)
    dflt = sc.StageFleet([Oracle("diff", N, rule="batched") for _ in range(B)], fleet.carried)
    for i in sv:
        if int(f.mode[i]) == nr.GOTO_POSE:
            tlen[i] = 1
        if f.reset[i]:
            fleet.xbar[i], fleet.ubar[i] = 0.0, 0.0
            dflt.xbar[i], dflt.ubar[i] = 0.0, 0.0
    pose, vel = f.pose.astype(np.float64), f.vel.astype(np.float64)
    _, u0_d, _, _ = dflt.tick(pose, vel, None, traj, tlen, only=sv)
    cmd_o, u0_o, st_o, _ = fleet.tick(pose, vel, None, traj, tlen, P=P, only=sv)
    assert (st_o[sv] == 0).all() and (tk.status.cpu().numpy()[sv] == 0).all()
    assert np.abs(tk.u0.cpu().numpy().T[sv] - u0_o[sv]).max() <= TOL_U
    assert np.abs(tk.cmd.cpu().numpy().T[sv] - cmd_o[sv]).max() <= TOL_U
    assert np.abs(u0_d[sv] - u0_o[sv]).max() > 100 * TOL_U  # (the default box gives another answer)


def test_node_tick_uses_the_stage_table(built):
    B = 12
    f, p = mixed_fleet(B), node_params()
    solver, P, fleet = node_setup(B)
    tab, before = table_bytes(solver), state_of(solver)
    tk = Tick(f, "diff")
    tk.run(solver, p)
    check_node(tk, f, solver, P, fleet, before, tab)


def test_node_tick_queue_uses_the_stage_table(built):
    assert qc.N == NODE_N
    f = qc.from_node_fleet(mixed_fleet(12))
    solver, P, fleet = node_setup(f.B)
    tab, before = table_bytes(solver), state_of(solver)
    tk = QTick(f, "diff")
    tk.run(solver, node_params())
    tk.solved = lambda: np.isin(tk.event.cpu().numpy(), (nr.EV_SOLVED, nr.EV_SOLVE_FAILED))
    check_node(tk, f, solver, P, fleet, before, tab)


@pytest.mark.parametrize("entry", ["run_path", "follow_path"])
def test_path_ticks_use_the_stage_table(built, entry):
    """run_path / follow_path against the oracles on the poses the launch reports"""
    model, N, B = "diff", 20, 12
    rng = np.random.default_rng(99)
    segs, nseg, nu = random_paths(B, seed=99, max_segs=4, reverse_frac=0.0)
    nu[:] = 0.0 if entry == "follow_path" else rng.uniform(0, 0.3, B)
    exp, _ = path_discretize(segs, nseg, nu, 1 / 40, N + 1, False)
    pose = exp[:, 0, :].copy()
    pose[:, :2] += rng.uniform(-0.02, 0.02, (B, 2))
    v = rng.uniform(0.2, 0.5, B)
    vel = np.zeros((B, 3))
    vel[:, 0] = v
    pose32, vel32 = pose.astype(np.float32), vel.astype(np.float32)
    carried = np.stack([v, v], axis=1).astype(np.float32)
    solver = BatchSolver(model, N, B, device=DEV)
    solver.state()[2].copy_from(t(carried.T))
    P = sc.profile(model, N, sc.speed_of(model, carried), T0)
    upload(solver, P)
    _, fleet = sc.default_fleet(model, N, B)
    fleet.carried[:] = carried
    traj = torch.zeros(N + 1, 3, B, device=DEV)
    out = dict(cmd=torch.zeros(3, B, device=DEV), u0=torch.zeros(2, B, device=DEV),
               status=torch.full((B,), -7, dtype=torch.int32, device=DEV))
    d64 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float64)).to(DEV)  # noqa: E731
    args = (t(pose32.T), t(vel32.T), d64(segs), t(nseg, torch.int32), d64(nu), 1 / 40)
    getattr(solver, entry)(*args, traj_out=traj, **out)
    torch.cuda.synchronize()
    th = np.ascontiguousarray(traj.cpu().numpy().transpose(2, 0, 1), np.float64)
    dflt = sc.StageFleet([Oracle(model, N, rule="batched") for _ in range(B)], fleet.carried)
    inp = (pose32.astype(np.float64), vel32.astype(np.float64), None, th, np.full(B, N + 1, np.int32))
    _, u0_d, _, _ = dflt.tick(*inp)
    cmd_o, u0_o, st_o, _ = fleet.tick(*inp, P=P)
    assert (st_o == 0).all() and (out["status"] == 0).all(), (st_o, out["status"])
    assert np.abs(out["u0"].cpu().numpy().T - u0_o).max() <= TOL_U
    assert np.abs(out["cmd"].cpu().numpy().T - cmd_o).max() <= TOL_U
    assert np.abs(u0_d - u0_o).max() > 100 * TOL_U


# ---- 8. clear, save and restore --------------------------------------------------------------------------------------
def test_clear_restores_table_off_results(built):
    model, N, B = "diff", 20, 12
    plain, on, cleared = (BatchSolver(model, N, B, device=DEV) for _ in range(3))
    a, b, c = Loop(plain, model, B), Loop(on, model, B), Loop(cleared, model, B)
    P = sc.profile(model, N, cm_of(a), T0)
    for s in (on, cleared):
        upload(s, P)
    cleared.clear_stage_bounds()
    assert cleared.stage_bounds() is None and on.stage_bounds() is not None
    b.run()
    for tick in range(2):
        a.run()
        c.run()
        if tick == 0:
            assert not torch.equal(a.out["u0"], b.out["u0"])  # (with the table on the same fleet gets another answer)
        for k in a.out:
            assert torch.equal(a.out[k], c.out[k]), (tick, k)
        for k, (x, y) in enumerate(zip(state_of(plain), state_of(cleared))):
            assert torch.equal(x, y), (tick, k)
        a.advance()
        c.advance()


@pytest.mark.parametrize("robot_table", [False, True])
def test_save_restore_replays_two_ticks(built, robot_table):
    model, N, B = "diff", 20, 12
    s = BatchSolver(model, N, B, device=DEV)
    if robot_table:
        s.set_robot_params(**table_args(rc.robot_params(model, N, B)))
    loop = Loop(s, model, B)
    loop.run()
    loop.advance()
    cm = cm_of(loop)
    upload(s, sc.profile(model, N, cm, T0))
    saved = s.save_state()
    assert len(saved) == (7 if robot_table else 6) and torch.equal(saved[-1]["stage_bounds"], table_bytes(s))
    world = [x.clone() for x in (loop.pose, loop.vel, loop.prog, loop.traj, loop.tlen)]

    def two_ticks():
        outs = []
        for _ in range(2):
            loop.run()
            outs.append({k: v.clone() for k, v in loop.out.items()})
            s.shift_stage_bounds(1)
            loop.advance()
        return outs, state_of(s), table_bytes(s)

    first, after, tab = two_ticks()
    assert not torch.equal(tab, saved[-1]["stage_bounds"])
    s.clear_stage_bounds()
    s.restore_state(saved)
    assert torch.equal(table_bytes(s), saved[-1]["stage_bounds"])
    for dst, src in zip((loop.pose, loop.vel, loop.prog, loop.traj, loop.tlen), world):
        dst.copy_(src)
    again, after2, tab2 = two_ticks()
    for x, y in zip(first, again):
        for k in x:
            assert torch.equal(x[k], y[k]), k
    for k, (x, y) in enumerate(zip(after, after2)):
        assert torch.equal(x, y), k
    assert torch.equal(tab, tab2)
    # a checkpoint taken with the stage table off turns it off again
    s.restore_state(saved[:-1])
    assert s.stage_bounds() is None and (s.robot_params() is not None) == robot_table
