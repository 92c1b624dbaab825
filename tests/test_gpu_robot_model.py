"""GPU tests of the model table (csrc/robot_tables.hip, robot_vals in csrc/sqp_steps.hpp, the team kernel's MT
instantiations) against one fp64 Oracle per robot (tests/robot_model_cases.py).

Tolerance of the oracle comparisons: test_gpu_parity.py's, |u0 - u0_oracle|_inf and |cmd - cmd_oracle|_inf <= 1e-3 with
every status 0. On the CPU (tests/test_robot_model_ref.py) putting any one parameter of the rule back to the handle's
value moves some robot's u0 by 6e-2 to 1.0 on every tick from tick 1 (diff, omni4: from tick 0), so a library that
ignores the table, or any one row of it, cannot pass. Nine robots are two full waves plus a one-team wave of the team
kernel, and each full wave holds four different p.

The team kernel's table-on launches take the sparse per-team form of the M block (m_block_team, csrc/team_common.hpp),
whose sums come in the column form's order: a table holding the handle's own p is bit-identical to table off in both
kernels (test_own_values_run).
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from nmpc_nav_control_amd.batch import BatchSolver
from nmpc_nav_control_amd.scenario import make_fleet
from oracle.oracle import path_discretize
from tests import node_ref as nr
from tests import robot_model_cases as mc
from tests import robot_param_cases as rc
from tests import stage_bound_cases as sc
from tests.path_cases import random_paths
from tests.test_gpu_node import N as NODE_N
from tests.test_gpu_node import Tick, mixed_fleet
from tests.test_gpu_node import params as node_params
from tests.table_harness import CASES, FORMS, MODELS, TOL_U, Loop, check_tick, make_solver, state_of, t, table_args

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
N, B = 20, 9
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def upload(solver, Pm, mask=None):
    """a parameter array [B][np] into the solver's model table ([np][B] on the device)"""
    solver.set_robot_model(t(Pm.T), mask=mask)


class FleetLoop(Loop):
    """Loop on a given fleet dict (make_fleet's fields, [field][B]) instead of the seeded fleet's first B robots"""

    def __init__(self, solver, model, fl):
        self.s, self.model, self.B = solver, model, fl["pose"].shape[1]
        Bn, Nn = self.B, solver.N
        self.fl = fl
        cr = torch.zeros(fl["carried"].shape[0], solver.capacity, device=DEV)
        cr[:, :Bn] = t(fl["carried"])
        solver.state()[2].copy_from(cr)
        self.pose, self.vel, self.steer = t(fl["pose"]), t(fl["vel"]), t(fl["steer"])
        self.path, self.prog = t(fl["path"]), t(fl["s"])
        self.steer_arg = self.steer if model == "tric" else None
        self.traj = torch.zeros(Nn + 1, 3, Bn, device=DEV)
        self.tlen = torch.zeros(Bn, dtype=torch.int32, device=DEV)
        self.out = dict(cmd=torch.zeros(3, Bn, device=DEV), u0=torch.zeros(solver.nu, Bn, device=DEV),
                        status=torch.zeros(Bn, dtype=torch.int32, device=DEV),
                        qp_iter=torch.zeros(Bn, dtype=torch.int32, device=DEV), qp_res=torch.zeros(3, Bn, device=DEV))
        solver.fleet_sim_step(self.path, self.prog, self.pose, self.vel, self.steer_arg, None, None, self.traj,
                              self.tlen, advance=False)


# ---- 1. closed-loop parity in every launch form ----------------------------------------------------------------------
@pytest.mark.parametrize("model,form", CASES)
def test_closed_loop_matches_per_robot_oracles(built, monkeypatch, model, form):
    T = 6
    solver = make_solver(monkeypatch, model, N, B, form)
    plan = solver.plan_ex(B, "run")
    assert FORMS[form][2](plan), plan
    Pm = mc.robot_model(model, N, B)
    assert solver.robot_model() is None  # (the table is off until the first writer)
    upload(solver, Pm)
    torch.cuda.synchronize()
    assert np.array_equal(solver.robot_model().to_tensor().cpu().numpy()[:, :B], Pm.T.astype(np.float32))
    loop = Loop(solver, model, B)
    fleet = rc.OracleFleet(mc.oracles(model, N, Pm), loop.fl["carried"].T)
    for tick in range(T):
        inp = loop.host_inputs()
        loop.run()
        check_tick(loop, fleet, inp, tick)
        loop.advance()


# ---- 2. wave-mates: one robot's state in the four teams of one wave, four different p --------------------------------
@pytest.mark.parametrize("model", MODELS)
def test_wave_mates_get_their_own_constant_rows(built, monkeypatch, model):
    """Constant rows of [B A] taken from the wave's first team would give the other three teams a wrong Newton system:
    on the CPU the four solutions differ pairwise by at least 0.15 (diff), 0.11 (omni4), 0.09 (tric) in u0 on ticks 1
    to 3 (tests/test_robot_model_ref.py asserts >= 15e-3)."""
    r = mc.WAVE_ROBOT[model]
    solver = make_solver(monkeypatch, model, N, 4, "team_plain")
    assert FORMS["team_plain"][2](solver.plan_ex(4, "run"))
    Pm = mc.robot_model(model, N, 4)
    upload(solver, Pm)
    full = make_fleet(model, r + 1, seed=mc.SEED)
    fl = {k: np.ascontiguousarray(np.repeat(v[..., r:r + 1], 4, axis=-1)) for k, v in full.items()}
    loop = FleetLoop(solver, model, fl)
    fleet = rc.OracleFleet(mc.oracles(model, N, Pm), fl["carried"].T)
    for tick in range(4):
        inp = loop.host_inputs()
        loop.run()
        check_tick(loop, fleet, inp, tick)
        if tick >= 1:
            u = loop.out["u0"].cpu().numpy().T
            assert min(np.abs(u[a] - u[b]).max() for a in range(4) for b in range(a + 1, 4)) >= 15 * TOL_U
        loop.advance()


# ---- 3. the product against the row-form checker build ---------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
def test_product_matches_the_row_form_checker(built, tmp_path, model):
    """the nine-robot table through the product library (the sparse per-team M block) and through lib/mrow (the team
    kernel with the row form of the M block for every launch), one child process each. u0 within
    test_gpu_split.py::test_constant_rows_per_launch's bound for the same comparison (3e-4)."""
    mrow = os.path.join(ROOT, "nmpc_nav_control_amd", "lib", "mrow", "libnmpc_amd.so")
    assert os.path.exists(mrow), "lib/mrow/libnmpc_amd.so is built by the csrc Makefile (all)"
    outs = {}
    for name, lib in (("product", None), ("mrow", mrow)):
        env = dict(os.environ)
        env.pop("NMPC_AMD_LIB", None)
        if lib:
            env["NMPC_AMD_LIB"] = lib
        out = str(tmp_path / f"{name}.npz")
        res = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "robot_model_probe.py"), model, str(N), str(B),
                              "3", out], env=env, capture_output=True, text=True, timeout=300)
        assert res.returncode == 0, res.stderr[-3000:]
        outs[name] = np.load(out)
    a, b = outs["product"], outs["mrow"]
    assert str(b["lib"]).endswith("mrow/libnmpc_amd.so") and str(a["lib"]) == ""
    assert (a["status"] == 0).all() and np.array_equal(a["status"], b["status"])
    di = int(np.abs(a["qp_iter"] - b["qp_iter"]).max())
    du = float(np.abs(a["u0"] - b["u0"]).max())
    print(f"{model}: product vs row-form checker: |du0| {du:.2e}, IPM counts differ by at most {di}")
    assert di <= 3
    assert du <= 3e-4


# ---- 4. a table holding the handle's own p ---------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["seg", "team_plain"])
@pytest.mark.parametrize("model", MODELS)
def test_own_values_run(built, monkeypatch, model, form):
    """outputs, iterate, carried refs and warm flags bit for bit over three ticks, in both kernels"""
    off, on = (make_solver(monkeypatch, model, N, B, form) for _ in range(2))
    upload(on, mc.handle_model(model, N, B))
    assert off.robot_model() is None and on.robot_model() is not None
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
        for x, y in ((a.pose, b.pose), (a.vel, b.vel)):  # (and the plant steps the same vehicle)
            assert torch.equal(x, y), tick
    assert (a.out["status"] == 0).all()


# ---- 5. placement: p follows the robot, not the team slot -------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
def test_placement_changes_nothing(built, monkeypatch, model):
    for k, v in FORMS["team_plain"][0].items():
        monkeypatch.setenv(k, v)
    Pm = mc.robot_model(model, N, B)
    res = []
    for sched in ("off", "sorted"):
        s = BatchSolver(model, N, B, device=DEV)
        s.set_schedule(sched)
        upload(s, Pm)
        loop = Loop(s, model, B)
        for _ in range(3):  # two ticks leave iter_key behind; the third is compared
            loop.run()
            loop.advance()
        res.append({k: v.clone() for k, v in loop.out.items()})
    a, b = res
    assert len(set(a["qp_iter"].cpu().numpy().tolist())) > 1  # (the sorted order is not the index order)
    assert torch.equal(a["status"], b["status"]) and (a["status"] == 0).all()
    assert float((a["u0"] - b["u0"]).abs().max()) <= 1e-6


# ---- 6. a change between ticks ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["seg", "team_plain"])
@pytest.mark.parametrize("model", MODELS)
def test_masked_write_between_ticks(built, monkeypatch, model, form):
    """after tick 2 robots 1, 4 and 7 get their left neighbour's column: from tick 3 they match oracles changed in step
    and leave the unchanged run; the other six stay bit-identical to it, and no warm flag moves with the write"""
    ch, ref = (make_solver(monkeypatch, model, N, B, form) for _ in range(2))
    Pm = mc.robot_model(model, N, B)
    for s in (ch, ref):
        upload(s, Pm)
    a, b = Loop(ch, model, B), Loop(ref, model, B)
    fleet = rc.OracleFleet(mc.oracles(model, N, Pm), a.fl["carried"].T)
    who = [1, 4, 7]
    rest = torch.tensor([i for i in range(B) if i not in who], device=DEV)
    mask = torch.zeros(B, dtype=torch.uint8, device=DEV)
    mask[who] = 1
    for tick in range(5):
        if tick == 3:
            P2 = np.roll(Pm, 1, axis=0)
            assert all((P2[i] != Pm[i]).any() for i in who)
            warm = state_of(ch)[3]
            upload(ch, P2, mask=mask)
            torch.cuda.synchronize()
            want = Pm.copy()
            want[who] = P2[who]
            assert np.array_equal(ch.robot_model().to_tensor().cpu().numpy()[:, :B], want.T.astype(np.float32))
            assert torch.equal(state_of(ch)[3], warm)
            for i in who:
                mc.set_p(fleet.os[i], P2[i])
        inp = a.host_inputs()
        a.run()
        b.run()
        check_tick(a, fleet, inp, tick)
        for k in a.out:
            assert torch.equal(a.out[k][..., rest], b.out[k][..., rest]), (tick, k)
        for k, (x, y) in enumerate(zip(state_of(ch), state_of(ref))):
            assert torch.equal(x[:, rest], y[:, rest]), (tick, k)
        same = torch.equal(a.out["u0"][:, who], b.out["u0"][:, who])
        assert same == (tick < 3), tick
        a.advance()
        b.advance()


# ---- 7. a bad parameter fails its robot alone -------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["seg", "team_plain"])
@pytest.mark.parametrize("model", MODELS)
def test_nan_and_zero_fail_alone(built, monkeypatch, model, form):
    """a NaN in p[1] of robot 3 and a zero in p[0] of robot 5: status 1 and a stop command on those two, which keep
    their iterate and carried refs; every other robot is bit-identical to the run without them"""
    bad, ref = (make_solver(monkeypatch, model, N, B, form) for _ in range(2))
    Pm = mc.robot_model(model, N, B)
    for s in (bad, ref):
        upload(s, Pm)
    a, b = Loop(bad, model, B), Loop(ref, model, B)
    for loop in (a, b):
        loop.run()
        loop.advance()
    P2 = Pm.copy()
    P2[3, 1] = np.nan
    P2[5, 0] = 0.0
    upload(bad, P2)
    torch.cuda.synchronize()
    before = state_of(bad)
    a.run()
    b.run()
    st = a.out["status"].cpu().numpy()
    print(f"{model} {form}: status {st.tolist()}")
    assert st[3] == 1 and st[5] == 1, st
    keep = torch.tensor([i for i in range(B) if i not in (3, 5)], device=DEV)
    assert (st[keep.cpu().numpy()] == 0).all() and (b.out["status"] == 0).all()
    assert (a.out["cmd"][:, [3, 5]] == 0).all()
    for k, (x, y) in enumerate(zip(state_of(bad)[:3], before[:3])):
        assert torch.equal(x[:, [3, 5]], y[:, [3, 5]]), k
    for k in a.out:
        assert torch.equal(a.out[k][..., keep], b.out[k][..., keep]), k
    for k, (x, y) in enumerate(zip(state_of(bad), state_of(ref))):
        assert torch.equal(x[:, keep], y[:, keep]), k


# ---- 8. every entry point ---------------------------------------------------------------------------------------------
def test_node_tick_uses_the_table(built):
    """test_gpu_node.py's mixed-mode fleet: the robots that solve match their own oracle on the references the gate
    made; the others' state, and the table, are untouched"""
    model, Nn, Bn = "diff", NODE_N, 12
    f, p = mixed_fleet(Bn), node_params()
    solver = BatchSolver(model, Nn, Bn, device=DEV)
    Pm = mc.robot_model(model, Nn, Bn)
    upload(solver, Pm)
    torch.cuda.synchronize()
    tab = solver.robot_model().to_tensor()
    before = state_of(solver)
    fleet = rc.OracleFleet(mc.oracles(model, Nn, Pm), np.zeros((Bn, 2)))
    tk = Tick(f, model)
    tk.run(solver, p)
    solved = tk.solved()
    assert 0 < solved.sum() < Bn
    sv, ns = np.flatnonzero(solved), np.flatnonzero(~solved)
    assert torch.equal(solver.robot_model().to_tensor(), tab)
    for k, (x, y) in enumerate(zip(state_of(solver), before)):
        assert torch.equal(x[:, ns], y[:, ns]), k
    traj = np.ascontiguousarray(tk.traj.cpu().numpy().transpose(2, 0, 1), np.float64)
    tlen = np.full(Bn, Nn + 1, np.int32)
    for i in sv:
        if int(f.mode[i]) == nr.GOTO_POSE:
            tlen[i] = 1
        if f.reset[i]:
            fleet.xbar[i], fleet.ubar[i] = 0.0, 0.0
    cmd_o, u0_o, st_o, _ = fleet.tick(f.pose.astype(np.float64), f.vel.astype(np.float64), None, traj, tlen, only=sv)
    assert (st_o[sv] == 0).all() and (tk.status.cpu().numpy()[sv] == 0).all()
    assert np.abs(tk.u0.cpu().numpy().T[sv] - u0_o[sv]).max() <= TOL_U
    assert np.abs(tk.cmd.cpu().numpy().T[sv] - cmd_o[sv]).max() <= TOL_U
    # and the table matters here: the handle's p gives another answer
    dflt = rc.OracleFleet(mc.oracles(model, Nn, mc.handle_model(model, Nn, Bn)), np.zeros((Bn, 2)))
    for i in sv:
        if f.reset[i]:
            dflt.xbar[i], dflt.ubar[i] = 0.0, 0.0
    _, u0_d, _, _ = dflt.tick(f.pose.astype(np.float64), f.vel.astype(np.float64), None, traj, tlen, only=sv)
    assert np.abs(u0_d[sv] - u0_o[sv]).max() > 15 * TOL_U


def test_follow_path_uses_the_table(built):
    """one follow_path tick against the oracles on the poses the launch reports"""
    model, Bn = "diff", B
    rng = np.random.default_rng(99)
    segs, nseg, nu = random_paths(Bn, seed=99, max_segs=4, reverse_frac=0.0)
    nu[:] = 0.0
    exp, _ = path_discretize(segs, nseg, nu, 1 / 40, N + 1, False)
    pose = exp[:, 0, :].copy()
    pose[:, :2] += rng.uniform(-0.02, 0.02, (Bn, 2))
    v = rng.uniform(0.2, 0.5, Bn)
    vel = np.zeros((Bn, 3))
    vel[:, 0] = v
    vel[:, 2] = rng.uniform(-0.5, 0.5, Bn)  # (a yaw rate: direct kinematics then read b)
    pose32, vel32 = pose.astype(np.float32), vel.astype(np.float32)
    carried = np.stack([v, v], axis=1).astype(np.float32)
    solver = BatchSolver(model, N, Bn, device=DEV)
    solver.state()[2].copy_from(t(carried.T))
    Pm = mc.robot_model(model, N, Bn)
    upload(solver, Pm)
    traj = torch.zeros(N + 1, 3, Bn, device=DEV)
    out = dict(cmd=torch.zeros(3, Bn, device=DEV), u0=torch.zeros(2, Bn, device=DEV),
               status=torch.full((Bn,), -7, dtype=torch.int32, device=DEV))
    d64 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float64)).to(DEV)  # noqa: E731
    solver.follow_path(t(pose32.T), t(vel32.T), d64(segs), t(nseg, torch.int32), d64(nu), 1 / 40, traj_out=traj, **out)
    torch.cuda.synchronize()
    th = np.ascontiguousarray(traj.cpu().numpy().transpose(2, 0, 1), np.float64)
    inp = (pose32.astype(np.float64), vel32.astype(np.float64), None, th, np.full(Bn, N + 1, np.int32))
    fleet = rc.OracleFleet(mc.oracles(model, N, Pm), carried)
    dflt = rc.OracleFleet(mc.oracles(model, N, mc.handle_model(model, N, Bn)), carried)
    _, u0_d, _, _ = dflt.tick(*inp)
    cmd_o, u0_o, st_o, _ = fleet.tick(*inp)
    assert (st_o == 0).all() and (out["status"] == 0).all(), (st_o, out["status"])
    assert np.abs(out["u0"].cpu().numpy().T - u0_o).max() <= TOL_U
    assert np.abs(out["cmd"].cpu().numpy().T - cmd_o).max() <= TOL_U
    assert np.abs(u0_d - u0_o).max() > 15 * TOL_U


@pytest.mark.parametrize("form", ["seg", "team_plain"])
def test_solve_iterate_uses_the_table(built, monkeypatch, form):
    """one solve_iterate call on a caller-held iterate: the rule's closed loop on the CPU up to tick 2, that tick's
    inputs on the device"""
    model = "diff"
    Pm = mc.robot_model(model, N, B)
    os_ = mc.oracles(model, N, Pm)
    kept = {}

    def hook(tick, i, pose, vel, steer, traj, carried, xbar, ubar):
        if tick == 2:
            kept[i] = os_[i].prepare(pose, vel, steer, traj, carried) + (xbar, ubar)

    mc.cpu_closed_loop(model, N, B, 3, Pm, hook=hook)
    rec = [kept[i] for i in range(B)]
    solver = make_solver(monkeypatch, model, N, B, form)
    assert solver.plan_ex(B, "solve")["kernel"] == ("rowpar" if form == "seg" else "team")
    upload(solver, Pm)
    xbar = t(np.stack([r[3] for r in rec]).reshape(B, -1).T)
    ubar = t(np.stack([r[4] for r in rec]).reshape(B, -1).T)
    status = torch.full((B,), -7, dtype=torch.int32, device=DEV)
    solver.solve_iterate(t(np.stack([r[0] for r in rec]).T), t(np.stack([r[1] for r in rec]).transpose(1, 2, 0)), xbar,
                         ubar, We=t(np.stack([r[2] for r in rec]).T), status=status)
    torch.cuda.synchronize()
    assert (status == 0).all(), status
    dflt = mc.oracle_for(model, N, mc.handle_model(model, N, 1)[0])
    moved = 0.0
    for i, (o, r) in enumerate(zip(os_, rec)):
        st, _, _, ub = o.sqp_rti(r[3], r[4], r[0], r[1], r[2])
        assert st == 0
        assert np.abs(ubar[:solver.nu, i].cpu().numpy() - ub[0]).max() <= TOL_U, i
        _, _, _, ud = dflt.sqp_rti(r[3], r[4], r[0], r[1], r[2])
        moved = max(moved, np.abs(ud[0] - ub[0]).max())
    assert moved > 15 * TOL_U


# ---- 9. clear, save and restore --------------------------------------------------------------------------------------
def test_clear_restores_table_off_results(built):
    model = "diff"
    plain, on, cleared = (BatchSolver(model, N, B, device=DEV) for _ in range(3))
    for s in (on, cleared):
        upload(s, mc.robot_model(model, N, B))
    cleared.clear_robot_model()
    assert cleared.robot_model() is None and on.robot_model() is not None
    a, b, c = Loop(plain, model, B), Loop(on, model, B), Loop(cleared, model, B)
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
        for x, y in ((a.pose, c.pose), (a.vel, c.vel)):  # (the plant is the handle's vehicle again)
            assert torch.equal(x, y), tick


def test_save_restore_replays_a_tick(built):
    model = "diff"
    s = BatchSolver(model, N, B, device=DEV)
    assert len(s.save_state()) == 5  # table off: the checkpoint is what it was
    Pm = mc.robot_model(model, N, B)
    upload(s, Pm)
    loop = Loop(s, model, B)
    for _ in range(2):
        loop.run()
        loop.advance()
    torch.cuda.synchronize()
    saved = s.save_state()
    assert len(saved) == 6 and torch.equal(saved[5]["robot_model"], s.robot_model().to_tensor())
    loop.run()
    first = {k: v.clone() for k, v in loop.out.items()}
    after = state_of(s)
    # another table, another tick, then back
    upload(s, np.roll(Pm, 2, axis=0))
    loop.run()
    assert not torch.equal(loop.out["u0"], first["u0"])
    s.restore_state(saved)
    assert torch.equal(s.robot_model().to_tensor(), saved[5]["robot_model"])
    loop.run()
    for k in first:
        assert torch.equal(loop.out[k], first[k]), k
    for k, (x, y) in enumerate(zip(state_of(s), after)):
        assert torch.equal(x, y), k
    # a checkpoint taken with the table off turns it off again
    s.restore_state(saved[:5])
    assert s.robot_model() is None


# ---- 10. all three tables on at once ---------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["seg", "team_plain"])
@pytest.mark.parametrize("model", MODELS)
def test_all_three_tables(built, monkeypatch, model, form):
    """W and W_e from the per-robot table's rule, the box from the stage table's ramp (shifted one stage per tick), p
    from this rule; the reference holds all three. Tolerance: test_gpu_stage_bounds.py's (1e-3)."""
    solver = make_solver(monkeypatch, model, N, B, form)
    R, Pm = rc.robot_params(model, N, B), mc.robot_model(model, N, B)
    solver.set_robot_params(**table_args(R))
    upload(solver, Pm)
    loop = Loop(solver, model, B)
    cm = sc.speed_of(model, loop.carried().cpu().numpy().T)
    P = sc.profile(model, N, cm, sc.T0)
    solver.set_stage_bounds(**{k: t(P[k].transpose(1, 2, 0)) for k in sc.FIELDS})
    assert all(v is not None for v in (solver.robot_params(), solver.stage_bounds(), solver.robot_model()))
    os_ = [rc.oracle_for(model, N, R, i, p=[float(v) for v in Pm[i]]) for i in range(B)]
    fleet = sc.StageFleet(os_, loop.fl["carried"].T)
    for tick in range(3):
        if tick:
            solver.shift_stage_bounds(1, B=B)
            P = sc.shifted(P, 1)
        inp = loop.host_inputs()
        loop.run()
        cmd_o, u0_o, st_o, it_o = fleet.tick(*inp, P=P)
        st = loop.out["status"].cpu().numpy()
        eu = np.abs(loop.out["u0"].cpu().numpy().T - u0_o).max()
        ec = np.abs(loop.out["cmd"].cpu().numpy().T - cmd_o).max()
        print(f"tick {tick}: oracle status {st_o.tolist()} iters <= {it_o.max()}; device status {st.tolist()}; "
              f"|du0| {eu:.2e} |dcmd| {ec:.2e}")
        assert (st_o == 0).all() and (st == 0).all(), (tick, st_o, st)
        assert eu <= TOL_U and ec <= TOL_U, (tick, eu, ec)
        loop.advance()
