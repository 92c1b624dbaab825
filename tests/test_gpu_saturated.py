"""GPU tests of both solve kernels on saturated QPs (tests/saturated_cases.py) against one fp64 solve per robot on the
same QP with the same per-stage box (tests/stage_bound_cases.py: solve_spliced / StageFleet, oracle rule "batched").

Every oracle comparison elsewhere in the suite runs in a closed loop whose plant moves: a bound is active at a few
stages for a few ticks and the iterate is never exactly on one. Here the plant stands still under a speed limit that
starts on the robot's own carried speed (family A), the iterate sits exactly on its bounds, or one fp32 ulp to either
side (family B), and every input is on its bound over the whole horizon as well (family C).

Tolerance: test_gpu_parity.py's, every status 0, |u0 - u0_ref|_inf and |cmd - cmd_ref|_inf <= 1e-3, qp_iter < 50; in
solve mode the predicted states within 1e-3 as well. No robot is left out beyond the case table's own list.
"""
import numpy as np
import pytest
import torch

from oracle.oracle import Oracle
from tests import saturated_cases as sat
from tests import stage_bound_cases as sc
from tests.table_harness import CASES, FORMS, TOL_U, Loop, check_tick, make_solver, t

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
B, T = sat.B, sat.T
SOLVE_FORMS = ["seg", "serial", "team_split_launch", "team_plain"]
SOLVE = [("diff", 20), ("omni4", 20), ("tric", 20), ("diff", 40)]


def upload(solver, P):
    """a profile dict [B][stages][n] into the solver's stage table ([stages][n][B] on the device)"""
    solver.set_stage_bounds(**{k: t(P[k].transpose(1, 2, 0)) for k in sc.FIELDS})


# ---- family A: the static-plant loop -----------------------------------------------------------------------------------
def static_loop(monkeypatch, model, form, N):
    solver = make_solver(monkeypatch, model, N, B, form)
    plan = solver.plan_ex(B, "run")
    assert FORMS[form][2](plan), plan
    loop = Loop(solver, model, B)
    _, fleet = sc.default_fleet(model, N, B)
    inp = loop.host_inputs()  # tick 0's measurements and reference lists, at every tick: the plant is never advanced
    eu, ec, its = 0.0, 0.0, 0
    for tick in range(T):
        P = sat.zone_profile(model, N, loop.carried().cpu().numpy().T)  # c from the device's carried refs
        upload(solver, P)
        loop.run()
        a, b = check_tick(loop, fleet, inp, tick, P=P)
        it = int(loop.out["qp_iter"].max())
        assert it < sat.QP_ITER_MAX, (tick, it)
        eu, ec, its = max(eu, a), max(ec, b), max(its, it)
    held = sat.on_limit(model, fleet.xbar, P)
    print(f"{model} {form} N={N}: |du0| {eu:.2e} |dcmd| {ec:.2e} qp_iter <= {its}; stages on the limit "
          f"{held.tolist()}")
    assert sum(1 for i in range(B) if sat.limited(i) and held[i] > N / 4) >= 3  # (the loop is the saturated one)


@pytest.mark.parametrize("model,form", CASES)
def test_static_loop(built, monkeypatch, model, form):
    static_loop(monkeypatch, model, form, 20)


@pytest.mark.parametrize("form", ["seg", "team_plain"])
def test_static_loop_N40(built, monkeypatch, form):
    static_loop(monkeypatch, "diff", form, 40)


@pytest.mark.parametrize("N", [21, 22])
def test_static_loop_rotation_remainders(built, monkeypatch, N):
    """N + 1 = 22 and 23: with N = 20 the team kernel's three-row rotation of P0 ends on each of its remainders"""
    static_loop(monkeypatch, "diff", "team_plain", N)


# ---- families B and C: the iterate exactly on its bounds, solve mode ---------------------------------------------------
def pad(a, cap):
    out = torch.zeros(a.shape[0], cap, device=DEV)
    out[:, :a.shape[1]] = a
    return out


def solve_case(solver, c, ref):
    """the case cold, then the same data once more on the warm handle; both against the reference"""
    n, N, nx, nu = len(c.keep), c.N, solver.nx, solver.nu
    cap = solver.state()[0].shape[1]
    xbar, ubar = t(c.xbar.reshape(n, -1).T), t(c.ubar.reshape(n, -1).T)
    x0, yref, We = t(c.x0.T), t(c.yref.transpose(1, 2, 0)), t(c.We.T)
    upload(solver, c.P)
    solver.forget_warm()
    worst = [0.0, 0.0, 0]
    for warm in (False, True):
        solver.state()[0].copy_from(pad(xbar, cap))
        solver.state()[1].copy_from(pad(ubar, cap))
        o = dict(u0=torch.zeros(nu, n, device=DEV), xtraj=torch.zeros((N + 1) * nx, n, device=DEV),
                 status=torch.full((n,), -7, dtype=torch.int32, device=DEV),
                 qp_iter=torch.zeros(n, dtype=torch.int32, device=DEV), qp_res=torch.zeros(3, n, device=DEV))
        solver.solve(x0, yref, We=We, **o)
        torch.cuda.synchronize()
        st, it = o["status"].cpu().numpy(), o["qp_iter"].cpu().numpy()
        eu = np.abs(o["u0"].cpu().numpy().T - ref["u0"]).max()
        ex = np.abs(o["xtraj"].cpu().numpy().T.reshape(n, N + 1, nx) - ref["xbar"]).max()
        print(f"{c.model} N={N} {c.name} {'warm' if warm else 'cold'}: status {st.tolist()} iters {it.tolist()} "
              f"(reference <= {ref['iters'].max()}); |du0| {eu:.2e} |dx| {ex:.2e}")
        assert (st == 0).all(), (c.name, warm, st)
        assert it.max() < sat.QP_ITER_MAX, (c.name, warm, it)
        assert eu <= TOL_U, (c.name, warm, eu)
        assert ex <= TOL_U, (c.name, warm, ex)
        worst = [max(worst[0], eu), max(worst[1], ex), max(worst[2], int(it.max()))]
    return worst


_REF = {}


def reference(model, N):
    """the fp64 reference of every case of (model, N), once for all forms"""
    if (model, N) not in _REF:
        o = Oracle(model, N, rule="batched")
        out = []
        for c in sat.solve_cases(model, N):
            r = [sc.solve_spliced(o, c.xbar[i], c.ubar[i], c.x0[i], c.yref[i], c.We[i], c.box(i))
                 for i in range(len(c.keep))]
            assert all(s == 0 for s, *_ in r), c.name
            out.append(dict(iters=np.array([q for _, q, _, _ in r]), xbar=np.stack([xb for *_, xb, _ in r]),
                            u0=np.stack([ub[0] for *_, ub in r])))
        _REF[(model, N)] = out
    return _REF[(model, N)]


@pytest.mark.parametrize("form", SOLVE_FORMS)
@pytest.mark.parametrize("model,N", SOLVE)
def test_solve_cases(built, monkeypatch, model, N, form):
    """family B (K = 1, N/2 - 3, N; the bound exactly on the iterate, one ulp above, one ulp below) and family C (every
    input on its bound as well), each cold and once more warm"""
    cases, refs = sat.solve_cases(model, N), reference(model, N)
    worst = [0.0, 0.0, 0]
    for c, ref in zip(cases, refs):
        solver = make_solver(monkeypatch, model, N, len(c.keep), form)
        plan = solver.plan_ex(len(c.keep), "solve")
        assert FORMS[form][2](plan), plan
        w = solve_case(solver, c, ref)
        worst = [max(a, b) for a, b in zip(worst, w)]
    print(f"{model} N={N} {form}: |du0| {worst[0]:.2e} |dx| {worst[1]:.2e} qp_iter <= {worst[2]}")


# ---- the recorded failure ----------------------------------------------------------------------------------------------
# (form, robots). The recording was made by a launch of 1024 robots: above 256 robots the row-parallel kernel runs two
# waves per robot with 4 segments at N = 40, up to 256 four waves with 5 segments, which is another instruction stream.
# "seg" is therefore the smallest batch that takes the recording's plan; "seg_small" is the small-batch plan.
RECORDED = {"seg": ("seg", 257), "seg_small": ("seg", 5), "serial": ("serial", 5), "team_plain": ("team_plain", 5)}


@pytest.mark.parametrize("case", list(RECORDED))
def test_recorded_case(built, monkeypatch, case):
    """The stored tick sequence of the robot that failed under the seeded speed map (tests/golden/
    make_saturated_fixture.md), replayed from a cold handle with run(): every slot of the batch holds the robot, so it
    leads a wave and trails one, and the replay rebuilds the warm multipliers in the form's own record layout. Each
    tick's stored limits are uploaded with set_stage_limits first. Every tick, the recorded failing one included, has
    status 0 and u0 and cmd within 1e-3 of the StageFleet chain on the same limits. In the plan that made the recording
    ("seg": rowpar, 4 segments, two waves per robot) the carried refs before every tick, the iteration counts and u0
    of the ticks before the failing one are the stored ones bit for bit: the replay is the recorded run. Before the
    fix that case ended tick 32 with status 1 at iteration 21 and qp_res (0, 0, NaN), as the recording did; the other
    three solved it. Measured with the fix: |u0 - ref| 7.3e-4 at tick 32 in "seg" (the master's guard ends the solve at
    iteration 20), 2.1e-4 in "seg_small", 1.2e-5 in "serial" and "team_plain"."""
    form, n = RECORDED[case]
    d = sat.recorded()
    model, N, tk = "diff", d["N"], d["tick"]
    solver = make_solver(monkeypatch, model, N, n, form)
    plan = solver.plan_ex(n, "run")
    assert FORMS[form][2](plan), plan
    if case == "seg":
        assert (plan["segments"], plan["waves_per_robot"]) == (4, 2), plan
    fleet = sc.StageFleet([Oracle(model, N, rule="batched")], np.zeros((1, solver.nbx)))  # (one robot: every slot's)
    one = lambda a: np.asarray(a, np.float64)[None]                                        # noqa: E731
    rep = lambda a: np.repeat(np.asarray(a, np.float32)[..., None], n, axis=-1)           # noqa: E731
    out = dict(cmd=torch.zeros(3, n, device=DEV), u0=torch.zeros(solver.nu, n, device=DEV),
               status=torch.zeros(n, dtype=torch.int32, device=DEV),
               qp_iter=torch.zeros(n, dtype=torch.int32, device=DEV), qp_res=torch.zeros(3, n, device=DEV))
    tlen = np.ones(1, np.int32)  # GOTO_POSE: the goal alone, padded by the solve
    eu = ec = 0.0
    its = []
    for tick in range(tk + 1):
        solver.set_stage_limits(v_max=t(rep(d["vlim"][tick])))
        if d["reset"][tick]:
            fleet.xbar[:], fleet.ubar[:] = 0.0, 0.0
        before = solver.state()[2].to_tensor()[:, :n].cpu().numpy()
        solver.run(t(rep(d["pose"][tick])), t(rep(d["vel"][tick])), t(rep(d["traj"][tick])),
                   traj_len=t(np.ones(n, np.int32), torch.int32),
                   reset=t(np.full(n, d["reset"][tick], np.uint8), torch.uint8), **out)
        torch.cuda.synchronize()
        cmd_o, u0_o, st_o, it_o = fleet.tick(one(d["pose"][tick]), one(d["vel"][tick]), None, one(d["traj"][tick]), tlen,
                                             P=sat.limits_profile(model, N, one(d["vlim"][tick])))
        st, it = out["status"].cpu().numpy(), out["qp_iter"].cpu().numpy()
        u0 = out["u0"].cpu().numpy()
        a = np.abs(u0.T - u0_o).max()
        b = np.abs(out["cmd"].cpu().numpy().T - cmd_o).max()
        print(f"tick {tick}: reference status {st_o.tolist()} iters {it_o.tolist()}; device status {np.unique(st).tolist()} "
              f"iters {np.unique(it).tolist()} (recorded {d['status'][tick]}, {d['qp_iter'][tick]}) qp_res "
              f"{out['qp_res'][:, 0].cpu().numpy().tolist()}; |du0| {a:.2e} |dcmd| {b:.2e}")
        if case == "seg":
            assert np.array_equal(before, rep(d["carried"][tick])), tick
            if tick < tk:
                assert (it == d["qp_iter"][tick]).all() and np.array_equal(u0, rep(d["u0"][tick])), tick
        assert (st_o == 0).all(), (tick, st_o)
        assert (st == 0).all(), (tick, np.unique(st), np.unique(it))
        assert it.max() < sat.QP_ITER_MAX
        assert a <= TOL_U and b <= TOL_U, (tick, a, b)
        eu, ec = max(eu, a), max(ec, b)
        its.append(int(it.max()))
    print(f"recorded case, {case}: |du0| {eu:.2e} |dcmd| {ec:.2e} qp_iter <= {max(its)}, at the recorded tick {its[-1]}")
