"""The solve kernels far from the map origin against the fp64 oracle (-m gpu).

Both kernels carry x and y as absolute fp32 values from the input to the stored iterate, and every other fleet of the
suite sits within two metres of (0, 0). Here the fleet of tests/table_harness.py and the edge table of
tests/run_edge_cases.py are moved by tests/far_field_cases.py's OFFSETS (shown to be a valid instrument by
tests/test_far_field_cases.py) and go through run mode and solve mode in the launch forms of table_harness.FORMS.
The reference everywhere is the fp64 oracle on the same fp32-valued inputs, with its own fp64 warm chain in the closed
loops. Shapes: N = 20, B = 21 (no multiple of 4, across the 16-robot boundary), 6 ticks; tick 0 is cold from the
created iterate, which is at the origin (a primal step of size D through the fp32 IPM), and every fifth robot is reset
before tick 3 (the same step again).

Tolerance (far_field_cases.tol_scale, DESIGN.md "Coordinate range"): test_gpu_parity.py's TOL_U = TOL_X = 1e-3 and
TOL_UTRAJ = 5e-3, unchanged up to the supported radius R and times D / R beyond it: the error's only legitimate source
is ulp(D), which is linear in D. At every offset: status 0, finite outputs, qp_iter < qp_iter_max.

Measured (MI355X), the maxima over the forms; `warm` is the replayed warm-tick figure of test_run_closed_loop_far:
                    run mode, closed loop (cold and reset ticks included)     solve mode (warm)
  model  offset        u0       cmd      x        warm                        u0       x1       x        u
  diff   (0, 0)        1.0e-05  1.8e-06  4.5e-06  7.4e-06
         (64, -32)     1.8e-04  1.4e-05  8.6e-05  7.4e-06                     3.3e-06  2.7e-06  3.8e-06  3.8e-06
         (512, -256)   6.2e-04  4.5e-05  7.0e-04  6.4e-06                     4.1e-06  3.0e-05  3.0e-05  4.1e-06
         (4096, 2048)  8.4e-03  6.6e-04  5.3e-03  6.3e-06                     4.1e-06  2.4e-04  2.4e-04  4.1e-06
  omni4  (0, 0)        1.1e-05  1.0e-06  5.9e-06  2.1e-06
         (64, -32)     3.1e-05  1.2e-06  3.0e-05  1.9e-06                     3.1e-06  3.6e-06  3.8e-06  1.9e-05
         (512, -256)   2.6e-04  8.5e-06  3.9e-04  8.3e-06                     3.2e-06  2.9e-05  3.0e-05  2.0e-05
         (4096, 2048)  4.1e-03  1.1e-04  3.4e-03  8.1e-06                     4.7e-06  2.0e-04  2.4e-04  2.7e-05
  tric   (0, 0)        2.5e-06  1.1e-07  3.9e-05  2.4e-06
         (64, -32)     2.6e-06  1.1e-07  5.5e-06  2.5e-06                     4.1e-06  3.5e-06  1.3e-05  4.3e-05
         (512, -256)   3.4e-06  1.3e-07  7.4e-05  2.8e-06                     4.1e-06  3.0e-05  3.0e-05  4.2e-05
         (4096, 2048)  3.1e-06  1.4e-07  1.5e-03  2.5e-06                     3.9e-06  2.2e-04  2.4e-04  4.4e-05
Every status is 0, at most 19 IPM iterations. The worst u0 error is at most 5e-4 up to (64, -32) and 6.2e-4 at
(512, -256) (diff, Mehrotra's rule; 5.6e-4 with the default rule), so R = 64 m. The whole of it is the cold tick and
the reset tick (diff at 4096 m: 8.4e-3 on tick 0, 3.8e-3 on tick 3 and 2.8e-3 on the tick after it, about 2e-4 on the
others, where the two warm chains have drifted by that much): the primal step of size D goes through the fp32 IPM there, and its relative error of about 2e-6
times D lands in u0. tric's u0 sits on its bounds on those ticks and sees nothing. The warm figures are the state's
storage rounding, ulp(D) / 2, and nothing else. The shifted edge table at R: u0 <= 4.1e-5, x <= 3.9e-5, u <= 2.2e-4.

What the tests see, checked with scratch builds of the library that revert one thing each:
  * the shooting defect as xn - x_next with xn = x + step rounded at ulp(D) (the form before rk4_column returned the
    step's increment): test_run_closed_loop_far fails at (4096, 2048) for diff and omni4 in every form (the replayed
    warm ticks, e.g. [diff-team_plain-4096_2048]), test_solve_far at (4096, 2048) for every model and form (u0 up to
    5.2e-3, e.g. [diff-seg-4096_2048]); run mode's u0 at (512, -256) was 5.7e-4 then and the edge table's 1.4e-3;
  * the stopping rule's relative stationarity escape off (kStatRelT = 0): nothing fails and no IPM count of any tick
    changes. On these ticks the IPM leaves through the complementarity clauses (mu <= 1e-2 tol_comp, or stalled),
    never through stat_ok, so the rule's stationarity clause is not what the cold ticks depend on.
"""
import functools

import numpy as np
import pytest
import torch

import run_edge_cases as ec
from helpers import oracle_closed_loop
from nmpc_nav_control_amd._lib import default_params
from nmpc_nav_control_amd.scenario import make_fleet
from oracle.oracle import Oracle
from tests import far_field_cases as ff
from tests import robot_param_cases as rc
from tests.table_harness import CASES, DEV, FORMS, MODELS, Loop, check_tick, make_solver, state_of, t
from tests.test_gpu_parity import TOL_U, TOL_UTRAJ, TOL_X
from tests.test_gpu_run_edges import check_edges, state_host

pytestmark = pytest.mark.gpu
N, B, T, RESET_TICK = 20, 21, 6, 3
FEW = ("seg", "team_plain")  # the forms of the two near offsets, and of the tests that need one form per kernel


def report(what, model, form, off, **worst):
    """the worst errors of one (model, form, offset), printed with -s: the rows of the measured table"""
    print(f"far-field maxima {what} {model} {form} {ff.off_id(off)}: " + " ".join(f"{k} {v:.2e}" for k, v in worst.items()))


class BatchOracle:
    """Oracle.batch_tick over its own fp64 iterate and carried refs, in the form check_tick takes"""

    def __init__(self, model, carried):
        o = self.o = Oracle(model, N, rule="batched")
        self.xbar, self.ubar = np.zeros((B, N + 1, o.nx)), np.zeros((B, N, o.nu))
        for i in range(B):
            self.xbar[i], self.ubar[i] = o.iterate_create()
        self.carried = np.ascontiguousarray(carried, np.float64).copy()

    def tick(self, pose, vel, steer, traj, tlen, reset=None):
        nf, cmd, u0, st, it = self.o.batch_tick(pose, vel, steer, traj, tlen, reset, self.carried, self.xbar, self.ubar)
        return cmd, u0, st, it


def finite_and_inside(loop, model, tick):
    out = {k: v.cpu().numpy() for k, v in loop.out.items()}
    for k in ("cmd", "u0", "qp_res"):
        assert np.isfinite(out[k]).all(), (tick, k)
    assert out["qp_iter"].max() < default_params(model, N).qp_iter_max, (tick, out["qp_iter"])


RUN_CASES = [(m, f, off) for m, f in CASES for off in ff.OFFSETS if ff.distance(off) >= 512.0 or f in FEW]


@pytest.mark.parametrize("model,form,off", RUN_CASES, ids=lambda v: ff.off_id(v) if isinstance(v, tuple) else v)
def test_run_closed_loop_far(built, monkeypatch, model, form, off):
    solver = make_solver(monkeypatch, model, N, B, form)
    plan = solver.plan_ex(B, "run")
    assert FORMS[form][2](plan), plan
    loop = Loop(solver, model, B, offset=off)
    fleet = BatchOracle(model, loop.fl["carried"].T)
    mask = (np.arange(B) % 5 == 0).astype(np.uint8)
    mask_d = torch.from_numpy(mask).to(DEV)
    tol = TOL_U * ff.tol_scale(off)
    worst = dict(u0=0.0, cmd=0.0, x=0.0, warm=0.0)
    for tick in range(T):
        inp = loop.host_inputs()
        before = state_host(solver, B, fleet.o)
        loop.run(reset=mask_d if tick == RESET_TICK else None)
        if tick == 0:
            eu, ecmd = check_tick(loop, fleet, inp, tick, tol)  # the cold tick: the iterate is at the origin
        elif tick == RESET_TICK:
            eu, ecmd = check_tick(loop, fleet, inp, tick, tol, reset=mask)  # the reset tick: every fifth one is again
        else:
            eu, ecmd = check_tick(loop, fleet, inp, tick, tol)
        finite_and_inside(loop, model, tick)
        if tick not in (0, RESET_TICK):
            # Beyond the rule, which the cold and the reset tick set: a tick whose iterate is already at the robot
            # rounds nothing at ulp(D) but the store of x + dx (test_solve_far has the argument), so replayed through
            # the oracle from the handle's own state before the tick (tests/test_gpu_run_edges.py's form, in which the
            # two warm chains cannot drift apart) u0 and cmd keep the unchanged tolerance at every distance
            _, cmd_r, u0_r, st_r, _ = fleet.o.batch_tick(*inp, None, *before)
            ew = max(np.abs(loop.out["u0"].cpu().numpy().T - u0_r).max(),
                     np.abs(loop.out["cmd"].cpu().numpy().T - cmd_r).max())
            print(f"tick {tick}: replayed from the handle's state |du0|, |dcmd| <= {ew:.2e}")
            assert (st_r == 0).all(), (tick, st_r)
            assert ew <= TOL_U, (tick, ew, "warm tick, replayed")
            worst["warm"] = max(worst["warm"], float(ew))
        X = state_of(solver)[0][:, :B].cpu().numpy().astype(np.float64).T.reshape(B, N + 1, -1)
        worst.update(u0=max(worst["u0"], eu), cmd=max(worst["cmd"], ecmd),
                     x=max(worst["x"], float(np.abs(X - fleet.xbar).max())))
        loop.advance()
    report("run", model, form, off, **worst)


def round_quant(tick, pose, traj):
    return ec.f32(pose), ec.f32(traj)


@functools.lru_cache(maxsize=None)
def solve_reference(model, off):
    """The last tick's solve inputs of the oracle's closed loop on the shifted fleet, each rounded to fp32 once (the
    device gets that value, the oracle the same value widened), and the oracle's solution of each."""
    fl = ff.shift_fleet(make_fleet(model, B, seed=rc.SEED), off)
    o, rec = oracle_closed_loop(model, N, B, T, fl=fl, quant=round_quant)
    rec = [tuple(ec.f32(a) for a in r) for r in rec]
    sols = []
    for r in rec:
        st, _, xb, ub = o.sqp_rti(r[3], r[4], r[0], r[1], r[2])
        assert st == 0
        sols.append((xb, ub))
    return o, rec, sols


@pytest.mark.parametrize("off", ff.OFFSETS[1:], ids=ff.off_id)
@pytest.mark.parametrize("form", ["seg", "serial", "team_plain", "mehrotra"])
@pytest.mark.parametrize("model", MODELS)
def test_solve_far(built, monkeypatch, model, form, off):
    """solve mode, as test_solve_matches_oracle: u0, x1 and the full state and input trajectories"""
    o, rec, sols = solve_reference(model, off)
    solver = make_solver(monkeypatch, model, N, B, form)
    plan = solver.plan_ex(B, "solve")
    assert FORMS[form][2](plan), plan
    nx, nu = o.nx, o.nu
    xv, uv, _ = solver.state()
    xv.copy_from(t(np.stack([r[3] for r in rec]).reshape(B, -1).T))
    uv.copy_from(t(np.stack([r[4] for r in rec]).reshape(B, -1).T))
    out = dict(u0=torch.zeros(nu, B, device=DEV), x1=torch.zeros(nx, B, device=DEV),
               xtraj=torch.zeros((N + 1) * nx, B, device=DEV), utraj=torch.zeros(N * nu, B, device=DEV),
               status=torch.full((B,), -7, dtype=torch.int32, device=DEV),
               qp_iter=torch.zeros(B, dtype=torch.int32, device=DEV))
    solver.solve(t(np.stack([r[0] for r in rec]).T), t(np.stack([r[1] for r in rec]).transpose(1, 2, 0)),
                 We=t(np.stack([r[2] for r in rec]).T), **out)
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy().astype(np.float64) for k, v in out.items()}
    xb, ub = np.stack([s[0] for s in sols]), np.stack([s[1] for s in sols])
    err = dict(u0=np.abs(got["u0"].T - ub[:, 0]).max(), x1=np.abs(got["x1"].T - xb[:, 1]).max(),
               x=np.abs(got["xtraj"].T.reshape(B, N + 1, nx) - xb).max(),
               u=np.abs(got["utraj"].T.reshape(B, N, nu) - ub).max())
    report("solve", model, form, off, **err)
    print(f"status {out['status'].tolist()} qp_iter {out['qp_iter'].tolist()}")
    assert (out["status"] == 0).all(), out["status"]
    assert all(np.isfinite(got[k]).all() for k in ("u0", "x1", "xtraj", "utraj"))
    assert int(out["qp_iter"].max()) < default_params(model, N).qp_iter_max
    scale = ff.tol_scale(off)
    for k, tol in (("u0", TOL_U), ("x1", TOL_X), ("x", TOL_X), ("u", TOL_UTRAJ)):
        assert err[k] <= scale * tol, (k, err[k])
    # Beyond the rule, which the cold ticks of run mode set: a warm solve rounds nothing at ulp(D) but the store of
    # x + dx. The defect subtracts two stored states a stage apart before it adds the step (rk4_column), the cost
    # takes x - yref of two nearby values, and no input is a coordinate. So the inputs keep the unchanged tolerances
    # at every distance, and the states the unchanged one plus one ulp of the larger coordinate.
    ulp = float(np.spacing(np.float32(ff.distance(off))))
    for k, tol in (("u0", TOL_U), ("u", TOL_UTRAJ), ("x1", TOL_X + ulp), ("x", TOL_X + ulp)):
        assert err[k] <= tol, (k, err[k], "warm solve")


@pytest.mark.parametrize("form", FEW)
@pytest.mark.parametrize("model", MODELS)
def test_run_edges_far(built, monkeypatch, model, form):
    """test_gpu_run_edges.py's table, placements and assertions at the supported radius: the hack's equality test, the
    unwrap and the padding rules decide there as they do at the origin"""
    off = next(o for o in ff.OFFSETS if ff.distance(o) == ff.R)
    n = 21
    worst = check_edges(monkeypatch, model, form, n, ff.shift_cases(ec.cases(model, n), off), ff.tol_scale(off))
    report("edges", model, form, off, **worst)


@pytest.mark.parametrize("form", FEW)
@pytest.mark.parametrize("model", MODELS)
def test_distance_stays_on_its_robot(built, monkeypatch, model, form):
    """One batch with the four offsets interleaved robot by robot (i mod 4), so every wave and every 16-lane row mixes
    near and far: for the robots at the origin every output, the iterate rows, the carried refs and the warm flags are
    bit-identical to the same robots in an all-origin batch of the same size, in the same slots."""
    per = np.array([ff.OFFSETS[i % 4] for i in range(B)])
    near = torch.arange(0, B, 4, device=DEV)
    mixed, origin = (make_solver(monkeypatch, model, N, B, form) for _ in range(2))
    assert FORMS[form][2](mixed.plan_ex(B, "run"))
    a, b = Loop(mixed, model, B, offset=per), Loop(origin, model, B)
    mask = torch.from_numpy((np.arange(B) % 5 == 0).astype(np.uint8)).to(DEV)
    for tick in range(T):
        rs = mask if tick == RESET_TICK else None
        a.run(reset=rs)
        b.run(reset=rs)
        assert (a.out["status"] == 0).all() and (b.out["status"] == 0).all(), (tick, a.out["status"], b.out["status"])
        finite_and_inside(a, model, tick)
        for k in a.out:
            assert torch.equal(a.out[k][..., near], b.out[k][..., near]), (tick, k)
        for k, (x, y) in enumerate(zip(state_of(mixed), state_of(origin))):
            assert torch.equal(x[:, near], y[:, near]), (tick, k)
        a.advance()
        b.advance()
