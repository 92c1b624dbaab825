"""Run mode's on-device pre-solve (x0 packing with direct kinematics, the references' heading unwrap, padding past
traj_len, diff's terminal-weight hack) and post-solve (vel-ref carry, inverse kinematics, command) at their edges,
in every kernel form, against the fp64 oracle (-m gpu).

The pre-solve exists three times (the team kernel's plain pass, its split launch, the row-parallel kernel's last
wave), each with its own loop, clamp and end condition. The case table (tests/run_edge_cases.py; shown to be a valid
instrument, and to see every mistake of tests/prepare_ref.py at >= 10 x the tolerance, by
tests/test_run_edge_cases.py) goes through nmpc_batch_run itself here: list lengths around N + 1 over garbage rows,
the hack's boundary, +-pi crossings once and many times per list, a goal across the cut, a pose heading outside
[-pi, pi], every velocity sign, tric's steering angles, a reset.

Matrix: model x form x N in {20, 21, 22} (N + 1 meets every remainder of the row-parallel kernel's three-buffer
rotation and of the team pass's two-ahead loads), and N in {1, 2} on the plain team form and the default form. The
forms are tests/table_harness.py's and the two-wave segmented row-parallel form (>= 257 robots; omni4 takes
the team kernel there, so it has none). Placement: rc.placements -- B = 81 (257), no multiple of 4, each of the
traj_len = N and the multi-crossing cases once in slot 0 and in the last slot (one batch per such case) and on both
sides of a 16-robot boundary.

Per tick (tests/sim_regress.py's replay form, so errors do not compound): the handle's iterate and carried refs are
read before the tick and the tick is replayed through Oracle.batch_tick from exactly that state. Then status is 0 on
both sides, |u0|, |cmd|, the carried refs and the new resident state trajectory agree within 1e-3 and the new
resident inputs within 5e-3: tests/test_gpu_parity.py's TOL_U, TOL_X and TOL_UTRAJ, with the derivation given there.

Measured (MI355X), the maxima over the forms, horizons, placements and ticks per model; every case passes in every
form, at most 17 IPM iterations:
           u0       cmd      carried  state trajectory  inputs
  diff     1.8e-05  1.7e-06  4.5e-07  4.9e-06           1.9e-04
  omni4    1.5e-04  3.5e-06  3.8e-06  5.1e-06           1.8e-04
  tric     2.9e-05  7.2e-07  7.2e-07  9.8e-06           2.4e-04

What the test sees, checked with scratch builds of the library that revert one thing each:
  * the heading comparison of the hack dropped in both kernels: every diff parametrisation fails, no other;
  * a kernel that does not pad at all -- the clamp of the row it reads (`kt`) and the `k < len` of RefUnwrap::step both
    reverted: in the team kernel every team form of every model fails and no row-parallel one, in the row-parallel
    kernel the other way round.
Each of those two guards alone is redundant, which is why reverting only one of them changes no bit of any result: with
the `kt` clamp alone gone the rows past traj_len are read and then dropped by step's `in` select, and with `k < len`
alone gone the last valid pose is read again and unwrapped again, which gives the value it already had (the raw
heading is at most one 2 pi step from its unwrapped self: tests/prepare_ref.py, unwrap_pad).
"""
import numpy as np
import pytest
import torch

import run_edge_cases as rc
from nmpc_nav_control_amd._lib import default_params
from nmpc_nav_control_amd.batch import BatchSolver
from oracle.oracle import Oracle
from tests.test_gpu_parity import TOL_U, TOL_UTRAJ, TOL_X
from tests.table_harness import FORMS as PARAM_FORMS

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
MODELS = ["diff", "omni4", "tric"]

# form: (environment, qp_ipm, what nmpc_batch_plan_ex must report); FORMS adds the robots the form needs at least
FORMS = {k: v + (0,) for k, v in PARAM_FORMS.items()}
FORMS["seg"] = FORMS["seg"][:2] + (lambda p: PARAM_FORMS["seg"][2](p) and p["waves_per_robot"] == 4, 0)
FORMS["seg_w2"] = ({}, 1, lambda p: p["kernel"] == "rowpar" and p["segments"] > 0 and p["waves_per_robot"] == 2, 257)
# what a caller gets without overrides: at the shortest horizons and these sizes the row-parallel kernel, so that with
# the plain team form both kernels see N = 1 and N = 2
FORMS["default"] = ({}, 1, lambda p: p["kernel"] == "rowpar", 0)


def has_form(model, form):
    return not (form == "rec_split" and model != "diff") and not (form == "seg_w2" and model == "omni4")


MATRIX = [(m, f, N) for m in MODELS for f in FORMS if f != "default" and has_form(m, f) for N in (20, 21, 22)]
MATRIX += [(m, f, N) for m in MODELS for f in ("team_plain", "default") for N in (1, 2)]


def t(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device=DEV, dtype=dtype)


def host(a):
    return np.ascontiguousarray(a.cpu().numpy(), np.float64)


def solver_of(monkeypatch, model, N, B, form):
    """a handle of B robots created under the form's launch-choice overrides (read at creation) and IPM rule"""
    env, ipm, _, _ = FORMS[form]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    prm = default_params(model, N)
    prm.qp_ipm = ipm
    return BatchSolver(model, N, B, params=prm, device=DEV)


class Outs:
    def __init__(self, s, B):
        self.cmd = torch.full((3, B), 7.0, device=DEV)
        self.u0 = torch.full((s.nu, B), 7.0, device=DEV)
        self.status = torch.full((B,), -7, dtype=torch.int32, device=DEV)
        self.qp_iter = torch.full((B,), -7, dtype=torch.int32, device=DEV)

    def kw(self):
        return dict(cmd=self.cmd, u0=self.u0, status=self.status, qp_iter=self.qp_iter)


def device_inputs(model, inp):
    pose, vel, steer, traj, tlen, reset = inp
    return dict(pose=t(pose.T), vel=t(vel.T), steer=t(steer) if model == "tric" else None,
                traj=t(traj.transpose(1, 2, 0)), traj_len=t(tlen, torch.int32), reset=t(reset, torch.uint8))


def state_host(s, B, o):
    """the resident state of the first B robots as the oracle holds it: carried [B][nbx], xbar [B][N+1][nx],
    ubar [B][N][nu]"""
    torch.cuda.synchronize()
    X, U, C = (v.to_tensor() for v in s.state())
    return (np.ascontiguousarray(host(C[:, :B]).T), np.ascontiguousarray(host(X[:, :B]).T.reshape(B, o.N + 1, o.nx)),
            np.ascontiguousarray(host(U[:, :B]).T.reshape(B, o.N, o.nu)))


@pytest.mark.parametrize("model,form,N", MATRIX)
def test_run_edges_match_oracle(built, monkeypatch, model, form, N):
    check_edges(monkeypatch, model, form, N, rc.cases(model, N))


def check_edges(monkeypatch, model, form, N, cs, scale=1.0):
    """the table cs (rc.cases(model, N), or that table moved: tests/test_gpu_far_field.py) through nmpc_batch_run in
    every placement, each tick replayed through the oracle; scale: the factor on the three tolerances. Returns the
    maxima."""
    o = Oracle(model, N, rule="batched")
    worst = dict(u0=0.0, cmd=0.0, carried=0.0, x=0.0, u=0.0)
    for order in rc.placements(cs, FORMS[form][3]):
        B = len(order)
        assert B <= 300 and B % 4 and B % 16
        s = solver_of(monkeypatch, model, N, B, form)
        plan = s.plan_ex(B, "run")
        assert FORMS[form][2](plan), (form, plan)
        out = Outs(s, B)
        for tick in range(rc.T):
            inp = rc.batch_inputs(cs, tick, order)
            names = [cs[i].name for i in order]
            carried, xbar, ubar = state_host(s, B, o)
            _, cmd_o, u0_o, st_o, it_o = o.batch_tick(inp[0], inp[1], inp[2] if model == "tric" else None, inp[3],
                                                      inp[4], inp[5], carried, xbar, ubar)
            s.run(**device_inputs(model, inp), **out.kw())
            carried_g, xbar_g, ubar_g = state_host(s, B, o)
            st = out.status.cpu().numpy()
            err = dict(u0=np.abs(host(out.u0).T - u0_o).max(1), cmd=np.abs(host(out.cmd).T - cmd_o).max(1),
                       carried=np.abs(carried_g - carried).max(1), x=np.abs(xbar_g - xbar).max((1, 2)),
                       u=np.abs(ubar_g - ubar).max((1, 2)))
            where = {k: (names[int(np.argmax(v))], int(np.argmax(v))) for k, v in err.items()}
            print(f"{model} {form} N={N} B={B} tick {tick} ({plan['kernel']}): qp_iter <= {int(out.qp_iter.max())} "
                  f"(oracle {int(it_o.max())}) " + " ".join(f"{k} {v.max():.2e}" for k, v in err.items()))
            worst = {k: max(v, float(err[k].max())) for k, v in worst.items()}
            assert (st_o == 0).all(), (tick, [(names[i], int(st_o[i])) for i in np.flatnonzero(st_o)])
            assert (st == 0).all(), (tick, [(names[i], i, int(st[i])) for i in np.flatnonzero(st)])
            for k, tol in (("u0", TOL_U), ("cmd", TOL_U), ("carried", TOL_U), ("x", TOL_X), ("u", TOL_UTRAJ)):
                assert err[k].max() <= scale * tol, (tick, k, float(err[k].max()), where[k])
        s.close()
    print(f"maxima {model} {form} N={N}: " + " ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    return worst


def run_ticks(s, model, cs, order, variant):
    """T ticks of the placement on one handle; variant(kw) edits each tick's arguments. Returns every tick's outputs
    and the resident state after the last one."""
    B = len(order)
    out, got = Outs(s, B), []
    for tick in range(rc.T):
        kw = device_inputs(model, rc.batch_inputs(cs, tick, order))
        variant(kw)
        s.run(**kw, **out.kw())
        torch.cuda.synchronize()
        got += [v.clone() for v in out.kw().values()]
    return got + [v.to_tensor()[:, :B].clone() for v in s.state()]


@pytest.mark.parametrize("form", ["seg", "team_plain"])
@pytest.mark.parametrize("model", MODELS)
def test_absent_arguments_are_their_defaults_bit_for_bit(built, monkeypatch, model, form):
    """traj_len=None against a full array of N + 1 and, for tric, steer=None against an array of zeros: the same
    launches bit for bit, on the rows of the table with full lists"""
    N = 21
    cs = [c for c in rc.cases(model, N) if c.ticks[0]["traj_len"] == N + 1]
    assert any(c.marks for c in cs) and len(cs) >= 15
    order = rc.placements(cs)[0]
    B = len(order)
    res = {}
    for variant in ("given", "no_len") + (("no_steer",) if model == "tric" else ()):
        s = solver_of(monkeypatch, model, N, B, form)
        assert FORMS[form][2](s.plan_ex(B, "run"))

        def edit(kw, variant=variant):
            assert (kw["traj_len"] == N + 1).all()
            if model == "tric":
                kw["steer"] = torch.zeros(B, device=DEV)
            if variant == "no_len":
                kw["traj_len"] = None
            if variant == "no_steer":
                kw["steer"] = None
        res[variant] = run_ticks(s, model, cs, order, edit)
        s.close()
    given = res.pop("given")
    assert len(given) == 4 * rc.T + 3 and (given[2] == 0).all()  # (the first tick's status)
    for variant, got in res.items():
        assert len(got) == len(given)
        for k, (a, b) in enumerate(zip(given, got)):
            assert torch.equal(a, b), (variant, k)
