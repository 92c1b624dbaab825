"""CPU checks of the stage-bound tests' reference (tests/stage_bound_cases.py): the spliced solve against the oracle's
own SQP-RTI step and against the independent dense restatement (tests/dense_qp.py), and the conditions of the ramp
rule that the GPU tests rely on (every QP of the ramp feasible, the abrupt drop infeasible on exactly the even
robots)."""
import numpy as np
import pytest

from tests import stage_bound_cases as sc
from tests.dense_qp import condense, dense_ipm, kkt_certificate
from tests.helpers import oracle_closed_loop

MODELS = ["diff", "omni4", "tric"]
ITER_MAX = {"diff": 24, "omni4": 16, "tric": 14}  # the ramp's largest IPM counts, of 50


@pytest.mark.parametrize("model", MODELS)
def test_uniform_profile_is_the_oracles_own_step(model):
    N, B = 20, 6
    o, rec = oracle_closed_loop(model, N, B, 4)
    for x0, yref, We, xbar, ubar in rec:
        s0, st0, xb0, ub0 = o.sqp_rti(xbar, ubar, x0, yref, We)
        s1, it1, xb1, ub1 = sc.solve_spliced(o, xbar, ubar, x0, yref, We, sc.uniform_box(o))
        assert s0 == s1 == 0 and st0["qp_iter"] == it1
        assert np.array_equal(xb0, xb1) and np.array_equal(ub0, ub1)


@pytest.fixture(scope="module")
def loops():
    """the 24-tick closed loops of the three variants, once per model, with the ramp's QPs of ticks 3 and 8 kept"""
    out = {}

    def get(model):
        if model not in out:
            kept = []

            def hook(t, i, o, args, box):
                if t in (3, 8):
                    kept.append((o, args, box))

            out[model] = dict(ramp=sc.cpu_closed_loop(model, 20, 12, 24, "ramp", hook=hook), kept=kept,
                              abrupt=sc.cpu_closed_loop(model, 20, 12, 4, "abrupt"),
                              default=sc.cpu_closed_loop(model, 20, 12, 24, "default"))
        return out[model]

    return get


@pytest.mark.parametrize("model", MODELS)
def test_spliced_qp_against_the_dense_restatement(loops, model):
    """ramp ticks 3 and 8: the inputs of the spliced solve against condense + dense_ipm on the same QP, to 1e-5
    (test_oracle.py's bar for this comparison)"""
    kept = loops(model)["kept"]
    assert len(kept) == 24
    for o, (xbar, ubar, x0, yref, We), box in kept:
        ix, iu = sc.idx(o)
        q = sc.spliced_qp(o, xbar, ubar, x0, yref, We, box)
        H, g, C, d, _, _ = condense(q, o.nbx, ix, o.nbu, iu)
        # dense_ipm at the tightest exit tolerance at which it converges: on diff's robot 0 (almost at rest, its ramp a
        # few stages long) it stalls just above its default 1e-12 and runs into its iteration limit with a stationarity
        # residual of 0.16 (tick 3) while the oracle's point is feasible with the lower objective. Its certificate on
        # the condensed QP is asserted, at test_oracle.py's bars, before it serves as the reference.
        for tol in (1e-12, 1e-11, 1e-10):
            with np.errstate(all="ignore"):
                u, z, it = dense_ipm(H, g, C, d, tol=tol)
            if it < 199 and np.isfinite(u).all():
                break
        stat, prim, dual, comp = kkt_certificate(H, g, C, d, u, z)
        assert stat <= 1e-9 * max(1.0, np.abs(g).max()) and prim <= 1e-10 and dual <= 0.0 and comp <= 1e-8
        st, _, _, ub = sc.solve_spliced(o, xbar, ubar, x0, yref, We, box)
        assert st == 0
        assert np.abs((ub - ubar).reshape(-1) - u).max() <= 1e-5


@pytest.mark.parametrize("model", MODELS)
def test_status_pattern_of_the_rule(loops, model):
    L = loops(model)
    ramp, abrupt, dflt = L["ramp"], L["abrupt"], L["default"]
    # the abrupt drop: status 4 on exactly the even robots at tick 3
    assert (abrupt["status"][3][0::2] == 4).all() and (abrupt["status"][3][1::2] == 0).all()
    assert all((s == 0).all() for s in abrupt["status"][:3])
    # the ramp: every QP solves, well inside the iteration limit, and the even robots reach their targets
    assert all((s == 0).all() for s in ramp["status"]), ramp["status"]
    assert max(it.max() for it in ramp["iters"]) <= ITER_MAX[model]
    target = 0.3 * ramp["cm"]
    speed = sc.speed_of(model, ramp["carried"])
    assert (speed[0::2] <= target[0::2] * 1.001).all(), (speed, target)
    # the table matters: the even robots' u0 leaves the default loop's, the odd robots' does not
    du = np.abs(ramp["u0"][8] - dflt["u0"][8]).max(axis=1)
    print(model, "tick 8 |u0 - u0_default|:", du.round(3).tolist())
    assert (du[1::2] == 0).all()
    assert np.sort(du[0::2])[1] > 0.2  # (all but at most one robot)
