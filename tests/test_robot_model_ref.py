"""CPU checks of the model-parameter rule (tests/robot_model_cases.py) that the GPU tests' tolerance relies on: every
oracle solve of the rule's closed loop succeeds well inside the iteration limit, putting any one parameter back to the
handle's value moves some robot's u0 by at least 15 x the GPU tolerance on the same inputs, and the four wave-mates of
the wave test get pairwise different solutions."""
import numpy as np
import pytest

from tests import robot_model_cases as mc

MODELS = ["diff", "omni4", "tric"]
TOL_U = 1e-3  # tests/test_gpu_robot_model.py's tolerance
N, B, T = 20, 9, 6


@pytest.fixture(scope="module")
def loops():
    """per model: the rule's closed loop, and per tick, robot and parameter j |u0(rule) - u0(p[j] reverted)|_inf on the
    same inputs"""
    out = {}

    def get(model):
        if model in out:
            return out[model]
        Pm = mc.robot_model(model, N, B)
        npar = Pm.shape[1]
        rule = mc.oracles(model, N, Pm)
        rev = [mc.oracles(model, N, mc.robot_model(model, N, B, revert=j)) for j in range(npar)]
        du = np.zeros((T, B, npar))

        def hook(t, i, pose, vel, steer, traj, carried, xbar, ubar):
            u = []
            for o in [rule[i]] + [rev[j][i] for j in range(npar)]:
                x0, yref, We = o.prepare(pose, vel, steer, traj, carried)
                st, _, _, ub = o.sqp_rti(xbar, ubar, x0, yref, We)
                assert st == 0
                u.append(ub[0])
            for j in range(npar):
                du[t, i, j] = np.abs(u[0] - u[1 + j]).max()

        out[model] = dict(log=mc.cpu_closed_loop(model, N, B, T, Pm, hook=hook), du=du, Pm=Pm)
        return out[model]

    return get


@pytest.mark.parametrize("model", MODELS)
def test_every_solve_of_the_rule_succeeds(loops, model):
    log = loops(model)["log"]
    iter_max = mc.oracle_for(model, N, loops(model)["Pm"][0]).prm.iter_max
    assert all((s == 0).all() for s in log["status"]), log["status"]
    top = max(int(it.max()) for it in log["iters"])
    print(model, "largest IPM count", top, "of", iter_max)
    assert top < iter_max


@pytest.mark.parametrize("model", MODELS)
def test_every_parameter_matters(loops, model):
    """ticks 1 to 5: reverting parameter j moves some robot's u0 by at least 15 x 1e-3"""
    L = loops(model)
    du, Pm = L["du"], L["Pm"]
    changed = np.abs(Pm - mc.handle_model(model, N, B)) > 0  # (a robot whose factor is 1 cannot move)
    for j in range(Pm.shape[1]):
        assert (du[:, ~changed[:, j], j] == 0).all()
        worst = du[1:, :, j].max(axis=1)
        print(model, f"p[{j}] reverted: max over robots |du0| per tick", du[:, :, j].max(axis=1).round(4).tolist())
        assert (worst >= 15 * TOL_U).all(), (j, worst)


@pytest.mark.parametrize("model", MODELS)
def test_wave_mates_differ(model):
    """one robot's state under the rule's columns 0 to 3: the four closed loops differ pairwise in u0 on ticks 1 to 3"""
    Pm = mc.robot_model(model, N, 4)
    log = mc.cpu_closed_loop(model, N, 4, 4, Pm, robots=[mc.WAVE_ROBOT[model]] * 4)
    assert all((s == 0).all() for s in log["status"])
    for t in (1, 2, 3):
        u = log["u0"][t]
        d = min(np.abs(u[a] - u[b]).max() for a in range(4) for b in range(a + 1, 4))
        print(model, "tick", t, "smallest pairwise |du0|", round(float(d), 4))
        assert d >= 15 * TOL_U, (t, d)
