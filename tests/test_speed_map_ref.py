"""The speed map's rule in the fp64 oracle's closed loop (tests/speed_map_cases.py), 16 robots, N = 20, on map A: the
six conditions that pin the rule and its inputs. They hold for the reference alone; the device is held to the same
reference in tests/test_gpu_speed_map.py.

Measured (diff / omni4 / tric): IPM iterations at most 23 / 17 / 16; the limit binds on 235 / 299 / 117 of 640
robot-ticks; the carried speed exceeds lim_1 by at most 3.9e-14; from tick 20 on a robot exceeds its own cell's limit by
at most 3.9e-3 (omni4; one ramp step is 0.02); the abrupt variant fails 137 / 258 / 126 of 480 solves; without a map
166 / 204 / 98 of 480 robot-ticks are above their cell's limit by more than 1e-3."""
import functools

import numpy as np
import pytest

from tests import speed_map_cases as mc
from tests import speed_map_ref as sr

MODELS = ["diff", "omni4", "tric"]
N, B, T = 20, 16, 40


@functools.lru_cache(maxsize=None)
def loop(model, variant, ticks):
    return mc.closed_loop(model, N, B, ticks, variant)


@pytest.mark.parametrize("model", MODELS)
def test_rule_in_closed_loop(built, model):
    L = loop(model, "rule", T)
    g = L["g"]
    assert abs(g - 0.02) < 1e-6  # 0.8 * a_max * dt with the defaults
    assert (L["status"] == 0).all(), np.argwhere(L["status"] != 0)
    over = (L["speed"] - L["lim1"]).max()
    bind = int((L["speed"] >= L["lim1"] - 1e-3).sum())
    zone = (L["speed"][20:] - L["zone"][20:]).max()
    print(f"{model}: iters <= {L['iters'].max()}, binds {bind} of {L['speed'].size}, speed - lim_1 <= {over:.1e}, "
          f"speed - cell limit from tick 20 <= {zone:.1e}")
    assert over <= 1e-9
    assert bind >= 0.1 * L["speed"].size
    assert zone <= g


@pytest.mark.parametrize("model", MODELS)
def test_abrupt_limit_fails_solves(built, model):
    A = loop(model, "abrupt", 30)
    fails = int((A["status"] != 0).sum())
    print(f"{model}: the cell limit at every stage fails {fails} of {A['status'].size} solves")
    assert fails >= 1


@pytest.mark.parametrize("model", MODELS)
def test_without_a_map_the_fleet_speeds_through_the_zones(built, model):
    Z = loop(model, "none", 30)
    above = int((Z["speed"] - Z["zone"] > 1e-3).sum())
    print(f"{model}: without a map {above} of {Z['speed'].size} robot-ticks above the cell's limit")
    assert (Z["status"] == 0).all()
    assert above >= 0.1 * Z["speed"].size


def test_restatement_by_hand():
    """the rule on numbers worked by hand: a 3 x 2 grid of 1 m cells at (10, 20); g = 0.8 * 0.5 * 0.25 = 0.1"""
    m = sr.Map(10.0, 20.0, 1.0, [[0.6, np.inf, 0.2], [np.nan, 0.9, 0.3]], outside=0.7)
    X = np.array([10.5, 11.5, 12.5, 9.5, 10.0, 13.0, 10.5, np.nan])
    Y = np.array([20.5, 20.5, 20.5, 20.5, 21.0, 20.0, 22.0, 20.5])
    got = m.cell(X, Y)
    want = np.array([0.6, np.inf, 0.2, 0.7, np.nan, 0.7, 0.7, 0.7], np.float32)  # half a cell below x0 is outside
    assert np.array_equal(got, want, equal_nan=True)
    # one robot driving along y = 20.5 from x = 10.5 in steps of 0.5: cells 0.6, 0.6, inf, inf, 0.2; cap 1
    pos = np.zeros((5, 2, 1), np.float32)
    pos[:, 0, 0], pos[:, 1, 0] = [10.5, 11.0 - 1e-3, 11.5, 12.0 - 1e-3, 12.5], 20.5
    lim = sr.limits(m, pos, 1.0, 0.5, 0.25, np.array([[0.45], [-0.55]], np.float32), 2, slope=0.8, v_floor=0.05)
    f = np.float32
    g = (f(0.8) * f(0.5)) * f(0.25)
    z = [f(0.6), f(0.6), f(1.0), f(1.0), f(0.2)]
    r = [min(z[j] + f(j - k) * g for j in range(k, 5)) for k in range(5)]
    want = [max(r[k], f(0.55) - f(k) * g) for k in range(5)]
    assert lim[:, 0].tolist() == want
    assert np.allclose(want, [0.6, 0.5, 0.4, 0.3, 0.2], atol=1e-6)  # the ramp into the 0.2 zone, then c - k g below it
    # tric: only the first carried state is a speed; a NaN cell acts as v_floor
    pos[:] = np.array([10.5, 21.5], np.float32)[None, :, None]
    lim = sr.limits(m, pos, 1.0, 0.5, 0.25, np.array([[0.0], [-0.55]], np.float32), 1)
    assert lim[:, 0].tolist() == [f(0.05)] * 5
