"""The restatement of the separation guard (tests/sep_guard_ref.py) by hand, and the guard in the fp64 oracle's closed
loop on the scenes of tests/sep_guard_cases.py: the head-on pair, the crossing and the convoy. CPU only. The measured
figures are in tests/sep_guard_cases.py's docstring."""
import functools

import numpy as np
import pytest

from tests import sep_guard_cases as gc
from tests import sep_guard_ref as gr
from tests import separation_cases as cs
from tests import separation_ref as sp

F32 = np.float32
MODELS = ["diff", "omni4"]  # (the convoy tests' models)


# ---- the hold by hand ----------------------------------------------------------------------------------------------
def gaps(*m):
    """gap_all [N+1 = 6][B] whose smallest value over the stages 0..4 is m[i]; stage 5 is closer and outside the field"""
    g = np.full((6, len(m)), 2.0, F32)
    g[2] = m
    g[5] = 0.1
    return g


def test_hysteresis_on_a_gap_sequence():
    """held at m < stop, kept while stop <= m < release, released at m == release exactly, taken again only below stop"""
    stop, rel = F32(0.45), F32(0.55)
    below = np.nextafter(stop, F32(0))
    seq = [(0.60, 0), (stop, 0), (below, 1), (stop, 1), (0.50, 1), (np.nextafter(rel, F32(0)), 1), (rel, 0), (0.50, 0),
           (below, 1), (np.inf, 0)]
    held = np.zeros(1, np.uint8)
    for m, want in seq:
        held = gr.hold(gaps(m), held, **gr.GUARD)
        assert held.tolist() == [want], (m, want)


def test_the_field_is_the_first_stages_and_clamps():
    g = gaps(0.5, 0.5)
    assert gr.hold(g, np.zeros(2, np.uint8), **dict(gr.GUARD, hold_stages=5)).tolist() == [1, 1]  # (stage 5: 0.1)
    assert gr.hold(g, np.zeros(2, np.uint8), **dict(gr.GUARD, hold_stages=9)).tolist() == [1, 1]  # (clamps to N)
    assert gr.hold(g, np.zeros(2, np.uint8), **dict(gr.GUARD, hold_stages=1)).tolist() == [0, 0]
    g[0, 0] = 0.3
    assert gr.hold(g, np.zeros(2, np.uint8), **dict(gr.GUARD, hold_stages=0)).tolist() == [1, 0]
    g[:] = np.nan  # (a NaN never counts)
    assert gr.hold(g, np.ones(2, np.uint8), **gr.GUARD).tolist() == [0, 0]


def test_reset_modes_and_the_switch():
    g = gaps(0.2, 0.2, 0.2, 0.2, 0.2)
    held = np.array([0, 1, 0, 1, 1], np.uint8)
    assert gr.hold(g, held, reset=[1, 1, 0, 0, 0], **gr.GUARD).tolist() == [0, 0, 1, 1, 1]  # a reset robot: never
    mode = [gr.GOTO_POSE, gr.FOLLOW_PATH, 0, 3, 4]  # IDLE, BREAK and ERROR clear held
    assert gr.hold(g, held, mode=mode, **gr.GUARD).tolist() == [1, 1, 0, 0, 0]
    assert gr.hold(g, held, **dict(gr.GUARD, hold=0)).tolist() == [0] * 5


# ---- qy, qa and who stands by hand --------------------------------------------------------------------------------
def one_robot(held=0, reset=0):
    """a robot whose iterate drives along +x from the origin, 0.1 m per stage, N = 4, and whose pose is (1, 0)"""
    N, nx = 4, 3
    xbar = np.zeros(((N + 1) * nx, 1), F32)
    xbar[0::nx, 0] = F32(0.1) * np.arange(N + 1, dtype=F32)
    pose = np.array([[1.0], [0.0], [0.0]], F32)
    return gr.positions(xbar, nx, N, 1, pose, [reset], [held]), (xbar, nx, N, pose)


def test_standing_and_direction():
    (pos, h), _ = one_robot()
    assert pos[:, 0, 0].tolist() == [F32(0.1) * F32(k) for k in range(5)] and (h[:, 0, 0] > 0).all()
    (pos, h), _ = one_robot(held=1)  # stands at its pose, keeps the iterate's direction
    assert (pos[:, 0, 0] == 1).all() and (h[:, 0, 0] > 0).all()
    (pos, h), _ = one_robot(reset=1)  # stands and has no direction
    assert (pos[:, 0, 0] == 1).all() and (h == 0).all()
    (pos, h), _ = one_robot(held=1, reset=1)
    assert (pos[:, 0, 0] == 1).all() and (h == 0).all()
    # a track behind a held robot does not count, one behind a reset robot does
    xy = np.array([[0.5, 0.0]]).T[None].copy()
    for kw, counts in ((dict(held=1), False), (dict(reset=1), True)):
        (pos, h), _ = one_robot(**kw)
        _, qa = gr.minima(pos, h, xy)
        assert np.isfinite(qa).all() == counts, kw


def test_right_of_way():
    (pos, h), _ = one_robot()
    xy = np.array([[1.0, 0.0], [2.0, 0.0], [1.5, 0.0]]).T[None].copy()  # ahead, 1, 2 and 1.5 m from the origin
    near = (F32(1.0) - pos[:, 0, 0]) ** 2
    mid, far = (F32(1.5) - pos[:, 0, 0]) ** 2, (F32(2.0) - pos[:, 0, 0]) ** 2
    for pr, own, want in (([5, 5, 5], [5], near),              # ties count
                          ([4, 5, 5], [5], mid),               # the nearest one yields to the robot
                          ([4, 5, 4], [5], far),
                          ([4, 4, 4], [5], np.full(5, np.inf)),  # the robot has right of way over everything
                          ([gr.INT_MIN, gr.INT_MAX, gr.INT_MIN], [gr.INT_MAX], far),
                          ([gr.INT_MIN, 0, 0], [gr.INT_MIN], near)):
        qy, qa = gr.minima(pos, h, xy, priority=np.array(pr, np.int32), own_priority=np.array(own, np.int32))
        assert np.array_equal(qy[:, 0], np.asarray(want, F32)), (pr, own)
        assert np.array_equal(qa[:, 0], near.astype(F32))  # the hold sees everything
    qy, qa = gr.minima(pos, h, xy)
    assert np.array_equal(qy, qa)
    # own_priority NULL: priority[own_first + i]; the own track is skipped by index, not by priority
    xy4 = np.concatenate([xy, np.zeros((1, 2, 1))], axis=2)
    qy, _ = gr.minima(pos, h, xy4, own_first=3, priority=np.array([4, 5, 4, 5], np.int32))
    assert np.array_equal(qy[:, 0], far.astype(F32))


def test_limits_without_priorities_or_held_are_the_rules():
    _, (xbar, nx, N, pose) = one_robot()
    xy = np.array([[0.9, 0.1], [0.2, -0.4]]).T[None].copy()
    car = np.full((1, 1), 0.3, F32)
    lim, gap, gap_all = gr.limits(xbar, nx, N, 1, xy, F32(1), F32(1), 0.05, car, 1, pose=pose)
    pos = sp.sr.stage_positions(xbar, nx, N, 1)
    want, want_gap = sp.limits(pos, xy, F32(1), F32(1), 0.05, car, 1)
    assert np.array_equal(lim.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(gap.view(np.uint32), want_gap.view(np.uint32)) and np.array_equal(gap, gap_all)


# ---- the scenes ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def head_on(model, guarded):
    if not guarded:
        return gc.closed_loop(model, gc.head_on_fleet(model), 260)
    return gc.closed_loop(model, gc.head_on_fleet(model), gc.HEAD_ON_TICKS, guard=gc.GUARD,
                          retarget={gc.RETARGET: gc.HEAD_ON_NEW_GOAL})


@pytest.mark.parametrize("model", MODELS)
def test_head_on_pair_is_held(model):
    stop, rel = gc.GUARD["stop_gap"], gc.GUARD["release_gap"]
    plain = head_on(model, False)
    assert plain["dist"].min() < stop and (plain["status"] == 0).all(), plain["dist"].min()  # (the scene matters)
    log = head_on(model, True)
    R, held, ev = gc.RETARGET, log["held"], log["event"]
    first = int(np.argmax(held.all(axis=1)))
    assert 0 < first < R and held[first:R].all() and (ev[first:R] == gc.EV_HELD).all()
    assert not held[:first].all(axis=1).any()
    solved = log["status"][:first][~held[:first].astype(bool)]
    assert (solved == 0).all() and (log["status"][first:R] == -1).all()
    d = log["dist"][first - 1] - log["dist"][R - 1]  # from the decision to standstill
    print(f"{model}: held from tick {first}; closes {d * 1e3:.2f} mm after the decision; smallest centre distance "
          f"{log['dist'][:R].min():.4f} m")
    assert d <= 2 * gc.D_STOP and log["dist"][:R].min() >= stop - 2 * gc.D_STOP
    assert abs(log["dist"][R - 1] - log["dist"][R - 20]) < 1e-5  # (standstill: the run-down is exponential)
    assert (log["mode"][:R] == gc.GOTO_POSE).all()  # the mode stays: a held robot resumes by itself
    # robot 0 is given a goal behind it with its reset flag: not held in that cycle, it solves and leaves
    i, _ = gc.HEAD_ON_NEW_GOAL
    other = 1 - i
    assert held[R, i] == 0 and ev[R, i] == gc.EV_SOLVED and not held[R:, i].any()
    assert held[R, other] == 1
    freed = R + int(np.argmin(held[R:, other]))
    assert R < freed < gc.HEAD_ON_TICKS and held[R:freed, other].all() and not held[freed:, other].any()
    # (the leaving robot's track is its iterate, whose stage 0 is the pose of the tick before: m lags the distance)
    assert log["dist"][freed - 1] >= rel > log["dist"][R]
    ran = log["status"][R:] != -1
    assert (log["status"][R:][ran] == 0).all()  # every resumed solve: the hold never needs to write reset
    assert (ev[freed:, other] == gc.EV_SOLVED).all() and log["dist"][-1] > log["dist"][freed]
    print(f"{model}: robot {other} released at tick {freed} at {log['dist'][freed - 1]:.4f} m")


@functools.lru_cache(maxsize=None)
def crossing(model, which):
    fl = gc.crossing_fleet(model)
    if which == "none":
        return gc.closed_loop(model, fl, gc.CROSS_TICKS, tracks=False)
    if which == "equal":  # today's behaviour: nobody has right of way, nobody is held
        return gc.closed_loop(model, fl, gc.CROSS_EQUAL_TICKS, guard=dict(gc.GUARD, hold=0))
    return gc.closed_loop(model, fl, gc.CROSS_TICKS, guard=gc.GUARD, priority=gc.CROSS_PRIORITY)


def all_arrived(log):
    """the first tick by which every robot has reported ARRIVED"""
    got = log["event"] == gc.EV_ARRIVED
    assert got.any(axis=0).all(), "a robot never arrives"
    return int(np.argmax(got, axis=0).max())


@pytest.mark.parametrize("model", MODELS)
def test_crossing_with_right_of_way(model):
    none, equal, prio = (crossing(model, w) for w in ("none", "equal", "prio"))
    cap = F32(1.0)
    assert none["dist"].min() < gc.RULE["clearance"], none["dist"].min()  # (the scene matters)
    assert ((equal["lim"][:, 1, :] < cap).any(axis=0)).all()  # equal priorities: both slow down, as without a guard
    win = int(np.argmax(gc.CROSS_PRIORITY))
    assert np.array_equal(prio["lim"][:, :, win].view(np.uint32), none["lim"][:, :, win].view(np.uint32))
    assert (prio["lim"][:, 1, 1 - win] < cap).any()
    assert not prio["held"].any() and not (prio["event"] == gc.EV_HELD).any()
    for log in (none, equal, prio):
        assert (log["status"][log["status"] != -1] == 0).all()
    t_prio, t_equal = all_arrived(prio), all_arrived(equal)
    print(f"{model}: both arrived by tick {t_prio} with priorities, {t_equal} with equal ones; smallest centre "
          f"distance {prio['dist'].min():.3f} / {equal['dist'].min():.3f} m, no tracks {none['dist'].min():.3f} m")
    assert t_prio < t_equal
    assert prio["dist"].min() >= gc.GUARD["stop_gap"]


def test_equal_priorities_without_hold_are_the_unguarded_rule():
    a = crossing("diff", "equal")
    b = gc.closed_loop("diff", gc.crossing_fleet("diff"), gc.CROSS_EQUAL_TICKS, guard=None)
    for k in ("lim", "pose", "status", "event"):
        assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("model", MODELS)
def test_convoy_with_the_default_guard_is_the_convoy(model):
    """nobody is ever held, and every limit, status and distance is the unguarded run's bit for bit"""
    want = cs.closed_loop(model, True)
    got = gc.closed_loop(model, cs.convoy_fleet(model), cs.TICKS, guard=gc.GUARD)
    assert not got["held"].any()
    assert np.array_equal(got["status"], want["status"]) and np.array_equal(got["dist"], want["dist"])
    assert np.array_equal(got["lim"][:, 1, :].view(np.uint32), want["lim1"].astype(F32).view(np.uint32))
    cs.distances_ok(got["dist"], True)
