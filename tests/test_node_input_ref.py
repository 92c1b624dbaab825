"""CPU checks of the host restatement of the node's input stage (tests/node_input_ref.py) and of the case stream
(tests/node_input_cases.py): the restatement against cases worked by hand, the velocity against an independent form on
an exact circle, and the stream's planted cases, each of which must really occur for at least one robot."""
import math

import numpy as np

from tests import node_input_cases as nc
from tests import node_input_ref as nr
from tests.frame_ref import Frames

MS = 1000000


def ring(depth=4, cap=3, tric=False, frames=None):
    return nr.InputRef(cap, depth, tric=tric, frames=frames)


def push1(r, t, x, y, yaw, i=0):
    B = r.cap
    st = np.zeros(B, np.int64)
    smp = np.zeros((3, B))
    st[i], smp[:, i] = t, (x, y, yaw)
    mask = np.zeros(B, np.uint8)
    mask[i] = 1
    return int(r.push(st, smp, mask)[i])


def test_sec_is_ros_duration_to_sec():
    assert nr.sec(0) == 0.0 and nr.sec(25 * MS) == 0.025 and nr.sec(1500 * MS) == 1.5
    assert nr.sec(-1) == -1.0 + 1e-9 * 999999999.0  # floor, then a non-negative nanosecond part
    assert nr.sec(-25 * MS) == -1.0 + 1e-9 * 975000000.0
    assert nr.sec(3 * nr.NS + 7) == 3.0 + 1e-9 * 7.0


def test_listener_by_hand():
    r = ring(depth=2)
    assert r.count[0] == 0 and (r.held == 0).all()
    assert push1(r, 100, 1.0, 2.0, 0.5) == 0
    assert (r.count[0], r.newest[0], r.stamp[0, 0]) == (1, 0, 100)  # an empty ring: slot 0
    assert push1(r, 100, 9.0, 9.0, 9.0) == 1 and push1(r, 99, 9.0, 9.0, 9.0) == 1  # not after the newest: dropped
    assert push1(r, 200, math.inf, 0.0, 0.0) == 1 and push1(r, 200, 0.0, 0.0, math.nan) == 1  # not finite
    assert (r.count[0], r.newest[0]) == (1, 0) and r.sample[0, :, 0].tolist() == [1.0, 2.0, 0.5]
    assert push1(r, 200, 3.0, 4.0, 0.6) == 0 and (r.count[0], r.newest[0]) == (2, 1)
    why = [set() for _ in range(r.cap)]
    st, smp = np.array([300, 0, 0], np.int64), np.zeros((3, 3))
    assert r.push(st, smp, np.array([1, 0, 0], np.uint8), why).tolist() == [0, 0, 0]
    assert (r.count[0], r.newest[0]) == (2, 0) and why[0] == {"wrap"}  # count saturates, the oldest is overwritten
    assert [t for t, _ in r.stored(0)] == [200, 300]
    assert r.count[1] == 0 and (r.stamp[:, 1:] == 0).all()  # the masked-off robots: untouched


def test_lookup_by_hand():
    r = ring()
    for k, t in enumerate((1000, 2000, 4000)):
        push1(r, t, float(k), 10.0 * k, 0.1 * k)
    assert r.lookup(0, 999) is None and r.lookup(0, 4001) is None and r.lookup(1, 1000) is None
    assert r.lookup(0, 2000) == (1.0, 10.0, 0.1)
    x, y, yaw = r.lookup(0, 2500)  # a quarter of the way from the second to the third
    assert (x, y) == (0.75 * 1.0 + 0.25 * 2.0, 0.75 * 10.0 + 0.25 * 20.0) and yaw == 0.1 + 0.25 * nr.norm_ang(0.2 - 0.1)
    # the yaw goes the short way round
    r = ring()
    push1(r, 0, 0.0, 0.0, 3.0)
    push1(r, 100, 0.0, 0.0, -3.0)
    assert abs(r.lookup(0, 50)[2] - (3.0 + 0.5 * (2.0 * math.pi - 6.0))) < 1e-15


def test_unwrap_hack_by_hand():
    pi = math.pi
    assert nr.unwrap_hack(0.0, 1.0) == 1.0
    assert nr.unwrap_hack(3.0, -3.0) == -3.0 + 2.0 * pi  # delta < -pi
    assert nr.unwrap_hack(-3.0, 3.0) == 3.0 - 2.0 * pi   # delta > pi
    why = set()
    assert nr.unwrap_hack(6.2, 0.4, why) == (0.4 + 2.0 * pi) - 2.0 * pi and why == {"unwrap_up", "clamp_pos"}
    why = set()
    assert nr.unwrap_hack(-6.2, -0.4, why) == (-0.4 - 2.0 * pi) + 2.0 * pi and why == {"unwrap_down", "clamp_neg"}
    assert math.isnan(nr.unwrap_hack(0.0, math.nan))  # (and returns)
    assert nr.unwrap_hack(0.0, 1e300) == 1e300        # no value spins the loops


def test_stage_by_hand():
    """two samples one period apart: pose, velocity, validity and the held values"""
    T = 5 * nr.NS
    r = ring(tric=True)
    mode = np.array([nr.GOTO_POSE, nr.IDLE, nr.FOLLOW_PATH], np.uint8)
    steer, ok = np.array([0.25, 0.5, 0.75], np.float32), np.array([1, 1, 0], np.uint8)
    out = r.stage(T, mode, steer, ok)
    assert out["valid"].tolist() == [0, 1, 0] and out["why"][0] == {"empty"} and (r.held[:6] == 0).all()
    assert r.held[nr.HSTEER].tolist() == [0.25, 0.0, 0.0]  # IDLE: untouched; steer_ok 0: held
    push1(r, T - 25 * MS, 1.0, 1.0, 0.0)
    out = r.stage(T, mode, steer, ok)
    assert out["pose_ok"][0] and not out["vel_ok"][0] and "before_oldest" in out["why"][0]
    assert r.held[:3, 0].tolist() == [1.0, 1.0, 0.0] and (r.held[3:6, 0] == 0).all()
    push1(r, T, 1.0 + 0.025, 1.0, 0.0)
    out = r.stage(T + MS, mode, steer, ok)
    assert out["valid"][0] == 1 and "exact" in out["why"][0]
    assert r.held[nr.HV, 0] == (1.025 - 1.0) / 0.025 and r.held[nr.HVN, 0] == 0.0 and r.held[nr.HW, 0] == 0.0
    assert out["pose"][:, 0].tolist() == [np.float32(1.025), 1.0, 0.0] and out["steer_out"][0] == 0.25
    # stale: the pose is written, valid follows pose_valid_overwritten
    push1(r, T + 25 * MS, 2.0, 1.0, 0.0)
    late = T + 25 * MS + 101 * MS
    out = r.stage(late, mode, steer, ok)
    assert not out["pose_ok"][0] and out["valid"][0] == 1 and r.held[nr.HX, 0] == 2.0
    assert r.stage(late, mode, steer, ok, pose_valid_overwritten=0)["valid"][0] == 0
    assert r.stage(late - MS, mode, steer, ok, pose_valid_overwritten=0)["valid"][0] == 1  # exactly the timeout: ok
    # dt <= 0 and dt > transform_timeout hold the velocity
    v = r.held[nr.HV, 0]
    for period in (0, -25 * MS, 101 * MS):
        out = r.stage(T + 26 * MS, mode, steer, ok, period_ns=period)
        assert not out["vel_ok"][0] and out["valid"][0] == 0 and r.held[nr.HV, 0] == v, period
    # the second robot never ran; the third is invalid through its steering alone
    assert (r.held[:, 1] == 0).all() and out["valid"][1] == 1 and "steer_bad" in out["why"][2]


def test_stage_recentres_and_converts_the_goal():
    cap, N, nx = 3, 2, 5
    fr = Frames(cap, N, nx, np.zeros(((N + 1) * nx, cap), np.float32))
    r = ring(cap=cap, frames=fr)
    push1(r, 10 * MS, 500000.25, 4649776.5, 0.0)
    mode = np.array([nr.GOTO_POSE, nr.IDLE, nr.IDLE], np.uint8)
    goal = np.array([[500001.0, 1.0, 2.0], [4649777.0, 1.0, 2.0], [0.5, 0.0, 0.0]])
    out = r.stage(20 * MS, mode, goal_map=goal, recentre_radius=8.0)
    assert out["moved"].tolist() == [1, 0, 0] and fr.origin[:, 0].tolist() == [500000.0, 4649776.0]
    assert out["pose"][:, 0].tolist() == [0.25, 0.5, 0.0] and out["goal_out"][:, 0].tolist() == [1.0, 1.0, 0.5]
    assert fr.xbar[0, 0] == np.float32(-500000.0) and fr.xbar[1, 0] == np.float32(-4649776.0)  # the iterate moved
    out = r.stage(20 * MS, mode, goal_map=goal, recentre_radius=8.0)
    assert out["moved"].tolist() == [0, 0, 0]
    out = r.stage(20 * MS, mode, goal_map=goal)  # an infinite radius: the origins are still read
    assert out["pose"][:, 0].tolist() == [0.25, 0.5, 0.0]


def test_velocity_on_an_exact_circle():
    """a robot on a circle of radius R at rate w, heading along the tangent: the independent form R(-mid_yaw) (dx, dy) /
    dt, and the closed form v = 2 R sin(w dt / 2) / dt, vn = 0, omega = w"""
    R, w, dt = 3.0, 0.7, 0.025
    for k in range(40):
        a1 = -3.0 + 0.17 * k
        a2 = a1 + w * dt
        p1 = (R * math.cos(a1), R * math.sin(a1), nr.norm_ang(a1 + math.pi / 2))
        p2 = (R * math.cos(a2), R * math.sin(a2), nr.norm_ang(a2 + math.pi / 2))
        v, vn, om = nr.body_velocity(p1, p2, dt)
        mid = p1[2] + nr.norm_ang(p2[2] - p1[2]) / 2.0
        c, s = math.cos(mid), math.sin(mid)
        d = np.array([[c, s], [-s, c]]) @ np.array([p2[0] - p1[0], p2[1] - p1[1]]) / dt
        assert abs(v - d[0]) < 1e-12 and abs(vn - d[1]) < 1e-12
        assert abs(v - 2.0 * R * math.sin(w * dt / 2.0) / dt) < 1e-11 and abs(vn) < 1e-11 and abs(om - w) < 1e-11


def run_stream(depth, tric=True, radius=nc.RADIUS):
    fr = Frames(nc.CAP, 2, 5, np.zeros((15, nc.CAP), np.float32))
    r = nr.InputRef(nc.CAP, depth, tric=tric, frames=fr)
    met = [set() for _ in range(nc.B)]
    log = []
    for cyc in nc.stream():
        for st, smp, mk in cyc["pushes"]:
            dropped = r.push(st, smp, mk, met)
            for i in np.flatnonzero(dropped):
                met[i].add("dropped_nan" if not np.isfinite(smp[:, i]).all() else "dropped_order")
        out = r.stage(cyc["now_ns"], cyc["mode"], cyc["steer"], cyc["steer_ok"], cyc["goal_map"],
                      recentre_radius=radius)
        for i in range(nc.B):
            met[i] |= out["why"][i]
        log.append(out)
    return r, met, log


def test_the_stream_contains_every_planted_case():
    r, met, log = run_stream(4)
    assert len(log) == nc.CYCLES == 12
    have = lambda k: [i for i in range(nc.B) if k in met[i]]  # noqa: E731
    assert have("empty") == [0]
    assert 1 in have("stale")
    assert len(have("before_oldest")) >= nc.B - 8  # the first cycle of every robot that runs
    assert 2 in have("exact") and "interp" not in met[2]
    assert len(have("interp")) >= 10 and len(have("interp_older_pair")) >= 1
    assert 3 in have("unwrap_up") and 4 in have("unwrap_down")
    assert 3 in have("clamp_pos") and 4 in have("clamp_neg")
    assert have("dropped_order") == [5] and have("dropped_nan") == [6]
    assert len(have("wrap")) >= nc.B - 2
    assert have("steer_bad") == [7]
    assert sum(int(out["moved"][8]) for out in log) >= 2  # crosses the radius again after its first move
    # the robots that do not run keep their held values, whatever their rings hold
    assert (r.held[:, [9, 10, 11]] == 0).all() and r.count[9] == 4 and all(o["valid"][9] == 1 for o in log)
    assert (r.held[:, nc.B:] == 0).all() and (r.count[nc.B:] == 0).all()
    # validity: the empty ring never, the first cycle nobody that runs, later nearly everybody
    assert all(o["valid"][0] == 0 for o in log) and log[0]["valid"][[2, 3, 12]].tolist() == [0, 0, 0]
    assert log[-1]["valid"].sum() == nc.B - 1
    assert log[3]["valid"][7] == 0 and log[5]["valid"][7] == 1


def test_depth_two_still_interpolates_or_fails_cleanly():
    """with two slots t1 is either bracketed by the two stored samples or before the older one"""
    r, met, log = run_stream(2)
    assert any("interp" in m for m in met) and any("before_oldest" in m for m in met)
    assert "exact" in met[2] and (r.count[:nc.B][1:] == 2).all()
