"""Hand-computed cases of tests/node_ref.py, one per branch of the node's state machine (CPU only)."""
import math

import numpy as np
import pytest

from tests import node_ref as nr
from tests.path_cases import _line

N = 8
P = dict(nr.DEFAULT)
LINE = np.array([_line((0, 0), (2, 0), 0.5)])  # y = 0, x in [0, 2], 0.5 m/s: 0.0125 m per pose


def test_idle_error_break_and_bad_mode():
    for m in (nr.IDLE, nr.ERROR):
        t = nr.node_ref(P, m, (0, 0, 0), N)
        assert (t.mode, t.event, t.solves) == (m, nr.EV_NONE, False)
    t = nr.node_ref(P, nr.BREAK, (0, 0, 0), N)
    assert (t.mode, t.event, t.solves) == (nr.IDLE, nr.EV_BREAK, False)
    t = nr.node_ref(P, 9, (0, 0, 0), N)
    assert (t.mode, t.event, t.solves) == (nr.ERROR, nr.EV_NONE, False)


def test_missing_inputs_are_an_error():
    assert nr.node_ref(P, nr.GOTO_POSE, (0, 0, 0), N, goal=None)[:3] == (nr.ERROR, nr.EV_NONE, False)
    assert nr.node_ref(P, nr.FOLLOW_PATH, (0, 0, 0), N, segs=None)[:3] == (nr.ERROR, nr.EV_NONE, False)


def test_goto_pose_branches():
    # 2.5 m away: too far with the guard on, a solve with it off
    t = nr.node_ref(P, nr.GOTO_POSE, (0, 0, 0), N, goal=(2.5, 0, 0))
    assert (t.mode, t.event, t.solves) == (nr.IDLE, nr.EV_GOAL_TOO_FAR, False)
    t = nr.node_ref(dict(P, enable_safe_conditions=0), nr.GOTO_POSE, (0, 0, 0), N, goal=(2.5, 0, 0))
    assert (t.mode, t.event, t.solves, t.traj_len) == (nr.GOTO_POSE, nr.EV_SOLVED, True, 1)
    assert t.poses == [(2.5, 0.0, 0.0)] * (N + 1)
    # 5 mm and 0.5 degrees: arrived
    t = nr.node_ref(P, nr.GOTO_POSE, (0.003, 0.004, 0.5 * nr.DEG), N, goal=(0, 0, 0))
    assert (t.mode, t.event, t.solves) == (nr.IDLE, nr.EV_ARRIVED, False)
    # 5 mm and +2 degrees: not yet
    t = nr.node_ref(P, nr.GOTO_POSE, (0.003, 0.004, 2 * nr.DEG), N, goal=(0, 0, 0))
    assert (t.mode, t.event, t.solves) == (nr.GOTO_POSE, nr.EV_SOLVED, True)
    # 3 cm: not yet
    assert nr.node_ref(P, nr.GOTO_POSE, (0.03, 0, 0), N, goal=(0, 0, 0)).solves


def test_signed_angle_quirk():
    """ang = normAngRad(pose.theta - goal.theta) = -1 rad: the node's signed comparison says arrived, |ang| not"""
    pose, goal = (0.003, 0.004, 0.0), (0.0, 0.0, 1.0)
    t = nr.node_ref(P, nr.GOTO_POSE, pose, N, goal=goal)
    assert (t.mode, t.event, t.solves) == (nr.IDLE, nr.EV_ARRIVED, False)
    t = nr.node_ref(dict(P, final_ori_signed=0), nr.GOTO_POSE, pose, N, goal=goal)
    assert (t.mode, t.event, t.solves) == (nr.GOTO_POSE, nr.EV_SOLVED, True)
    # +1 rad has not arrived under either rule
    assert nr.node_ref(P, nr.GOTO_POSE, (0.003, 0.004, 1.0), N, goal=(0, 0, 0)).solves


def test_follow_path_branches():
    # no segments: executeNMPC's empty list
    t = nr.node_ref(P, nr.FOLLOW_PATH, (0, 0, 0), N, segs=LINE, nseg=0)
    assert (t.mode, t.event, t.solves) == (nr.IDLE, nr.EV_NONE, False)
    # 0.1 m beside x = 0.5 (U = 0.25), heading 0.2 rad: solves on 9 poses 0.0125 m apart
    t = nr.node_ref(P, nr.FOLLOW_PATH, (0.5, 0.1, 0.2), N, segs=LINE, nseg=1)
    assert (t.mode, t.event, t.solves, t.traj_len) == (nr.FOLLOW_PATH, nr.EV_SOLVED, True, N + 1)
    assert abs(t.path_u - 0.25) < 1e-12 and abs(t.err[0] - 0.1) < 1e-12 and abs(t.err[1] - 0.2) < 1e-12
    xs = [q[0] for q in t.poses]
    assert len(xs) == N + 1 and abs(xs[0] - 0.5125) < 2e-4 and abs(xs[-1] - 0.5 - 9 * 0.0125) < 2e-3
    # the search never goes back behind path_u
    t = nr.node_ref(P, nr.FOLLOW_PATH, (0.5, 0.1, 0.2), N, segs=LINE, nseg=1, path_u=0.4)
    assert t.path_u == 0.4 and abs(t.err[0] - math.hypot(0.3, 0.1)) < 1e-12
    # each threshold of the path guard on its own
    t = nr.node_ref(P, nr.FOLLOW_PATH, (0.5, 0.6, 0.2), N, segs=LINE, nseg=1)
    assert (t.mode, t.event, t.solves) == (nr.ERROR, nr.EV_OFF_PATH, False) and abs(t.path_u - 0.25) < 1e-12
    t = nr.node_ref(P, nr.FOLLOW_PATH, (0.5, 0.1, 1.2), N, segs=LINE, nseg=1)
    assert (t.mode, t.event, t.solves) == (nr.ERROR, nr.EV_OFF_PATH, False)
    # guard off: by the switch, and by an infinite threshold
    assert nr.node_ref(dict(P, enable_safe_conditions=0), nr.FOLLOW_PATH, (0.5, 0.6, 1.2), N, segs=LINE, nseg=1).solves
    assert nr.node_ref(dict(P, max_pos_err=math.inf), nr.FOLLOW_PATH, (0.5, 0.6, 0.2), N, segs=LINE, nseg=1).solves
    assert not nr.node_ref(dict(P, max_pos_err=math.inf), nr.FOLLOW_PATH, (0.5, 0.6, 1.2), N, segs=LINE, nseg=1).solves
    # 6 mm before the path end, along it: every pose is the end, and the robot has arrived
    t = nr.node_ref(P, nr.FOLLOW_PATH, (1.994, 0.0, 0.0), N, segs=LINE, nseg=1)
    assert (t.mode, t.event, t.solves) == (nr.IDLE, nr.EV_ARRIVED, False) and abs(t.path_u - 0.997) < 1e-12
    # omni4 takes the holonomic heading (0 on LINE) where diff takes the tangent (+ pi when driven backwards)
    back = np.array([_line((0, 0), (2, 0), -0.5)])
    assert abs(nr.node_ref(P, nr.FOLLOW_PATH, (0.5, 0.1, 0.2), N, segs=back, nseg=1, omni4=True).err[1] - 0.2) < 1e-12
    assert nr.node_ref(P, nr.FOLLOW_PATH, (0.5, 0.1, 0.2), N, segs=back, nseg=1).event == nr.EV_OFF_PATH


def test_a_tie_is_refused():
    with pytest.raises(nr.TieError):
        nr.node_ref(P, nr.GOTO_POSE, (0.01, 0, 0), N, goal=(0, 0, 0))
    with pytest.raises(nr.TieError):
        nr.node_ref(P, nr.GOTO_POSE, (2.0, 0, 0), N, goal=(0, 0, 0))
    with pytest.raises(nr.TieError):
        nr.node_ref(P, nr.FOLLOW_PATH, (0.5, 0.5, 0.0), N, segs=LINE, nseg=1)
    with pytest.raises(nr.TieError):
        nr.node_ref(P, nr.GOTO_POSE, (0.001, 0, P["final_ori_err"] + 1e-12), N, goal=(0, 0, 0))


def test_failed_solve_goes_to_error():
    t = nr.node_ref(P, nr.GOTO_POSE, (0.5, 0, 0), N, goal=(0, 0, 0))
    assert nr.after_solve(t, 0) == t
    f = nr.after_solve(t, 1)
    assert (f.mode, f.event) == (nr.ERROR, nr.EV_SOLVE_FAILED)
    idle = nr.node_ref(P, nr.IDLE, (0, 0, 0), N)
    assert nr.after_solve(idle, 1) == idle
