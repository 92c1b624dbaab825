"""fp64 restatement of the branches of NMPCNavControlROS::mainCycle (NMPCNavControlROS.cpp:516-538, processBreak
:612-616, processGoToPose :618-646, processFollowPath :648-698, executeNMPC :700-720) for one robot, the oracle of
nmpc_batch_node_tick's gate. The nearest point is tests/path_nearest_ref.py's, the discretizer tests/path_ref.py's.

node_ref returns what the node decides before the solve; a failed solve (status != 0 -> Error, SOLVE_FAILED) is the
caller's to apply (after_solve). Every quantity compared with a threshold must be at least MARGIN away from it, so a
GPU test can never pass or fail on a tie: node_ref raises otherwise.
"""
import math
from collections import namedtuple

from tests.path_nearest_ref import near_err, nearest_one, norm_ang
from tests.path_ref import PathDiscretizer, TPath

IDLE, GOTO_POSE, FOLLOW_PATH, BREAK, ERROR = 0, 1, 2, 3, 4
EV_NONE, EV_SOLVED, EV_ARRIVED, EV_GOAL_TOO_FAR, EV_OFF_PATH, EV_SOLVE_FAILED, EV_BREAK = range(7)
MARGIN = 1e-9  # m or rad

DEG = math.pi / 180.0
# the shipped nmpc_nav_control.yaml (:7-13), degrees converted
DEFAULT = dict(final_pos_err=0.01, final_ori_err=1.0 * DEG, max_goal_dist=2.0, max_pos_err=0.5, max_ori_err=60.0 * DEG,
               enable_safe_conditions=1, final_ori_signed=1, sample_period=1.0 / 40.0, is_holonomic=0)

Tick = namedtuple("Tick", "mode event solves poses traj_len path_u err")


class TieError(AssertionError):
    pass


def _clear(value, threshold, what):
    """the comparison value <op> threshold is decided by more than MARGIN (NaN and infinite operands never tie)"""
    if math.isfinite(value) and math.isfinite(threshold) and abs(value - threshold) < MARGIN:
        raise TieError(f"{what}: {value!r} within {MARGIN} of its threshold {threshold!r}")


def dist(x0, y0, x1, y1):
    return math.sqrt((x0 - x1) ** 2 + (y0 - y1) ** 2)


def _arrived(p, pose, ref):
    """the end-of-trajectory test (:636-639, :681-684): the signed angle, as the node writes it"""
    d = dist(pose[0], pose[1], ref[0], ref[1])
    ang = norm_ang(pose[2] - ref[2])
    if not p["final_ori_signed"]:
        ang = abs(ang)
    _clear(d, p["final_pos_err"], "end test distance")
    _clear(ang, p["final_ori_err"], "end test angle")
    return d <= p["final_pos_err"] and ang <= p["final_ori_err"]


def node_ref(p, mode, pose, N, goal=None, segs=None, nseg=0, path_u=0.0, omni4=False, U=None):
    """One robot, one tick. p: dict of nmpc_node_params fields; pose / goal: 3 floats (the fp32 inputs widened);
    segs [S][16], nseg, path_u: the robot's active path and its progress (None: the caller passed no paths); omni4:
    the holonomic heading in the path error. U: take this nearest parameter (the device's) instead of the oracle's
    own search, e.g. to march from the same point. Returns Tick(mode', event, solves, poses [N+1][3] or None,
    traj_len, path_u', err (pos, ori))."""
    nan = math.nan
    pose = [float(v) for v in pose]
    none = (nan, nan)
    mode = int(mode)
    if mode > ERROR:
        mode = ERROR
    if mode == GOTO_POSE and goal is None:
        mode = ERROR
    if mode == FOLLOW_PATH and segs is None:
        mode = ERROR
    if mode in (IDLE, ERROR):
        return Tick(mode, EV_NONE, False, None, 0, path_u, none)
    if mode == BREAK:
        return Tick(IDLE, EV_BREAK, False, None, 0, path_u, none)
    if mode == GOTO_POSE:
        goal = [float(v) for v in goal]
        d = dist(goal[0], goal[1], pose[0], pose[1])
        if p["enable_safe_conditions"]:
            _clear(d, p["max_goal_dist"], "goal distance")
            if d >= p["max_goal_dist"]:
                return Tick(IDLE, EV_GOAL_TOO_FAR, False, None, 0, path_u, none)
        if _arrived(p, pose, goal):
            return Tick(IDLE, EV_ARRIVED, False, None, 0, path_u, none)
        return Tick(GOTO_POSE, EV_SOLVED, True, [tuple(goal)] * (N + 1), 1, path_u, none)
    # FollowPath
    n = int(nseg)
    if n < 1:
        return Tick(IDLE, EV_NONE, False, None, 0, path_u, none)  # executeNMPC's empty list (:702-705)
    if U is None:
        U = nearest_one(segs, n, (pose[0], pose[1]), (float(path_u), nan))[0]
    _, err = near_err(segs, n, U, pose, omni4)
    err = (float(err[0]), float(err[1]))
    if p["enable_safe_conditions"]:
        _clear(err[0], p["max_pos_err"], "position error to path")
        _clear(err[1], p["max_ori_err"], "orientation error to path")
        if err[0] >= p["max_pos_err"] or err[1] >= p["max_ori_err"]:
            return Tick(ERROR, EV_OFF_PATH, False, None, 0, U, err)
    disc = PathDiscretizer(p["sample_period"], N + 1, bool(p["is_holonomic"]))
    poses, _ = disc.getNextNPoses([TPath(segs[k]) for k in range(n)], U)
    if _arrived(p, pose, poses[-1]):
        return Tick(IDLE, EV_ARRIVED, False, None, 0, U, err)
    return Tick(FOLLOW_PATH, EV_SOLVED, True, poses, N + 1, U, err)


def after_solve(tick, status):
    """the node after executeNMPC: an exception (status != 0) sends it to Error (:716-719)"""
    if tick.solves and status != 0:
        return tick._replace(mode=ERROR, event=EV_SOLVE_FAILED)
    return tick
