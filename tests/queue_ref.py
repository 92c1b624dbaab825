"""fp64 restatement of the path-set bookkeeping of NMPCNavControlROS for one robot and one tick, the oracle of
nmpc_batch_node_tick_queue (include/nmpc_amd/nmpc_batch.h, steps 1 to 9 there): processPathReceived's
processPathBuffers(0.0) (NMPCNavControlROS.cpp:573), processPathBuffers (:576-595), the pop of the parts behind the
robot (:603-609), the path errors with the front part's sign (:654-657), the hop to the next queued part (:685-690) and
pubControlStatus' patch_remains (:374-375). The robot's whole part list stays where it is; active_path_ is the parts
[head, tail) and upcoming_path_ the parts [tail, npart).

Everything else is tests/node_ref.py's (the other modes, the guard, the end test), tests/path_ref.py's discretizer and
tests/path_nearest_ref.py's search. Like node_ref, queue_ref takes the device's nearest parameter `U` in place of its
own search, and with it the device's near pose and position error at that parameter (nmpc_path_nearest's outputs on
the same window): the heading error is then formed here from the near pose with additions and fmod only, which are
exact to the bit on both sides.

Ties: node_ref's MARGIN guard, extended to the active length L against max_active_len. A velocity product that is
exactly 0 with a part queued behind it is refused as well (its sign test would hang on the sign of a zero).
"""
import math
from collections import namedtuple

from tests import node_ref as nr
from tests.node_ref import MARGIN, TieError, _arrived, _clear  # noqa: F401
from tests.path_nearest_ref import near_err, nearest_one, norm_ang
from tests.path_ref import PathDiscretizer, TPath

EV_NEXT_PART = 7
# nmpc_path_queue_default: SetPathLength(1000) (:571) and max_active_path_length (nmpc_nav_control.yaml:6)
QDEFAULT = dict(part_length=1000.0, max_active_len=5.0)

QTick = namedtuple("QTick", "mode event solves poses traj_len head tail path_u err remains")


def clamp(v, lo, hi):
    return lo if v < lo else (hi if v > hi else v)


def window(npart, head, tail, stride):
    """step 1: (nP, h, t), never past the robot's own records"""
    nP = clamp(int(npart), 0, int(stride))
    h = clamp(int(head), 0, nP)
    t = clamp(int(tail), h, nP)
    return nP, h, t


def fill(q, segs, frames, lengths, h, t, nP, U):
    """processPathBuffers(U) (:576-595) on the window [h, t) of the parts segs[0:nP]; returns the new t"""
    def length(k):
        return q["part_length"] if lengths is None else float(lengths[k])

    L = 0.0
    for k in range(h, t):
        L += length(k) * (1 - U) if k == h else length(k)  # :580-581
    while True:
        if t < nP:
            _clear(L, q["max_active_len"], "active path length")
        if not (L < q["max_active_len"] and t < nP):  # :584
            break
        if t > h:
            vv = float(segs[t - 1][12]) * float(segs[t][12])
            if vv == 0.0:
                raise TieError("velocity product of exactly 0 before a queued part")
            if vv < 0.0:  # :588
                break
            if frames is not None and int(frames[t - 1]) != int(frames[t]):  # :589
                break
        t += 1  # :591-592
        L += length(t - 1)  # :593
    return t


def open_window(q, segs, npart, head, tail, stride, frames=None, lengths=None):
    """steps 1 and 2: the window the nearest-point search runs on, (nP, h, t); t == h: no search this tick"""
    nP, h, t = window(npart, head, tail, stride)
    if nP >= 1 and t == h:
        t = fill(q, segs, frames, lengths, h, t, nP, 0.0)  # processPathReceived's processPathBuffers(0.0), :573
    return nP, h, t


def remains_of(nP, h, path_u):
    """pubControlStatus (:374-375): active_path_.size() + upcoming_path_.size(), less active_path_u_"""
    r = float(nP - h)
    return r - path_u if r > 0 else r


def queue_ref(p, q, mode, pose, N, goal=None, segs=None, npart=0, head=0, tail=0, path_u=0.0, stride=None,
              frames=None, lengths=None, omni4=False, U=None, near=None, pos_err=None):
    """One robot, one tick. p: nmpc_node_params fields, q: part_length and max_active_len; segs [S][16] the robot's
    whole part list (None: the caller passed no paths), npart / head / tail / path_u its window and progress, frames /
    lengths [S] or None. U, near (x, y, theta, theta_holonomic), pos_err: the device's search result on the window
    open_window returns, in place of the oracle's own. Returns QTick; head, tail and path_u are what the tick leaves
    behind, remains is NaN unless the robot is still in FollowPath."""
    nan = math.nan
    none = (nan, nan)
    pose = [float(v) for v in pose]
    m = min(int(mode), nr.ERROR)
    if m == nr.FOLLOW_PATH and segs is None:
        m = nr.ERROR
    if m != nr.FOLLOW_PATH:
        t = nr.node_ref(p, m, pose, N, goal=goal)
        return QTick(t.mode, t.event, t.solves, t.poses, t.traj_len, head, tail, path_u, none, nan)
    stride = len(segs) if stride is None else stride
    nP, h, t = window(npart, head, tail, stride)
    if nP < 1:
        return QTick(nr.IDLE, nr.EV_NONE, False, None, 0, head, tail, path_u, none, nan)  # as nseg < 1: untouched
    if t == h:
        t = fill(q, segs, frames, lengths, h, t, nP, 0.0)
        if t == h:
            return QTick(nr.IDLE, nr.EV_NONE, False, None, 0, h, t, path_u, none, nan)  # executeNMPC's empty list
    # step 3: processNearestPoint on active_path_ (:599-601)
    n = t - h
    win = segs[h:t]
    if U is None:
        U = nearest_one(win, n, (pose[0], pose[1]), (float(path_u), nan))[0]
    U = float(U)
    if near is None:
        near, e = near_err(win, n, U, pose, omni4)
        pos_err = float(e[0])
    # step 4: the pop (:603-609)
    k = int(math.floor(U))
    if n > k:
        for _ in range(k):
            h += 1
            U = U - 1
    # step 5
    t = fill(q, segs, frames, lengths, h, t, nP, U)
    # step 6 (:654-657): the sign is the front part's after the pop
    if omni4:
        theta = float(near[3])
    else:
        theta = float(near[2]) + math.pi if float(segs[h][12]) < 0.0 else float(near[2])
    err = (float(pos_err), abs(norm_ang(theta - pose[2])))
    if p["enable_safe_conditions"]:
        _clear(err[0], p["max_pos_err"], "position error to path")
        _clear(err[1], p["max_ori_err"], "orientation error to path")
        if err[0] >= p["max_pos_err"] or err[1] >= p["max_ori_err"]:
            return QTick(nr.ERROR, nr.EV_OFF_PATH, False, None, 0, h, t, U, err, nan)
    # step 7
    disc = PathDiscretizer(p["sample_period"], N + 1, bool(p["is_holonomic"]))
    poses, _ = disc.getNextNPoses([TPath(segs[j]) for j in range(h, t)], U)
    # step 8 (:681-694)
    if _arrived(p, pose, poses[-1]):
        if t == nP:
            return QTick(nr.IDLE, nr.EV_ARRIVED, False, None, 0, h, t, U, err, nan)
        h, t = h + 1, t + 1  # pop_front, push the upcoming front: no sign or frame test (:687-689)
        return QTick(nr.FOLLOW_PATH, EV_NEXT_PART, False, None, 0, h, t, 0.0, err, remains_of(nP, h, 0.0))
    return QTick(nr.FOLLOW_PATH, nr.EV_SOLVED, True, poses, N + 1, h, t, U, err, remains_of(nP, h, U))


def after_solve(tick, status):
    """executeNMPC's exception (:716-719): Error, and pubControlStatus no longer reports a remainder"""
    if tick.solves and status != 0:
        return tick._replace(mode=nr.ERROR, event=nr.EV_SOLVE_FAILED, remains=math.nan)
    return tick
