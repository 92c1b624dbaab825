"""Scenarios of the path-queue tests, host side only (numpy): tests/test_queue_ref.py runs them through
tests/queue_ref.py with its own search to show that none sits on a tie, tests/test_gpu_queue.py runs them on the device.
"""
import math

import numpy as np

from tests import node_ref as nr
from tests import queue_ref as qr
from tests.path_cases import _line

N = 8  # tests/test_gpu_node.py's horizon
S = 6  # segment records per robot


class QFleet:
    """Host arrays of B robots with path sets: mode [B], pose / goal [B][3] (fp32), vel [B][3], segs [B][S][16] (NaN
    past npart), npart / head / tail [B], path_u [B], frame [B][S], length [B][S], reset [B]. arrays: the fleet's
    queue carries frame and length (else every part counts part_length and all frames are equal)."""

    def __init__(self, B, arrays=False, q=None):
        self.B, self.arrays = B, arrays
        self.q = dict(qr.QDEFAULT, **(q or {}))
        self.mode = np.zeros(B, np.uint8)
        self.pose = np.zeros((B, 3), np.float32)
        self.vel = np.zeros((B, 3), np.float32)
        self.goal = np.full((B, 3), np.nan, np.float32)
        self.segs = np.full((B, S, 16), np.nan)
        self.npart = np.zeros(B, np.int32)
        self.head = np.zeros(B, np.int32)
        self.tail = np.zeros(B, np.int32)
        self.path_u = np.zeros(B)
        self.frame = np.zeros((B, S), np.int32)
        self.length = np.full((B, S), self.q["part_length"])
        self.reset = np.zeros(B, np.uint8)

    def set_parts(self, i, recs, head=0, tail=0, path_u=0.0, npart=None, frames=None, lengths=None):
        self.segs[i] = np.nan
        if len(recs):
            self.segs[i, :len(recs)] = recs
        self.npart[i] = len(recs) if npart is None else npart
        self.head[i], self.tail[i], self.path_u[i] = head, tail, path_u
        if frames is not None:
            self.frame[i, :len(frames)] = frames
        if lengths is not None:
            self.length[i, :len(lengths)] = lengths

    def ref_args(self, i):
        return dict(goal=self.goal[i].astype(np.float64), segs=self.segs[i], npart=self.npart[i], head=self.head[i],
                    tail=self.tail[i], path_u=self.path_u[i], stride=S,
                    frames=self.frame[i] if self.arrays else None, lengths=self.length[i] if self.arrays else None)

    def open_windows(self):
        """(nP, h, t) per robot after steps 1 and 2, (0, 0, 0) for the robots that do not search"""
        out = []
        for i in range(self.B):
            w = (0, 0, 0)
            if int(self.mode[i]) == nr.FOLLOW_PATH:
                a = self.ref_args(i)
                w = qr.open_window(self.q, a["segs"], a["npart"], a["head"], a["tail"], S, a["frames"], a["lengths"])
                if w[0] < 1:
                    w = (0, 0, 0)
            out.append(w)
        return out

    def ref(self, p, omni4=False, search=None):
        """queue_ref of every robot; search: per robot None or (U, near[4], pos_err), the device's"""
        out = []
        for i in range(self.B):
            kw = {}
            if search is not None and search[i] is not None:
                kw = dict(U=search[i][0], near=search[i][1], pos_err=search[i][2])
            out.append(qr.queue_ref(p, self.q, self.mode[i], self.pose[i].astype(np.float64), N, omni4=omni4, **kw,
                                    **self.ref_args(i)))
        return out


def chain(signs, L=1.0, speed=0.5, x0=0.0):
    """parts laid end to end along y = 0 from x0, each L long, part k driven at signs[k] * speed"""
    return [_line((x0 + k * L, 0.0), (x0 + (k + 1) * L, 0.0), s * speed) for k, s in enumerate(signs)]


FOLLOW = nr.FOLLOW_PATH
# name, mode, pose, parts (signs), window and options
TABLE = [
    ("fresh", FOLLOW, (0.3, 0.05, 0.1), (1, 1, 1), {}),
    ("extend", FOLLOW, (0.997, 0.02, 0.1), (1, 1, 1), dict(tail=1)),
    ("no_extend_sign", FOLLOW, (0.997, 0.02, 0.1), (1, -1, 1), dict(tail=1)),
    ("no_extend_frame", FOLLOW, (0.997, 0.02, 0.1), (1, 1, 1), dict(tail=1, frames=(0, 1, 1))),
    ("pop", FOLLOW, (1.4, 0.03, 0.05), (1, 1, 1), dict(tail=2, path_u=0.5)),
    ("end_of_mixed_window", FOLLOW, (2.3, 0.0, 0.1), (1, -1), dict(tail=2)),
    ("real_lengths", FOLLOW, (0.3, 0.02, 0.0), (1, 1, 1, 1), dict(lengths=(2.0, 2.0, 2.0, 2.0))),
    ("arrived_last", FOLLOW, (0.994, 0.0, 0.0), (1,), dict(tail=1)),
    ("next_part_sign", FOLLOW, (0.994, 0.0, 0.0), (1, -1, 1), dict(tail=1, reset=1)),
    ("next_part_same", FOLLOW, (0.994, 0.0, 0.0), (1, 1), dict(tail=1, reset=1)),
    ("off_path", FOLLOW, (1.4, 0.7, 0.0), (1, 1, 1), dict(tail=2)),
    ("no_parts", FOLLOW, (0.3, 0.0, 0.0), (1, 1), dict(npart=0, head=3, tail=5, path_u=0.25)),
    ("head_past_npart", FOLLOW, (0.3, 0.0, 0.0), (1, 1), dict(head=5, tail=7, path_u=0.25)),
    ("tail_before_head", FOLLOW, (1.5, 0.02, 0.0), (1, 1, 1), dict(head=1, tail=0)),
    ("npart_past_stride", FOLLOW, (4.5, 0.02, 0.0), (1, 1, 1, 1, 1, 1), dict(npart=9, head=4, tail=9)),
    ("reverse_part", FOLLOW, (0.5, 0.02, 3.1), (-1, 1), dict(tail=1)),
    ("negative_window", FOLLOW, (0.5, 0.02, 0.0), (1, 1), dict(npart=-3, head=-1, tail=-2)),
    ("idle", nr.IDLE, (0.3, 0.0, 0.0), (1, 1), dict(head=1, tail=1, path_u=0.75)),
    ("break", nr.BREAK, (0.3, 0.0, 0.0), (1, 1), dict(head=7, tail=-2, path_u=0.75)),
    ("error", nr.ERROR, (0.3, 0.0, 0.0), (1, 1), dict(head=1, tail=2, path_u=0.5)),
    ("goto", nr.GOTO_POSE, (0.3, 0.0, 0.0), (1, 1), dict(head=0, tail=1, path_u=0.125, goal=(0.8, 0.3, 0.4), reset=1)),
]
TABLE_ROW = {row[0]: k for k, row in enumerate(TABLE)}


def table_rows(B):
    """the table row of every robot of a fleet of B: all of them from B = 21 on, in an order that mixes the rows of a
    wave"""
    return [(i * 8) % len(TABLE) for i in range(B)]


def table_fleet(B, arrays):
    f = QFleet(B, arrays)
    for i, r in enumerate(table_rows(B)):
        _, mode, pose, signs, o = TABLE[r]
        f.mode[i], f.pose[i] = mode, pose
        f.set_parts(i, chain(signs), head=o.get("head", 0), tail=o.get("tail", 0), path_u=o.get("path_u", 0.0),
                    npart=o.get("npart"), frames=o.get("frames"), lengths=o.get("lengths"))
        f.reset[i] = o.get("reset", 0)
        if "goal" in o:
            f.goal[i] = o["goal"]
    f.vel[:, 0] = 0.1
    return f


def from_node_fleet(nf, one_part=False):
    """A tests/test_gpu_node.py Fleet as path sets. one_part: every path robot's set is its first segment, a new set
    (head = tail = 0). Else the robot's path follows a 1 m lead-in line that ends where the path starts, and the whole
    set is the active window [0, 1 + nseg) with nothing queued: the robots stand near the start of their paths, so
    most of them have the lead-in behind them."""
    f = QFleet(nf.B)
    f.mode[:], f.pose[:], f.vel[:], f.goal[:], f.reset[:] = nf.mode, nf.pose, nf.vel, nf.goal, nf.reset
    for i in range(nf.B):
        n = int(nf.nseg[i])
        recs = list(nf.segs[i, :n])
        if one_part:
            f.set_parts(i, recs[:1], path_u=nf.path_u[i])
        elif n < 1:
            f.set_parts(i, [], path_u=nf.path_u[i])
        else:
            x0, y0, dx, dy = recs[0][0], recs[0][4], recs[0][1], recs[0][5]
            d = math.hypot(dx, dy)
            lead = _line((x0 - dx / d, y0 - dy / d), (x0, y0), 0.5)
            f.set_parts(i, [lead] + recs, head=0, tail=1 + n, path_u=nf.path_u[i])
    return f


def compact(f, head=None, tail=None):
    """(segs [B][S][16], nseg [B]): every robot's window [head, tail) moved to the front of its records"""
    head = f.head if head is None else head
    tail = f.tail if tail is None else tail
    segs = np.full((f.B, S, 16), np.nan)
    nseg = np.zeros(f.B, np.int32)
    for i in range(f.B):
        h, t = int(head[i]), int(tail[i])
        if 0 <= h < t <= S:
            segs[i, :t - h] = f.segs[i, h:t]
            nseg[i] = t - h
    return segs, nseg


def mission_fleet(omni4):
    """The closed-loop mission: 48 robots, N = 8. Robots 0-15 carry a forward / reverse / forward set of short lines
    (7 to 13 cm out, back past the start by a third of that, and out again: from the 5 cm at which a part counts as
    done the next part's end is up to 12 cm away), robots 16-31 a two-part
    forward set: 16-23 with the parts' real lengths, so that the window spans both and the first part is popped on
    the way, 24-31 with the node's 1000 per part, so that the second part waits in the queue until the first ends.
    Robots 32-47 are Idle. Arrival is within 5 cm and (signed) 0.2 rad, as tests/test_gpu_node.py's closed loop."""
    B = 48
    f = QFleet(B, arrays=True)
    rng = np.random.default_rng(23)
    for i in range(B):
        x, y, th = rng.uniform(-2, 2), rng.uniform(-2, 2), rng.uniform(-math.pi, math.pi)
        hold = th + 1.2 if omni4 else th  # the heading the robot holds
        f.pose[i] = (x, y, hold)
        c, s_ = math.cos(th), math.sin(th)
        L = 0.07 + 0.004 * (i % 16)
        at = lambda d: (x + d * c, y + d * s_)  # noqa: E731
        if i < 16:
            f.mode[i] = FOLLOW
            f.set_parts(i, [_line(at(0), at(L), 0.5, hold, hold), _line(at(L), at(-0.3 * L), -0.5, hold, hold),
                            _line(at(-0.3 * L), at(0.9 * L), 0.5, hold, hold)])
        elif i < 32:
            f.mode[i] = FOLLOW
            f.set_parts(i, [_line(at(0), at(L), 0.5, hold, hold), _line(at(L), at(2 * L), 0.5, hold, hold)],
                        lengths=(L, L) if i < 24 else None)
    f.reset[:] = 1
    return f
