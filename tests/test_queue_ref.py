"""CPU checks of tests/queue_ref.py: against a literal model of the node's two std::list buffers, on hand-computed
cases, and on the scenarios of tests/test_gpu_queue.py, which must not sit on a tie."""
import math

import numpy as np
import pytest

from tests import node_ref as nr
from tests import queue_cases as qc
from tests import queue_ref as qr
from tests.path_cases import _line
from tests.path_nearest_ref import near_err, nearest_one, norm_ang
from tests.path_ref import PathDiscretizer, TPath

N = qc.N
P = dict(nr.DEFAULT)


class ListNode:
    """NMPCNavControlROS's FollowPath bookkeeping written as the reference writes it: two lists of parts, popped and
    pushed (processPathReceived :566-573, processPathBuffers :576-595, processNearestPoint :597-610, processFollowPath
    :648-698, pubControlStatus :374-375). A part is (record, frame, length)."""

    def __init__(self, p, q, parts, omni4=False):
        self.p, self.q, self.omni4 = p, q, omni4
        self.status = nr.FOLLOW_PATH
        self.upcoming = list(parts)  # :570 (the lengths are the caller's: :571 sets 1000)
        self.active = []
        self.u = 0.0
        self.process_path_buffers(0.0)  # :573

    def process_path_buffers(self, u):
        length = 0.0
        for k, part in enumerate(self.active):
            length += part[2] * (1 - u) if k == 0 else part[2]
        while length < self.q["max_active_len"] and len(self.upcoming) > 0:
            if len(self.active) > 0:
                a, b = self.active[-1], self.upcoming[0]
                if a[0][12] * b[0][12] < 0.0:
                    break
                if a[1] != b[1]:
                    break
            self.active.append(self.upcoming.pop(0))
            length += self.active[-1][2]

    def tick(self, pose):
        """one mainCycle in FollowPath; returns the event"""
        if not self.active:  # (the device's step 2: no active path, executeNMPC's empty list)
            self.status = nr.IDLE
            return nr.EV_NONE
        segs = np.array([a[0] for a in self.active])
        n = len(self.active)
        self.u = nearest_one(segs, n, (pose[0], pose[1]), (self.u, math.nan))[0]
        near, e = near_err(segs, n, self.u, pose, self.omni4)
        num = int(math.floor(self.u))
        if len(self.active) > num:
            for _ in range(num):
                self.active.pop(0)
                self.u = self.u - 1
        self.process_path_buffers(self.u)
        theta = near[2]
        if self.omni4:
            theta = near[3]
        elif self.active[0][0][12] < 0.0:
            theta += math.pi
        self.err = (float(e[0]), abs(norm_ang(theta - pose[2])))
        if self.p["enable_safe_conditions"] and (self.err[0] >= self.p["max_pos_err"] or
                                                 self.err[1] >= self.p["max_ori_err"]):
            self.status = nr.ERROR
            return nr.EV_OFF_PATH
        disc = PathDiscretizer(self.p["sample_period"], N + 1, bool(self.p["is_holonomic"]))
        poses, _ = disc.getNextNPoses([TPath(a[0]) for a in self.active], self.u)
        d = nr.dist(pose[0], pose[1], poses[-1][0], poses[-1][1])
        ang = norm_ang(pose[2] - poses[-1][2])
        if d <= self.p["final_pos_err"] and ang <= self.p["final_ori_err"]:
            if len(self.upcoming) == 0:
                self.status = nr.IDLE
                return nr.EV_ARRIVED
            self.active.pop(0)
            self.active.append(self.upcoming.pop(0))
            self.u = 0.0  # (the device's rule; the node leaves the old value until the next search)
            return qr.EV_NEXT_PART
        return nr.EV_SOLVED

    def remains(self):
        if self.status != nr.FOLLOW_PATH:
            return math.nan
        r = float(len(self.active) + len(self.upcoming))
        return r - self.u if r > 0 else r


def random_set(rng):
    """1 to 6 parts end to end, mixed signs and frames, lengths of their own"""
    n = int(rng.integers(1, 7))
    p = rng.uniform(-1, 1, 2)
    h = rng.uniform(-math.pi, math.pi)
    recs, frames, lengths = [], [], []
    sign, frame = 1.0, 0
    for _ in range(n):
        L = rng.uniform(0.05, 3.0)
        if rng.uniform() < 0.35:
            sign = -sign
        if rng.uniform() < 0.2:
            frame += 1
        q = p + L * np.array([math.cos(h), math.sin(h)])
        recs.append(_line(p, q, sign * rng.uniform(0.2, 0.8)))
        frames.append(frame)
        lengths.append(L)
        p, h = q, h + rng.uniform(-0.6, 0.6)
    return recs, frames, lengths


@pytest.mark.parametrize("real_lengths", [False, True])
def test_against_the_two_lists(real_lengths):
    """A robot teleported along random sets: after every tick the window [head, tail) over the part list holds
    exactly the list model's active parts and [tail, npart) its upcoming ones, with the same event, progress, errors
    and remainder."""
    rng = np.random.default_rng(5 + real_lengths)
    p = dict(P, final_pos_err=0.03, final_ori_err=0.3)
    q = dict(qr.QDEFAULT, max_active_len=rng.uniform(1.0, 6.0))
    events = set()
    for case in range(120):
        recs, frames, lengths = random_set(rng)
        if not real_lengths:
            lengths = [q["part_length"]] * len(recs)
        segs = np.array(recs)
        node = ListNode(p, q, list(zip(recs, frames, lengths)))
        head, tail, u, mode = 0, 0, 0.0, nr.FOLLOW_PATH
        where = 0.0  # the set's parameter the robot is put at
        for tick in range(12):
            where = min(where + rng.uniform(0.0, 0.9), float(len(recs)))
            k = min(int(where), len(recs) - 1)
            x, y = TPath(recs[k]).GetX(where - k), TPath(recs[k]).GetY(where - k)
            th = TPath(recs[k]).GetTheta(where - k) + (math.pi if recs[k][12] < 0 else 0.0)
            pose = np.array([x + rng.uniform(-0.02, 0.02), y + rng.uniform(-0.02, 0.02), th + rng.uniform(-0.1, 0.1)],
                            np.float32).astype(np.float64)
            try:
                t = qr.queue_ref(p, q, mode, pose, N, segs=segs, npart=len(recs), head=head, tail=tail, path_u=u,
                                 stride=len(recs), frames=frames, lengths=lengths)
            except nr.TieError:
                break
            ev = node.tick(pose)
            events.add(ev)
            assert (t.event, t.mode) == (ev, node.status), (case, tick)
            assert recs[t.head:t.tail] == [a[0] for a in node.active] or t.mode != nr.FOLLOW_PATH, (case, tick)
            if t.mode == nr.FOLLOW_PATH:
                assert len(recs) - t.tail == len(node.upcoming)
                assert t.path_u == node.u and t.err == node.err, (case, tick)
                assert t.remains == node.remains()
            else:
                assert math.isnan(t.remains)
                break
            head, tail, u, mode = t.head, t.tail, t.path_u, t.mode
    assert {nr.EV_SOLVED, nr.EV_ARRIVED, qr.EV_NEXT_PART} <= events


def test_hand_computed_windows():
    q = dict(qr.QDEFAULT)
    segs = np.array(qc.chain((1, 1, -1, 1)))
    # step 1
    assert qr.window(9, 4, 9, 6) == (6, 4, 6) and qr.window(2, 5, 7, 6) == (2, 2, 2)
    assert qr.window(3, 1, 0, 6) == (3, 1, 1) and qr.window(-3, -1, -2, 6) == (0, 0, 0)
    # fill: one part of 1000 is enough; 3 left of it takes the next same-sign part; the sign change stops it
    assert qr.fill(q, segs, None, None, 0, 0, 4, 0.0) == 1
    assert qr.fill(q, segs, None, None, 0, 1, 4, 0.997) == 2
    assert qr.fill(q, segs, None, None, 1, 2, 4, 0.999) == 2
    assert qr.fill(q, segs, [0, 1, 1, 1], None, 0, 1, 4, 0.997) == 1
    # real lengths: 2 + 2 + 2 reaches 5 after three parts, were it not for the sign change behind the second
    assert qr.fill(q, segs, None, [2.0] * 4, 0, 0, 4, 0.0) == 2
    assert qr.fill(q, np.array(qc.chain((1, 1, 1, 1))), None, [2.0] * 4, 0, 0, 4, 0.0) == 3
    # remains
    assert qr.remains_of(3, 1, 0.25) == 1.75 and qr.remains_of(2, 2, 0.5) == 0.0


def test_table_rows_by_hand():
    """the rows of the GPU transition table, through the oracle's own search"""
    f = qc.table_fleet(len(qc.TABLE) * 8, arrays=True)
    rows = qc.table_rows(f.B)
    ref = f.ref(P)
    got = {}
    for i, r in enumerate(rows):
        got.setdefault(qc.TABLE[r][0], ref[i])
    want = {  # name: (mode, event, head, tail)
        "fresh": (nr.FOLLOW_PATH, nr.EV_SOLVED, 0, 1), "extend": (nr.FOLLOW_PATH, nr.EV_SOLVED, 0, 2),
        "no_extend_sign": (nr.FOLLOW_PATH, nr.EV_SOLVED, 0, 1), "no_extend_frame": (nr.FOLLOW_PATH, nr.EV_SOLVED, 0, 1),
        "pop": (nr.FOLLOW_PATH, nr.EV_SOLVED, 1, 2), "end_of_mixed_window": (nr.FOLLOW_PATH, nr.EV_SOLVED, 0, 2),
        "real_lengths": (nr.FOLLOW_PATH, nr.EV_SOLVED, 0, 3), "arrived_last": (nr.IDLE, nr.EV_ARRIVED, 0, 1),
        "next_part_sign": (nr.FOLLOW_PATH, qr.EV_NEXT_PART, 1, 2), "next_part_same": (nr.FOLLOW_PATH, qr.EV_NEXT_PART, 1, 2),
        "off_path": (nr.ERROR, nr.EV_OFF_PATH, 1, 2), "no_parts": (nr.IDLE, nr.EV_NONE, 3, 5),
        "head_past_npart": (nr.IDLE, nr.EV_NONE, 2, 2), "tail_before_head": (nr.FOLLOW_PATH, nr.EV_SOLVED, 1, 2),
        "npart_past_stride": (nr.FOLLOW_PATH, nr.EV_SOLVED, 4, 6), "reverse_part": (nr.FOLLOW_PATH, nr.EV_SOLVED, 0, 1),
        "negative_window": (nr.IDLE, nr.EV_NONE, -1, -2), "idle": (nr.IDLE, nr.EV_NONE, 1, 1),
        "break": (nr.IDLE, nr.EV_BREAK, 7, -2), "error": (nr.ERROR, nr.EV_NONE, 1, 2),
        "goto": (nr.GOTO_POSE, nr.EV_SOLVED, 0, 1),
    }
    assert set(want) == set(got) == set(qc.TABLE_ROW)
    for name, w in want.items():
        t = got[name]
        assert (t.mode, t.event, t.head, t.tail) == w, name
    assert got["pop"].path_u == pytest.approx(0.4, abs=1e-6) and got["pop"].remains == pytest.approx(1.6, abs=1e-6)
    assert got["end_of_mixed_window"].path_u == 2.0 and got["end_of_mixed_window"].remains == 0.0
    assert got["end_of_mixed_window"].err[1] == pytest.approx(0.1, abs=1e-6)  # the front part drives forwards
    assert got["next_part_sign"].path_u == 0.0 and got["next_part_sign"].remains == 2.0
    assert got["no_parts"].path_u == 0.25 and got["head_past_npart"].path_u == 0.25
    assert math.isnan(got["arrived_last"].remains) and math.isnan(got["off_path"].remains)
    assert got["off_path"].path_u == pytest.approx(0.4, abs=1e-6)
    # without the frame and length arrays: the frame row extends, the real-lengths row takes one part of 1000
    plain = dict(zip([qc.TABLE[r][0] for r in qc.table_rows(21)], qc.table_fleet(21, arrays=False).ref(P)))
    assert (plain["no_extend_frame"].tail, plain["real_lengths"].tail) == (2, 1)


@pytest.mark.parametrize("arrays", [False, True])
@pytest.mark.parametrize("B", [1, 5, 17, 65])
def test_gpu_table_has_no_tie(B, arrays):
    qc.table_fleet(B, arrays).ref(P)  # raises TieError on a tie


@pytest.mark.parametrize("one_part", [False, True])
@pytest.mark.parametrize("B", [5, 17, 65])
def test_gpu_mixed_fleets_have_no_tie(B, one_part):
    from tests.test_gpu_node import mixed_fleet
    for omni4 in (False, True):
        qc.from_node_fleet(mixed_fleet(B), one_part).ref(P, omni4)


def test_mission_starts_clear_of_ties():
    """(the closed loop's later ticks depend on the plant: test_gpu_queue.py's oracle raises there if one ties)"""
    for omni4 in (False, True):
        f = qc.mission_fleet(omni4)
        ref = f.ref(dict(P, final_pos_err=0.05, final_ori_err=0.2, is_holonomic=int(omni4)), omni4)
        assert [t.event for t in ref[:32]] == [nr.EV_SOLVED] * 32
        assert [(t.head, t.tail) for t in ref[:16]] == [(0, 1)] * 16
        assert [(t.head, t.tail) for t in ref[16:32]] == [(0, 2)] * 8 + [(0, 1)] * 8


def test_a_tie_is_refused():
    q = dict(qr.QDEFAULT)
    segs = np.array(qc.chain((1, 1)))
    with pytest.raises(nr.TieError):
        qr.fill(q, segs, None, None, 0, 1, 2, 0.995)  # L = 5 exactly
    zero = segs.copy()
    zero[1][12] = 0.0
    with pytest.raises(nr.TieError):
        qr.fill(q, zero, None, None, 0, 1, 2, 0.999)
    assert qr.fill(q, zero, None, None, 0, 1, 2, 0.5) == 1  # (the product is not looked at: L is long enough)
