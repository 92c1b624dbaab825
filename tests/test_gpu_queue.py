"""GPU tests of nmpc_batch_node_tick_queue (the Queue instantiations of csrc/node_gate.hip) against tests/queue_ref.py,
the fp64 restatement of NMPCNavControlROS's path-set bookkeeping, and against nmpc_batch_node_tick on the parts.

What is exact and why: queue_ref is given the device's search result on the window it opens (nmpc_path_nearest on a
compacted copy of that window, from the same path_u: the search the gate is specified to run), so head, tail, mode,
event, path_u (U - k is exact), remains (r - path_u is exact), the position error (nmpc_path_nearest's own) and the
heading error (additions and an exact fmod of nmpc_path_nearest's near heading) are compared bit for bit. The device's
search itself is held to tests/test_gpu_path_nearest.py's bars against the oracle's own search (the distance within
[d - 1e-12, d + 1e-9] m, the errors to 1e-12). queue_ref refuses scenarios within 1e-9 of a threshold, and
tests/test_queue_ref.py shows on the CPU that the scenarios here are clear of them.
"""
import math

import numpy as np
import pytest
import torch

from nmpc_nav_control_amd._lib import default_params
from nmpc_nav_control_amd.batch import BatchSolver, NodeParams
from nmpc_nav_control_amd.path import PathQueue, discretize, nearest
from tests import node_ref as nr
from tests import queue_cases as qc
from tests import queue_ref as qr
from tests.path_nearest_ref import dist_at, nearest_one
from tests.test_gpu_node import NU, Tick, dev, mixed_fleet, params, state_of, warm_up
from tests.test_gpu_path_nearest import wrap_diff

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
N, S = qc.N, qc.S


class QTick:
    """Device copies of a QFleet (in a PathQueue) and the outputs of one queue tick."""

    def __init__(self, f, model="diff"):
        B = f.B
        self.B, self.f = B, f
        z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=DEV)  # noqa: E731
        q = PathQueue(B, S, device=DEV, frames=f.arrays, lengths=f.arrays, part_length=f.q["part_length"],
                      max_active_len=f.q["max_active_len"])
        q.segs.copy_(dev(f.segs))
        q.npart.copy_(dev(f.npart))
        q.head.copy_(dev(f.head))
        q.tail.copy_(dev(f.tail))
        q.path_u.copy_(dev(f.path_u))
        if f.arrays:
            q.frame.copy_(dev(f.frame))
            q.length.copy_(dev(f.length))
        q.remains.fill_(7.0)
        self.queue = q
        self.mode, self.pose, self.vel, self.goal = dev(f.mode), dev(f.pose.T), dev(f.vel.T), dev(f.goal.T)
        self.reset = dev(f.reset)
        self.steer = z(B) if model == "tric" else None
        self.event, self.err = z(B, dt=torch.uint8), z(2, B, dt=torch.float64)
        self.traj, self.n = torch.full((N + 1, 3, B), 7.0, device=DEV), z(1, dt=torch.int32)
        self.cmd, self.u0, self.qp_res = z(3, B) + 5, z(NU[model], B) + 5, z(3, B) + 5
        self.status, self.qp_iter = z(B, dt=torch.int32) + 5, z(B, dt=torch.int32) + 5

    def run(self, solver, p):
        solver.node_tick_queue(NodeParams(**p), self.queue, self.mode, self.pose, self.vel, goal=self.goal,
                               steer=self.steer, reset=self.reset, event=self.event, err=self.err, traj_out=self.traj,
                               n_solved=self.n, cmd=self.cmd, u0=self.u0, status=self.status, qp_iter=self.qp_iter,
                               qp_res=self.qp_res)
        torch.cuda.synchronize()

    def outs(self):
        return dict(cmd=self.cmd, u0=self.u0, status=self.status, qp_iter=self.qp_iter, qp_res=self.qp_res)

    def window(self):
        q = self.queue
        return q.head.cpu().numpy(), q.tail.cpu().numpy(), q.path_u.cpu().numpy()


def same_bits(a, b):
    """equal to the bit, every NaN counting as the same value"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and \
        np.array_equal(a[~nan].view(np.uint64), b[~nan].view(np.uint64))


def device_search(f, omni4=False):
    """nmpc_path_nearest on a compacted copy of the window every FOLLOW_PATH robot's tick searches (steps 1 and 2 of
    the oracle), from its path_u: per robot None or (U, near [4], pos_err); and the windows"""
    wins = f.open_windows()
    segs, nseg = qc.compact(f, [w[1] for w in wins], [w[2] for w in wins])
    near = torch.empty((4, f.B), dtype=torch.float64, device=DEV)
    err = torch.empty((2, f.B), dtype=torch.float64, device=DEV)
    rng = torch.stack([dev(f.path_u), torch.full((f.B,), math.nan, dtype=torch.float64, device=DEV)])
    U = nearest(dev(segs), dev(nseg), dev(f.pose.T), u_range=rng, holonomic_heading=omni4, near=near, err=err)
    torch.cuda.synchronize()
    U, near, err = U.cpu().numpy(), near.cpu().numpy(), err.cpu().numpy()
    return [None if nseg[i] < 1 else (U[i], near[:, i], err[0, i]) for i in range(f.B)], wins, segs, nseg


def check_tick(t, p, omni4=False):
    """everything one queue tick wrote, against queue_ref on the device's search"""
    f, B = t.f, t.B
    search, wins, wsegs, wnseg = device_search(f, omni4)
    status = t.status.cpu().numpy()
    ref = [qr.after_solve(r, status[i]) for i, r in enumerate(f.ref(p, omni4, search))]
    mode, ev = t.mode.cpu().numpy(), t.event.cpu().numpy()
    head, tail, path_u = t.window()
    remains, err, traj = t.queue.remains.cpu().numpy(), t.err.cpu().numpy(), t.traj.cpu().numpy()
    assert [int(v) for v in mode] == [r.mode for r in ref]
    assert [int(v) for v in ev] == [r.event for r in ref]
    assert [int(v) for v in head] == [int(r.head) for r in ref]
    assert [int(v) for v in tail] == [int(r.tail) for r in ref]
    for name, got, want in (("path_u", path_u, [r.path_u for r in ref]), ("remains", remains, [r.remains for r in ref]),
                            ("pos_err", err[0], [r.err[0] for r in ref]), ("ori_err", err[1], [r.err[1] for r in ref])):
        assert same_bits(got, want), (name, got, want)
    solves = np.array([r.solves for r in ref])
    assert int(t.n.cpu()) == solves.sum()
    # the search itself, and the errors in the oracle's own arithmetic
    own = f.ref(p, omni4, [None if s is None else (s[0], None, None) for s in search])
    for i in range(B):
        if search[i] is None:
            continue
        pose = f.pose[i].astype(np.float64)
        n = int(wnseg[i])
        _, dr, _, _ = nearest_one(wsegs[i], n, pose[:2], (f.path_u[i], math.nan))
        d = dist_at(wsegs[i:i + 1], wnseg[i:i + 1], np.array([search[i][0]]), pose[None, :2])[0]
        assert dr - 1e-12 <= d <= dr + 1e-9, (i, d - dr)
        assert abs(err[0, i] - own[i].err[0]) <= 1e-12 and wrap_diff(err[1, i], own[i].err[1]) <= 1e-12, i
    # the pending reset: consumed by the robots that solved, kept by the others (a hop to the next part included)
    assert (t.reset.cpu().numpy() == np.where(solves, 0, f.reset)).all()
    # outputs: zero and NaN poses for the robots that do not solve; the goal repeated; or the discretizer's poses on
    # the window the tick leaves behind, from the path_u it leaves behind
    for k, a in t.outs().items():
        assert (a.cpu().numpy()[..., ~solves] == 0).all(), k
    assert np.isnan(traj[:, :, ~solves]).all()
    for i in np.flatnonzero(solves):
        if ref[i].traj_len == 1:
            assert (traj[:, :, i] == f.goal[i][None, :]).all(), i
    pr = np.array([i for i in np.flatnonzero(solves) if ref[i].traj_len != 1], dtype=np.int64)
    if len(pr):
        csegs, cn = qc.compact(f, head, tail)
        want = discretize(dev(csegs[pr]), dev(cn[pr]), dev(path_u[pr]), p["sample_period"], N + 1,
                          bool(p["is_holonomic"]))
        torch.cuda.synchronize()
        assert np.array_equal(want.cpu().numpy(), traj[:, :, pr])
    return ref


# ---- 1. transition table --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arrays", [False, True], ids=["plain", "arrays"])
@pytest.mark.parametrize("B", [1, 5, 17, 65])
def test_transition_table(built, B, arrays):
    f, p = qc.table_fleet(B, arrays), params()
    t = QTick(f)
    t.run(BatchSolver("diff", N, B, device=DEV), p)
    ref = check_tick(t, p)
    rows = qc.table_rows(B)
    got = {qc.TABLE[r][0]: (i, ref[i]) for i, r in reversed(list(enumerate(rows)))}
    want = {  # name: (mode, event, head, tail); the two rows that read frame / length differ without the arrays
        "fresh": (nr.FOLLOW_PATH, nr.EV_SOLVED, 0, 1), "extend": (nr.FOLLOW_PATH, nr.EV_SOLVED, 0, 2),
        "no_extend_sign": (nr.FOLLOW_PATH, nr.EV_SOLVED, 0, 1),
        "no_extend_frame": (nr.FOLLOW_PATH, nr.EV_SOLVED, 0, 1 if arrays else 2),
        "pop": (nr.FOLLOW_PATH, nr.EV_SOLVED, 1, 2), "end_of_mixed_window": (nr.FOLLOW_PATH, nr.EV_SOLVED, 0, 2),
        "real_lengths": (nr.FOLLOW_PATH, nr.EV_SOLVED, 0, 3 if arrays else 1),
        "arrived_last": (nr.IDLE, nr.EV_ARRIVED, 0, 1), "next_part_sign": (nr.FOLLOW_PATH, qr.EV_NEXT_PART, 1, 2),
        "next_part_same": (nr.FOLLOW_PATH, qr.EV_NEXT_PART, 1, 2), "off_path": (nr.ERROR, nr.EV_OFF_PATH, 1, 2),
        "no_parts": (nr.IDLE, nr.EV_NONE, 3, 5), "head_past_npart": (nr.IDLE, nr.EV_NONE, 2, 2),
        "tail_before_head": (nr.FOLLOW_PATH, nr.EV_SOLVED, 1, 2), "npart_past_stride": (nr.FOLLOW_PATH, nr.EV_SOLVED, 4, 6),
        "reverse_part": (nr.FOLLOW_PATH, nr.EV_SOLVED, 0, 1), "negative_window": (nr.IDLE, nr.EV_NONE, -1, -2),
        "idle": (nr.IDLE, nr.EV_NONE, 1, 1), "break": (nr.IDLE, nr.EV_BREAK, 7, -2), "error": (nr.ERROR, nr.EV_NONE, 1, 2),
        "goto": (nr.GOTO_POSE, nr.EV_SOLVED, 0, 1),
    }
    head, tail, path_u = t.window()
    remains = t.queue.remains.cpu().numpy()
    for name, (i, r) in got.items():
        assert (int(t.mode[i]), int(t.event[i]), int(head[i]), int(tail[i])) == want[name], name
        if name in ("no_parts", "head_past_npart", "negative_window", "idle", "break", "error", "goto"):
            assert path_u[i] == f.path_u[i] and math.isnan(remains[i]), name  # (the progress keeps its bits)
        if name.startswith("next_part"):
            assert path_u[i] == 0.0 and int(t.reset[i]) == 1 and (t.cmd[:, i] == 0).all(), name
            assert remains[i] == f.npart[i] - 1
        if name == "end_of_mixed_window":
            assert path_u[i] == 2.0 and remains[i] == 0.0 and abs(float(t.err[1, i]) - 0.1) < 1e-6
    if B >= len(qc.TABLE):
        assert set(got) == set(want)


# ---- 2 / 3. against nmpc_batch_node_tick on the parts ---------------------------------------------------------------
def compare_with_plain(model, f, pf_segs, pf_nseg, p):
    """one queue tick of the fleet f on handle A against nmpc_batch_node_tick on handle R with the robots' windows as
    their paths (pf_segs, pf_nseg), both handles in the same warmed state: every output and every row of resident
    state, bit for bit. Returns the queue tick."""
    B = f.B
    nf = mixed_fleet(B)
    A, R = (BatchSolver(model, N, B, device=DEV) for _ in range(2))
    warm_up((A, R), nf, model)
    t = QTick(f, model)
    t.run(A, p)
    o = Tick(nf, model)
    o.segs, o.nseg, o.path_u = dev(pf_segs), dev(pf_nseg), dev(f.path_u)
    o.run(R, p)
    for k, a in t.outs().items():
        assert torch.equal(a, o.outs()[k]), k
    for name, a, b in (("mode", t.mode, o.mode), ("event", t.event, o.event), ("path_u", t.queue.path_u, o.path_u),
                       ("n", t.n, o.n), ("reset", t.reset, o.reset)):
        assert torch.equal(a, b), name
    assert same_bits(t.err.cpu().numpy(), o.err.cpu().numpy())
    assert same_bits(t.traj.cpu().numpy().astype(np.float64), o.traj.cpu().numpy().astype(np.float64))
    for k, (a, b) in enumerate(zip(state_of(A), state_of(R))):
        assert torch.equal(a, b), k
    assert 0 < int(t.n.cpu()) < B
    return t


@pytest.mark.parametrize("model,B", [("diff", 5), ("diff", 17), ("diff", 65), ("omni4", 65), ("tric", 65)])
def test_unchanged_window_equals_the_plain_tick(built, model, B):
    """A mixed fleet whose path robots hold a lead-in line and their path as the window, nothing queued. A first tick
    (on a handle of its own) pops the parts behind each robot; from there the windows are stable, and the compared
    tick must be nmpc_batch_node_tick on a compacted copy of each window, bit for bit."""
    p = params()
    omni4 = model == "omni4"
    f = qc.from_node_fleet(mixed_fleet(B))
    first = QTick(f, model)
    first.run(BatchSolver(model, N, B, device=DEV), p)
    check_tick(first, p, omni4)  # (a tick that changes windows: its poses come from the final windows)
    head, tail, path_u = first.window()
    assert (head != f.head).any()
    g = qc.from_node_fleet(mixed_fleet(B))
    g.head[:], g.tail[:], g.path_u[:] = head, tail, path_u
    segs, nseg = qc.compact(g)
    t = compare_with_plain(model, g, segs, nseg, p)
    h2, t2, _ = t.window()
    assert (h2 == head).all() and (t2 == tail).all()
    follow = torch.from_numpy(g.mode == nr.FOLLOW_PATH).to(DEV)
    assert torch.isnan(t.queue.remains[~follow | (t.mode != nr.FOLLOW_PATH)]).all()
    still = (follow & (t.mode == nr.FOLLOW_PATH)).cpu().numpy()
    assert still.any() and same_bits(t.queue.remains.cpu().numpy()[still],
                                     (g.npart - h2)[still] - t.queue.path_u.cpu().numpy()[still])


def test_one_part_sets_equal_the_plain_tick(built):
    """new one-part sets (head = tail = 0) in a mixed fleet: the whole call is nmpc_batch_node_tick, and the robots in
    the other modes keep the bits of the window and the progress they were given"""
    B, p = 65, params()
    nf = mixed_fleet(B)
    f = qc.from_node_fleet(nf, one_part=True)
    other = f.mode != nr.FOLLOW_PATH
    f.head[other], f.tail[other], f.path_u[other] = 3, -7, 0.625
    segs, nseg = np.full((B, S, 16), np.nan), np.minimum(nf.nseg, 1).astype(np.int32)
    segs[:, 0] = f.segs[:, 0]
    t = compare_with_plain("diff", f, segs, nseg, p)
    head, tail, path_u = t.window()
    assert (head[other] == 3).all() and (tail[other] == -7).all() and (path_u[other] == 0.625).all()
    assert np.isnan(t.queue.remains.cpu().numpy()[other]).all()
    went = ~other & (nf.nseg >= 1)
    assert (head[went] == 0).all() and (tail[went] == 1).all()


# ---- 4. closed-loop mission -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["diff", "omni4"])
def test_closed_loop_mission(built, model):
    """tests/queue_cases.py's mission fleet on the harness plant (nmpc_fleet_sim_step). The host writes nothing
    between ticks but the plant step: at every tick mode, event, head and tail equal queue_ref on that tick's device
    poses, robots of both moving kinds finish every part of their sets (NEXT_PART at each queued part that a sign
    change or the 1000 m length kept out of the window, then ARRIVED -> Idle), and a finished robot's resident state
    stays frozen."""
    B, T = 48, 160
    omni4 = model == "omni4"
    p = params(final_pos_err=0.05, final_ori_err=0.2, is_holonomic=1 if omni4 else 0)
    f = qc.mission_fleet(omni4)
    prm = default_params(model, N)
    if omni4:  # (as tests/test_gpu_node.py's closed loop: the shipped pose weights move an omni4 2 mm in 27 ticks)
        for k in range(3):
            prm.W[k] *= 100.0
            prm.W_e[k] *= 100.0
    s = BatchSolver(model, N, B, params=prm, device=DEV)
    t = QTick(f, model)
    # the sets go in through the public call, as a fleet manager would hand them over
    q = PathQueue(B, S, device=DEV, frames=True, lengths=True)
    for i in np.flatnonzero(f.mode == nr.FOLLOW_PATH):
        n = int(f.npart[i])
        q.set_path_set(int(i), f.segs[i, :n], frames=f.frame[i, :n], lengths=f.length[i, :n])
    assert torch.equal(q.segs[:32], torch.nan_to_num(t.queue.segs[:32], nan=0.0)) and torch.equal(q.npart, t.queue.npart)
    t.queue = q
    hp = torch.zeros(6, B, device=DEV)
    hp[5] = -1.0  # (the harness's own references are not used)
    hs, htraj, hlen = torch.zeros(B, device=DEV), torch.zeros(N + 1, 3, B, device=DEV), torch.zeros(
        B, dtype=torch.int32, device=DEV)
    events = {i: [] for i in range(B)}
    frozen = {}
    for tick in range(T):
        f.mode = t.mode.cpu().numpy().copy()
        f.head, f.tail, f.path_u = (a.copy() for a in t.window())
        f.pose = t.pose.cpu().numpy().T.copy()
        ref = f.ref(p, omni4)
        t.run(s, p)
        status = t.status.cpu().numpy()
        ref = [qr.after_solve(r, status[i]) for i, r in enumerate(ref)]
        mode, ev = t.mode.cpu().numpy(), t.event.cpu().numpy()
        head, tail, _ = t.window()
        assert [int(v) for v in mode] == [r.mode for r in ref], tick
        assert [int(v) for v in ev] == [r.event for r in ref], tick
        assert [int(v) for v in head] == [int(r.head) for r in ref], tick
        assert [int(v) for v in tail] == [int(r.tail) for r in ref], tick
        st = [x.cpu().numpy() for x in state_of(s)]
        for i in range(B):
            if ev[i] not in (nr.EV_SOLVED, nr.EV_NONE):
                events[i].append((tick, int(ev[i])))
            if ev[i] == nr.EV_ARRIVED:
                frozen[i] = [x[:, i].copy() for x in st]
            elif i in frozen:
                assert mode[i] == nr.IDLE and ev[i] == nr.EV_NONE
                for x, y in zip(st, frozen[i]):
                    assert np.array_equal(x[:, i], y), (tick, i)
        s.fleet_sim_step(hp, hs, t.pose, t.vel, None, t.u0, t.status, htraj, hlen, advance=True)
    print("events (robot: [(tick, event)]):", {i: e for i, e in events.items() if e})
    head, tail, _ = t.window()
    kinds = [e[1] for e in events[0]], [e[1] for e in events[16]], [e[1] for e in events[24]]
    print("first robot of each kind:", kinds, "final modes:", t.mode.cpu().tolist())
    done = lambda i, hops: [e[1] for e in events[i]] == [qr.EV_NEXT_PART] * hops + [nr.EV_ARRIVED]  # noqa: E731
    mission = [i for i in range(16) if done(i, 2) and (head[i], tail[i]) == (2, 3)]
    spanned = [i for i in range(16, 24) if done(i, 0) and (head[i], tail[i]) == (1, 2)]
    queued = [i for i in range(24, 32) if done(i, 1) and (head[i], tail[i]) == (1, 2)]
    assert len(mission) >= 2 and len(spanned) + len(queued) >= 2 and spanned and queued
    moved = [i for i in mission if events[i][1][0] > events[i][0][0] + 1 and events[i][2][0] > events[i][1][0] + 1]
    assert moved, "no mission robot drove its reversing and its last part"
    assert (t.mode[32:] == nr.IDLE).all() and not any(events[i] for i in range(32, 48))
    assert all(e[1] in (qr.EV_NEXT_PART, nr.EV_ARRIVED) for i in range(B) for e in events[i])
