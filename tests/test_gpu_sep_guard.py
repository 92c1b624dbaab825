"""The separation guard on the device (-m gpu): the guarded writer and the hold (csrc/separation.hip,
nmpc_batch_stage_limits_from_tracks_ex, nmpc_batch_sep_hold) against tests/sep_guard_ref.py, the guard form without
priorities and without a hold against the existing writer, and nmpc_batch_node_cycle with a guard attached on the
head-on pair and the crossing of tests/sep_guard_cases.py.

Tolerances. vlim, gap, gap_all and held are compared with the restatement bit for bit (the same fp32 and fp64
operations in the same order, compiled without contraction; min is exact, so the tiles, the chunks, the cull and the
second accumulator cannot show) and stage tables handle to handle, byte for byte. The cycle's closed loop is held to
the bar of tests/test_gpu_separation.py's convoy: |u0 - reference| <= 1e-3 with every status 0, the reference being
tests/stage_bound_cases.py:solve_spliced on the device's own inputs and the restatement's limits; modes, events and held
are the restatement's on the device's own state, tick by tick; the resident rows of a held robot are compared byte for
byte before and after the cycle.

Shapes: B = 16 robots on a handle of capacity 24; N = 20 with M = 15, 16, 17 (the edges of a chunk of 16 tracks; no own
tracks, own_priority given) and M = 33 (three chunks, the own tracks at 5..20, own_priority NULL); N = 48 and 49 with
M = 17 (the edge of the tile of 48 stages: the second minimum through a second pass); hold_stages 0, 4, N and N + 5.

The plant of the cycle's loop: a robot that solved steps on the harness plant (nmpc_fleet_sim_step on its u0); a robot
that got the stop command steps as in tests/sep_guard_cases.py:stop_step (the harness plant integrates u0 from the
carried refs and has no stop command). A robot in IDLE is skipped by the input stage, so the cycle exports it at the
pose the stage last gave it; the reference does the same.

What "byte for byte" covers for a held robot: its columns of the iterate, the carried refs and the warm flags, its
reset flag and, with a queue, head, tail, path_u and remains, on every tick; the scratch records whole on the ticks
on which nobody solves (both robots of the head-on pair are held for 50 ticks). On a tick on which another robot
solves the records are not compared: their layout is the kernels' and the other robot's slots change. The placement
key is not read by this file: the handles here run with the schedule off, and the key is written by the solve launch's
sort for the robots that solve.

Measured (MI355X, diff): head-on through the cycle, plain tick and queue alike: held from tick 148, smallest centre
distance 0.4453 m, |u0 - reference| at most 5.4e-6. Held on a path: from tick 310 at x = 0.7521 with head 1, path_u
0.4918, remains 2.5082; 60 ticks after the release remains 2.0474; |u0 - reference| at most 6.8e-5."""
import numpy as np
import pytest
import torch

from nmpc_nav_control_amd import _lib
from nmpc_nav_control_amd.batch import BatchSolver, NodeInput, NodeParams, SepGuard, Tracks
from nmpc_nav_control_amd.path import PathQueue
from oracle.oracle import Oracle
from tests import node_input_ref as nr
from tests import sep_guard_cases as gc
from tests import sep_guard_ref as gr
from tests import separation_ref as sp
from tests import speed_map_cases as mc
from tests import stage_bound_cases as sc
from tests.table_harness import DEV, MODELS, TOL_U, t
from tests.test_gpu_node_input import DEPTH, MS, NOW, host, u8
from tests.test_gpu_separation import RULE, SEP, FleetLoop, place_classes, scene
from tests.test_gpu_speed_map import BASE, bits, dev_map, table_bytes

pytestmark = pytest.mark.gpu
F64, I64, U8, I32 = torch.float64, torch.int64, torch.uint8, torch.int32
F32 = np.float32


def set_held(s, held):
    h = np.zeros(s.capacity, np.uint8)
    h[:len(held)] = held
    s.sep_state().copy_from(u8(h)[None])


def get_held(s, B):
    torch.cuda.synchronize()
    return host(s.sep_state().to_tensor())[0, :B]


# ---- 1. the guarded writer and the hold against the restatement ----------------------------------------------------
def guard_case(model, N, M, own_first, frames, with_map, ahead_only, seed, B=16, cap=24, K=None):
    rng = np.random.default_rng(seed)
    K = N if K is None else K
    s, twin = (BatchSolver(model, N, cap, device=DEV) for _ in range(2))
    nx, nbx = s.nx, s.nbx
    at = np.array(BASE if frames else (0.0, 0.0))
    m = mc.map_b(tuple(at)) if with_map else None
    q, pose, xy = scene(N, B, cap, M, K, rng, spread=1.5)
    origin = None
    if frames:
        jit = rng.integers(-2, 3, (2, cap)).astype(np.float64)
        origin = at[:, None] + jit
        q = q - jit[None]
        pose[:2] -= jit[:, :B]
        for h in (s, twin):
            h.set_robot_frame(t(origin, F64))
    xbar = rng.uniform(-2, 2, ((N + 1) * nx, cap)).astype(F32)
    xbar.reshape(N + 1, nx, cap)[:, :2] = q.astype(F32)
    carried = rng.uniform(-0.6, 0.6, (nbx, cap)).astype(F32)
    for h in (s, twin):
        h.state()[0].copy_from(t(xbar))
        h.state()[2].copy_from(t(carried))
    o = Oracle(model, N, rule="batched")
    cap_v, acc = F32(o.prm.ubx[0]), F32(o.prm.ubu[0])
    reset = (np.arange(B) % 5 == 0).astype(np.uint8)
    held = (np.arange(B) % 3 == 1).astype(np.uint8)  # (robot 10 is both)
    mask = np.ones(B, np.uint8)
    mask[[3, 11]] = 0
    mode = np.full(B, nr.GOTO_POSE, np.uint8)
    mode[[6, 7, 13]] = (nr.IDLE, nr.FOLLOW_PATH, nr.ERROR)
    pose32 = pose.astype(F32)
    org_b = None if origin is None else origin[:, :B]
    pos, _ = gr.positions(xbar, nx, N, B, pose32, reset, held)
    xy = xy + at[None, :, None]
    place_classes(xy, pos[0].astype(np.float64) + (0 if org_b is None else org_b), B, own_first)
    if own_first >= 0:
        gr.export(xy, own_first, xbar, nx, N, B, org_b, pose32, reset=reset, held=held)
    # priorities with ties, both ends of the range, and most tracks near the robots' own
    pr = rng.integers(-2, 3, M).astype(np.int32)
    pr[rng.integers(0, M, 2)] = gr.INT_MAX
    pr[rng.integers(0, M, 2)] = gr.INT_MIN
    own_pr = None
    if own_first < 0:
        own_pr = rng.integers(-2, 3, B).astype(np.int32)
        own_pr[[2, 9]] = (gr.INT_MIN, gr.INT_MAX)
    sep = dict(SEP, ahead_only=ahead_only)
    want, want_gap, want_all = gr.limits(xbar, nx, N, B, xy, cap_v, acc, o.prm.dt, carried[:, :B],
                                         sc.speed_rows(model, nbx), pose=pose32, reset=reset, held=held, m=m,
                                         origin=org_b, own_first=own_first, priority=pr, own_priority=own_pr, **sep,
                                         **RULE)
    set_held(s, held)
    vlim, gap, gap_all = (torch.full((N + 1, B), 7.0, device=DEV) for _ in range(3))
    g = dict(stop_gap=0.5, release_gap=0.9)
    G = SepGuard(t(pr, I32), None if own_pr is None else t(own_pr, I32), **g)
    before = [v.to_tensor() for v in s.state()]
    tr = Tracks(t(xy, F64), own_first=own_first)
    s.stage_limits_from_tracks(tr, map=dev_map(m) if m else None, pose=t(pose32), reset=u8(reset), mask=u8(mask),
                               vlim=vlim, gap=gap, gap_all=gap_all, guard=G, **sep, **RULE)
    torch.cuda.synchronize()
    on = mask.astype(bool)
    for name, got, ref in (("gap_all", host(gap_all), want_all), ("gap", host(gap), want_gap), ("vlim", host(vlim), want)):
        assert np.array_equal(bits(got[:, on]), bits(ref[:, on])), (name, np.argwhere(bits(got[:, on]) != bits(ref[:, on]))[:8])
        assert (got[:, ~on] == 7.0).all(), name
    for x, y in zip(before, [v.to_tensor() for v in s.state()]):
        assert torch.equal(x, y)  # the writer reads the resident state
    assert np.array_equal(get_held(s, B), held)  # ... and the hold's
    ref_full = np.where(on[None, :], want, F32(7.0)).astype(F32)
    twin.set_stage_limits(v_max=t(ref_full), mask=u8(mask))
    assert torch.equal(table_bytes(s), table_bytes(twin))
    # the hold, on the processed robots' planes (the two masked robots: IDLE, so their stale planes are not read)
    mode_h = mode.copy()
    mode_h[~on] = nr.IDLE
    seen = set()
    for hs in (0, 4, N, N + 5):
        for md, rs in ((mode_h, reset), (None if on.all() else mode_h, None)):
            set_held(s, held)
            out = torch.full((B,), 7, dtype=U8, device=DEV)
            Gh = SepGuard(hold_stages=hs, **g)
            s.sep_hold(Gh, mode=None if md is None else u8(md), reset=None if rs is None else u8(rs), held_out=out)
            ref = gr.hold(want_all, held, rs, md, hold_stages=hs, **g)
            assert np.array_equal(get_held(s, B), ref) and np.array_equal(host(out), ref), (hs, rs is None)
            seen.update(zip(held.tolist(), ref.tolist()))
    assert seen == {(0, 0), (0, 1), (1, 0), (1, 1)}, seen  # taken, kept, released and left alone
    set_held(s, held)
    s.sep_hold(SepGuard(hold=0, **g))
    assert not get_held(s, B).any()
    # the scene is what it says: the filter removes something, not everything
    fin_y = np.isfinite(want_gap[:, on])
    assert fin_y.any() and (want_gap[:, on][fin_y] > want_all[:, on][fin_y]).any()
    assert np.isnan(xy).any()
    # a held robot stands and keeps its direction, a reset one has none
    only_held = np.flatnonzero(held.astype(bool) & ~reset.astype(bool) & on)
    posr, h = gr.positions(xbar, nx, N, B, pose32, reset, held)
    assert (posr[:, :, only_held] == pose32[None, :2, only_held]).all() and (h[:, :, only_held] != 0).any()


CHUNK = [(mdl, M) for mdl in MODELS for M in (15, 16, 17, 33)]


@pytest.mark.parametrize("model,M", CHUNK)
def test_guarded_writer_bit_for_bit(built, model, M):
    j = CHUNK.index((model, M))
    # frames at UTM-sized origins for omni4, a map for tric, ahead_only off for every other case
    guard_case(model, 20, M, 5 if M == 33 else -1, frames=model == "omni4", with_map=model == "tric",
               ahead_only=1 - j % 2, seed=81 + j)


@pytest.mark.parametrize("N", [48, 49])
def test_guarded_writer_at_the_tile_edge(built, N):
    guard_case("diff", N, 17, -1, frames=True, with_map=False, ahead_only=1, seed=95 + N, K=25)


def test_cull_with_priorities(built):
    """tests/test_gpu_separation.py:test_cull_is_invisible's ring at UTM-sized coordinates with priorities: sixteen
    tracks on a ring at range (1 +- 2^-20) around the standing robot 0 and nothing else in range of it. Case 1: every
    ring track yields to robot 0 (qy = +inf, qa finite). Case 2: only ring track 5, just inside range and kept by a
    box test that is all but an equality, has right of way: the filtered minimum comes from it alone."""
    N, B, M, rg = 20, 16, 512, 3.0
    rng = np.random.default_rng(61)
    s = BatchSolver("diff", N, B, device=DEV)
    k = np.arange(N + 1)
    start = rng.uniform(-300, 300, (2, B))
    th = rng.uniform(-np.pi, np.pi, B)
    pm = start[None] + 0.1 * k[:, None, None] * np.stack([np.cos(th), np.sin(th)])[None] + np.array(BASE)[None, :, None]
    origin = np.round(pm[0]) + rng.integers(-3, 4, (2, B))
    q = (pm - origin[None]).astype(F32)
    xbar = rng.uniform(-2, 2, ((N + 1) * s.nx, B)).astype(F32)
    xbar.reshape(N + 1, s.nx, B)[:, :2] = q
    s.set_robot_frame(t(origin, F64))
    s.state()[0].copy_from(t(xbar))
    pose = np.zeros((3, B), F32)
    pose[:2] = q[0]
    reset = np.zeros(B, np.uint8)
    reset[0] = 1
    xy = rng.uniform(-500, 500, (2, M))[None] + k[:, None, None] * rng.uniform(-0.1, 0.1, (2, M))[None]
    xy = xy + np.array(BASE)[None, :, None]
    X0 = q[0, :, 0].astype(np.float64) + origin[:, 0]
    far = np.hypot(*(xy[0] - X0[:, None])) < 20  # (nothing else near robot 0)
    xy[:, :, far] += 1000.0
    ang = 2 * np.pi * np.arange(16) / 16 + 0.1
    rad = rg * (1 + np.where(np.arange(16) % 2 == 0, 1.0, -1.0) * 2.0 ** -20)
    xy[:, :, 16:32] = (X0[:, None] + rad[None] * np.stack([np.cos(ang), np.sin(ang)]))[None]
    o = Oracle("diff", N, rule="batched")
    car = host(s.state()[2].to_tensor())[:, :B]
    own_pr = np.zeros(B, np.int32)
    own_pr[0] = 10
    for case, pr_ring in ((1, np.full(16, 9)), (2, np.where(np.arange(16) == 5, 10, 9))):
        pr = rng.integers(-3, 4, M).astype(np.int32)
        pr[16:32] = pr_ring
        want, want_gap, want_all = gr.limits(xbar, s.nx, N, B, xy, F32(o.prm.ubx[0]), F32(o.prm.ubu[0]), o.prm.dt, car,
                                             s.nbx, pose=pose, reset=reset, origin=origin, range=rg, priority=pr,
                                             own_priority=own_pr)
        vlim, gap, gap_all = (torch.zeros(N + 1, B, device=DEV) for _ in range(3))
        G = SepGuard(t(pr, I32), t(own_pr, I32))
        s.stage_limits_from_tracks(Tracks(t(xy, F64)), pose=t(pose), reset=u8(reset), vlim=vlim, gap=gap,
                                   gap_all=gap_all, range=rg, guard=G)
        torch.cuda.synchronize()
        for got, ref in ((gap_all, want_all), (gap, want_gap), (vlim, want)):
            assert np.array_equal(bits(host(got)), bits(ref)), case
        assert np.isfinite(want_all[:, 0]).all()
        if case == 1:
            assert np.isposinf(want_gap[:, 0]).all()
        else:
            pos, h = gr.positions(xbar, s.nx, N, B, pose, reset)
            qq, counts = sp.pairs(pos, h, xy, origin=origin, range=rg)
            assert counts[0, 0, 16 + 5] and (want_gap[:, 0] == np.sqrt(qq[:, 0, 16 + 5])).all()
            cull = sp.cull_counts(pos, xy, origin=origin, range=rg)
            assert cull["mask"][0, 16 + 5] and qq[0, 0, 16 + 5] > F32(rg * rg) * F32(1 - 2.0 ** -18)


# ---- 2. the guard form with nothing to do is the existing writer ---------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
def test_guard_without_priorities_or_hold_is_the_writer(built, model):
    N, B, cap, M = 20, 21, 24, 37
    rng = np.random.default_rng(111)
    a, b = (BatchSolver(model, N, cap, device=DEV) for _ in range(2))
    q, pose, xy = scene(N, B, cap, M, N, rng)
    xbar = rng.uniform(-2, 2, ((N + 1) * a.nx, cap)).astype(F32)
    xbar.reshape(N + 1, a.nx, cap)[:, :2] = q.astype(F32)
    carried = rng.uniform(-0.6, 0.6, (a.nbx, cap)).astype(F32)
    for h in (a, b):
        h.state()[0].copy_from(t(xbar))
        h.state()[2].copy_from(t(carried))
    reset, mask = u8(np.arange(B) % 5 == 0), u8(np.arange(B) % 7 != 3)
    tr = Tracks(t(xy, F64), own_first=5)
    dm = dev_map(mc.map_b())
    out = [[torch.full((N + 1, B), 7.0, device=DEV) for _ in range(3)] for _ in range(2)]
    kw = dict(map=dm, pose=t(pose.astype(F32)), reset=reset, mask=mask, **SEP, **RULE)
    a.stage_limits_from_tracks(tr, vlim=out[0][0], gap=out[0][1], **kw)
    b.stage_limits_from_tracks(tr, vlim=out[1][0], gap=out[1][1], gap_all=out[1][2], guard=SepGuard(hold=0), **kw)
    assert torch.equal(table_bytes(a), table_bytes(b))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1]) and torch.equal(out[1][1], out[1][2])
    b.sep_hold(SepGuard(hold=0))
    assert not get_held(b, B).any()


# ---- 3. the cycle --------------------------------------------------------------------------------------------------
class CycleLoop:
    """nmpc_batch_node_cycle on a fleet dict of tests/sep_guard_cases.py, every robot in GOTO_POSE, with the handle's
    own robots as the tracks (export_own) and the guard attached; per tick the restatement's limits and hold on the
    device's own state, the spliced fp64 reference for the robots that solve, and the plants."""

    def __init__(self, model, fl, guard=True, priority=None, queue=False, tracks=True, follow=None, extra=None):
        """follow {robot: [PathSegment, ...]}: those robots are in FOLLOW_PATH on a path set in the queue; extra [2][E]:
        standing obstacles, the tracks behind the handle's own"""
        self.model, self.B = model, fl["pose"].shape[1]
        B, N = self.B, gc.N
        s = self.s = BatchSolver(model, N, B, device=DEV)
        s.set_schedule("off")
        self.loop = FleetLoop(s, model, fl)
        self.fleet = sc.StageFleet([Oracle(model, N, rule="batched") for _ in range(B)], fl["carried"].T)
        self.o = self.fleet.os[0]
        s.enable_input(DEPTH)
        self.goal = fl["path"][:3].astype(np.float64).copy()  # [3][B]
        self.mode, self.reset = u8(np.full(B, nr.GOTO_POSE)), u8(np.ones(B))
        self.extra = np.zeros((2, 0)) if extra is None else np.array(extra, np.float64)
        self.xy = torch.zeros(N + 1, 2, B + self.extra.shape[1], dtype=F64, device=DEV)
        self.set_extra(self.extra)
        self.priority = priority
        self.guarded = guard and tracks
        if tracks:
            s.set_tracks(Tracks(self.xy, own_first=0), export_own=True, **gc.RULE)
        if guard:
            s.set_sep_guard(SepGuard(None if priority is None else t(priority, I32), **gc.GUARD))
        self.tracks = tracks
        self.follow = np.zeros(B, bool)
        self.q = PathQueue(B, max([2] + [len(v) for v in (follow or {}).values()]), device=DEV) if queue else None
        if queue:
            self.q.remains.fill_(5.0)
        for i, parts in (follow or {}).items():  # (as the node's path callback: the set, the mode, the reset flag)
            self.q.set_path_set(i, parts)
            self.follow[i] = True
        md = np.full(B, nr.GOTO_POSE, np.uint8)
        md[self.follow] = nr.FOLLOW_PATH
        self.mode = u8(md)
        self.buf = dict(valid=torch.full((B,), 9, dtype=U8, device=DEV), pose=torch.full((3, B), 7.0, device=DEV),
                        vel=torch.full((3, B), 7.0, device=DEV), steer_out=torch.full((B,), 7.0, device=DEV))
        self.event = torch.zeros(B, dtype=U8, device=DEV)
        self.n_solved = torch.zeros(1, dtype=I32, device=DEV)
        self.tick_no = 0
        p = host(self.loop.pose).astype(np.float64)
        s.push_samples(t(np.full(B, NOW - 27 * MS), I64), t(p, F64))  # (the robots stand)
        self.lim = None

    def set_extra(self, extra):
        self.extra = np.array(extra, np.float64)
        if self.extra.shape[1]:
            self.xy[:, :, self.B:] = t(self.extra, F64)[None]

    def resident(self):
        torch.cuda.synchronize()
        d = {f"state{k}": host(v.to_tensor()) for k, v in enumerate(self.s.state())}
        w, rec = self.s.warm_state()
        d.update(warm=host(w.to_tensor()), records=host(rec.to_tensor()), reset=host(self.reset))
        if self.q is not None:
            d.update(head=host(self.q.head), tail=host(self.q.tail), path_u=host(self.q.path_u),
                     remains=host(self.q.remains))
        return d

    def retarget(self, i, goal):
        """a new goal with the reset flag and, as the caller of a held robot must, zero carried speed refs"""
        self.goal[:, i] = goal
        r = host(self.reset)
        r[i] = 1
        self.reset.copy_(u8(r))
        c = self.s.state()[2].to_tensor()
        nv = sc.speed_rows(self.model, self.s.nbx)
        c[:nv, i] = 0.0
        self.s.state()[2].copy_from(c)
        self.fleet.carried[i][:nv] = 0.0

    def tick(self):
        s, B, N, o, model = self.s, self.B, gc.N, self.o, self.model
        now = NOW + self.tick_no * 25 * MS
        pose32 = host(self.loop.pose)
        s.push_samples(t(np.full(B, now - 2 * MS), I64), t(pose32.astype(np.float64), F64))
        # the input stage skips a robot in IDLE or ERROR: the cycle's export writes it at the pose the stage last gave
        # it, not where its plant has coasted to since (the stage's rule, nmpc_batch_node_input)
        skipped = ~np.isin(host(self.mode), (nr.GOTO_POSE, nr.FOLLOW_PATH, nr.BREAK))
        pose32[:, skipped] = host(self.buf["pose"])[:, skipped]
        # the restatement on the device's state before the cycle
        xbar = host(s.state()[0].to_tensor())[:, :B]
        car = host(s.state()[2].to_tensor())[:, :B]
        reset, mode = host(self.reset), host(self.mode)
        held = get_held(s, B) if self.guarded else np.zeros(B, np.uint8)
        xy = None
        if self.tracks:
            xy = np.zeros((N + 1, 2, B + self.extra.shape[1]))
            xy[:, :, B:] = self.extra[None]
            gr.export(xy, 0, xbar, o.nx, N, B, None, pose32, reset, mode, held)
        lim, _, gap_all = gr.limits(xbar, o.nx, N, B, xy, F32(o.prm.ubx[0]), F32(o.prm.ubu[0]), o.prm.dt, car,
                                    sc.speed_rows(model, o.nbx), pose=pose32, reset=reset, held=held,
                                    own_first=0 if self.tracks else -1, priority=self.priority, **gc.RULE)
        want_held = gr.hold(gap_all, held, reset, mode, **gc.GUARD) if self.guarded else held
        driving = np.isin(mode, (nr.GOTO_POSE, nr.FOLLOW_PATH))
        on_path = mode == nr.FOLLOW_PATH
        arrive = np.array([mode[i] == nr.GOTO_POSE and not want_held[i]
                           and gc.arrived(pose32[:, i].astype(np.float64), self.goal[:, i]) for i in range(B)])
        solve = driving & ~want_held.astype(bool) & ~arrive
        want_mode = np.where(arrive, nr.IDLE, mode)
        want_event = np.where(want_held.astype(bool) & driving, gr.EV_HELD,
                              np.where(arrive, _lib.NODE_EV_ARRIVED, np.where(solve, _lib.NODE_EV_SOLVED, 0)))
        before = self.resident()
        traj_out = torch.zeros(N + 1, 3, B, device=DEV)
        ni = NodeInput.default(now_ns=now, steer=self.loop.steer_arg, **self.buf)
        s.node_cycle(NodeParams.default(), ni, self.mode, goal_map=t(self.goal, F64), reset=self.reset,
                     event=self.event, traj_out=traj_out, n_solved=self.n_solved, queue=self.q, **self.loop.out)
        after = self.resident()
        what = (self.tick_no, held.tolist(), want_held.tolist())
        # a robot on a path that is not held: the gate and the march, which are unchanged, decide (SOLVED, NEXT_PART on a
        # hop, ARRIVED at the end); what they decided is taken from the device
        for i in np.flatnonzero(on_path & ~want_held.astype(bool)):
            ev = int(host(self.event)[i])
            assert ev in (_lib.NODE_EV_SOLVED, _lib.NODE_EV_NEXT_PART, _lib.NODE_EV_ARRIVED), (what, ev)
            want_event[i], want_mode[i], solve[i] = ev, host(self.mode)[i], ev == _lib.NODE_EV_SOLVED
        assert host(self.buf["valid"]).all(), what
        assert np.array_equal(bits(host(self.buf["pose"])[:2]), bits(pose32[:2])), what
        if self.guarded:
            assert np.array_equal(get_held(s, B), want_held), what
        assert np.array_equal(host(self.mode), want_mode), what
        assert np.array_equal(host(self.event), want_event), (what, host(self.event), want_event)
        assert int(self.n_solved[0]) == int(solve.sum()), what
        out = {k: host(v) for k, v in self.loop.out.items()}
        for i in np.flatnonzero(~solve):  # the stop command, the values of a robot that does not solve
            assert not out["cmd"][:, i].any() and not out["u0"][:, i].any() and not out["qp_res"][:, i].any(), what
            assert out["status"][i] == 0 and out["qp_iter"][i] == 0, what
            if want_held[i] or not on_path[i]:
                assert np.isnan(host(traj_out)[:, :, i]).all(), what
        for i in np.flatnonzero(want_held.astype(bool)):  # the resident rows of a held robot, byte for byte
            for k in before:
                if k in ("records",):
                    continue
                x, y = before[k], after[k]
                cx, cy = (x[..., i], y[..., i]) if x.ndim > 1 or k in ("reset", "head", "tail", "path_u", "remains") \
                    else (x, y)
                assert np.array_equal(np.ascontiguousarray(cx).view(np.uint8), np.ascontiguousarray(cy).view(np.uint8)), (what, k)
        # nobody solved and nobody's window hopped to its next part: everything resident, the records too
        if not solve.any() and not (on_path & ~want_held.astype(bool)).any():
            for k in before:
                assert np.array_equal(before[k].view(np.uint8), after[k].view(np.uint8)), (what, k)
        # the spliced fp64 reference on the device's inputs for the robots that solve
        f64 = lambda a: np.ascontiguousarray(a, np.float64)  # noqa: E731
        for i in np.flatnonzero(solve & reset.astype(bool)):
            self.fleet.xbar[i][:], self.fleet.ubar[i][:] = 0.0, 0.0
        goal32 = self.goal.astype(F32)  # (no frame table: the stage's goal_out is the fp32 rounding)
        traj = np.repeat(f64(goal32).T[:, None, :], N + 1, axis=1)
        dev_traj = f64(host(traj_out).transpose(2, 0, 1))  # the march's references of the robots on a path
        traj[on_path & solve] = dev_traj[on_path & solve]
        boxes = [mc.box_of(model, o, lim[:, i].astype(np.float64)) for i in range(B)]
        P = {k: np.stack([b[k] for b in boxes]) for k in sc.FIELDS}
        steer = f64(host(self.buf["steer_out"])) if model == "tric" else None
        _, u0_o, st_o, _ = self.fleet.tick(f64(host(self.buf["pose"]).T), f64(host(self.buf["vel"]).T), steer, traj,
                                           np.where(on_path, N + 1, 1).astype(np.int32), P=P,
                                           only=np.flatnonzero(solve))
        eu = float(np.abs(out["u0"].T - u0_o)[solve].max()) if solve.any() else 0.0
        assert (st_o == 0).all() and (out["status"] == 0).all(), (what, st_o, out["status"])
        assert eu <= TOL_U, (what, eu)
        # the plants
        status = torch.where(t(solve.astype(np.int32), I32) != 0, self.loop.out["status"], torch.ones_like(self.loop.out["status"]))
        L = self.loop
        s.fleet_sim_step(L.path, L.prog, L.pose, L.vel, L.steer_arg, L.out["u0"], status, L.traj, L.tlen, advance=True)
        torch.cuda.synchronize()
        p, v = host(L.pose).astype(np.float64), host(L.vel).astype(np.float64)
        for i in np.flatnonzero(~solve):
            pn, (vn, _) = gc.stop_step(model, o, p[:, i].copy(), v[:, i].copy(), 0.0)
            p[:, i], v[:, i] = pn, vn
        L.pose.copy_(t(p.astype(F32)))
        L.vel.copy_(t(v.astype(F32)))
        self.tick_no += 1
        self.lim = lim
        return dict(held=want_held, solve=solve, event=want_event, eu=eu, lim=lim, processed=driving,
                    dist=float(np.hypot(*(p[:2, 0] - p[:2, 1]))))


@pytest.mark.parametrize("queue", [False, True], ids=["plain", "queue"])
def test_cycle_head_on(built, queue):
    """the head-on pair through the cycle: both end held and report HELD from then on, nothing of them moves on the
    handle, the distance stays above stop_gap - 2 D_STOP; robot 0's new goal and reset flag take it out, robot 1
    resumes by itself"""
    model, T = "diff", 260
    c = CycleLoop(model, gc.head_on_fleet(model), queue=queue)
    log = []
    for tick in range(T):
        if tick == gc.RETARGET:
            c.retarget(*gc.HEAD_ON_NEW_GOAL)
        log.append(c.tick())
    held = np.array([r["held"] for r in log])
    dist = np.array([r["dist"] for r in log])
    R = gc.RETARGET
    first = int(np.argmax(held.all(axis=1)))
    print(f"{model}: held from tick {first}; smallest centre distance {dist[:R].min():.4f} m; |du0| at most "
          f"{max(r['eu'] for r in log):.2e}")
    assert 0 < first < R and held[first:R].all()
    assert dist[:R].min() >= gc.GUARD["stop_gap"] - 2 * gc.D_STOP
    i = gc.HEAD_ON_NEW_GOAL[0]
    assert not held[R:, i].any() and log[R]["solve"][i]
    freed = R + int(np.argmin(held[R:, 1 - i]))
    assert R < freed < T and held[R:freed, 1 - i].all() and not held[freed:, 1 - i].any()
    assert all(r["solve"][1 - i] for r in log[freed:]) and dist[-1] > dist[freed]
    if queue:  # (GOTO_POSE: the gate says "not in FollowPath" for a robot it decides, and nothing for a held one)
        assert np.isnan(host(c.q.remains)).all()


def test_cycle_crossing_winner_sees_no_tracks(built):
    """the crossing with priorities (0, 1) against a handle with no tracks attached, the same plant: the winner's
    limits are that handle's bit for bit on every tick, nobody is held, and the loser slows down"""
    model, T = "diff", 110
    a = CycleLoop(model, gc.crossing_fleet(model), priority=gc.CROSS_PRIORITY)
    b = CycleLoop(model, gc.crossing_fleet(model), guard=False, tracks=False)
    w = int(np.argmax(gc.CROSS_PRIORITY))
    twin = BatchSolver(model, gc.N, 2, device=DEV)
    slowed = 0
    for tick in range(T):
        ra, rb = a.tick(), b.tick()
        assert not ra["held"].any(), tick
        assert np.array_equal(bits(ra["lim"][:, w]), bits(rb["lim"][:, w])), tick
        # ... and on the device, every tick: the stage table against the restatement's limits through a twin. The
        # handle without tracks has no stage table at all: its launches take the handle's box, which is what the
        # restatement's lim is there (cap at every stage; asserted: c never exceeds it)
        assert (rb["lim"][:, w] == F32(1.0)).all(), tick
        slowed += int(ra["lim"][1, 1 - w] < F32(1.0))
        # (the writer processes the robots that drive; the rows of one that has arrived stay)
        twin.set_stage_limits(v_max=t(ra["lim"]), mask=u8(ra["processed"]))
        assert torch.equal(table_bytes(a.s), table_bytes(twin)), tick
        assert b.s.stage_bounds() is None
    assert slowed > 20 and ra["event"][w] in (_lib.NODE_EV_ARRIVED, _lib.NODE_EV_NONE)  # (the winner is through)


def test_cycle_held_on_a_path_keeps_its_window(built):
    """A robot in FOLLOW_PATH on a path set of four straight parts in the queue drives at a standing obstacle on its
    path. It is held in the second part (head 1, a finite remains, path_u inside the part): while it is held the window,
    path_u and remains stay byte for byte (CycleLoop.tick compares every resident row of a held robot), the mode stays
    FOLLOW_PATH and the event is HELD. The obstacle is then taken away: the robot is released in the next cycle and
    goes on along its path, remains falling. The second robot stands far away (it arrives at once and goes IDLE)."""
    from nmpc_nav_control_amd.path import PathSegment
    model = "diff"
    parts = [PathSegment.line((0.5 * k, 0.0), (0.5 * (k + 1), 0.0), 0.3) for k in range(4)]
    fl = gc.goal_fleet(model, [[0.0, 0.0, 0.0], [0.0, 10.0, 0.0]], [[0.0, 0.0, 0.0], [0.0, 10.0, 0.0]])
    c = CycleLoop(model, fl, queue=True, follow={0: parts}, extra=[[1.2], [0.0]])
    q = c.q
    log, first = [], None
    for tick in range(700):
        r = c.tick()
        log.append(r)
        if r["held"][0]:
            first = tick
            break
    assert first is not None and first > 20, "the robot is never held"
    snap = {k: host(getattr(q, k)).copy() for k in ("head", "tail", "path_u", "remains")}
    assert snap["head"][0] == 1 and snap["tail"][0] > snap["head"][0], snap
    assert np.isfinite(snap["remains"][0]) and 0 < snap["remains"][0] < 3 and 0 < snap["path_u"][0] < 1, snap
    for _ in range(30):
        r = c.tick()
        assert r["held"][0] and r["event"][0] == gr.EV_HELD and host(c.mode)[0] == nr.FOLLOW_PATH
        for k, v in snap.items():
            assert np.array_equal(host(getattr(q, k)).view(np.uint8), v.view(np.uint8)), k
    x_held = float(host(c.loop.pose)[0, 0])
    assert 1.2 - x_held >= gc.GUARD["stop_gap"] - 2 * gc.D_STOP
    c.set_extra([[100.0], [100.0]])
    after = [c.tick() for _ in range(60)]
    assert not any(r["held"][0] for r in after) and after[0]["solve"][0]
    assert sum(bool(r["solve"][0]) for r in after) >= 55 and host(c.mode)[0] == nr.FOLLOW_PATH
    assert float(host(c.loop.pose)[0, 0]) > x_held + 0.2 and abs(float(host(c.loop.pose)[1, 0])) < 0.02
    assert host(q.remains)[0] < snap["remains"][0] - 0.3
    print(f"held from tick {first} at x = {x_held:.4f} with head {snap['head'][0]}, path_u {snap['path_u'][0]:.4f}, "
          f"remains {snap['remains'][0]:.4f}; after the release remains {host(q.remains)[0]:.4f}; |du0| at most "
          f"{max(r['eu'] for r in log + after):.2e}")


def test_guard_without_tracks_is_inert(built):
    """a guard attached to a handle without tracks: the cycle's outputs and state are those of a handle that never
    heard of it, no stage table, held stays 0"""
    model, T = "diff", 6
    a = CycleLoop(model, gc.head_on_fleet(model), guard=True, tracks=False)
    b = CycleLoop(model, gc.head_on_fleet(model), guard=False, tracks=False)
    for tick in range(T):
        a.tick(), b.tick()
        ra, rb = a.resident(), b.resident()
        for k in ra:
            # (two handles: the row-parallel kernel's records hold slots that no solve reads and idle lanes store to,
            # tests/test_gpu_frame.py:same_resident; the multipliers a solve reads show in the next tick's outputs)
            if k != "records":
                assert np.array_equal(ra[k].view(np.uint8), rb[k].view(np.uint8)), (tick, k)
        for k in a.loop.out:
            assert torch.equal(a.loop.out[k], b.loop.out[k]), (tick, k)
        assert torch.equal(a.event, b.event) and torch.equal(a.mode, b.mode)
    assert a.s.stage_bounds() is None and not get_held(a.s, 2).any()
