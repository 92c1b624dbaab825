"""Fleet separation on the device (-m gpu): nmpc_batch_export_tracks and nmpc_batch_stage_limits_from_tracks
(csrc/separation.hip) against tests/separation_ref.py, the convoy and the seeded fleet in closed loop on the harness
plant against the spliced fp64 reference, and the cycle with tracks attached against its parts.

Tolerances. The export, vlim and gap are compared with the restatement bit for bit (the same fp32 and fp64 operations in
the same order, the files are compiled without contraction, sqrtf is correctly rounded; min is exact, so the kernel's
tiles, chunks and culls cannot show) and stage tables handle to handle, byte for byte. The closed loops are held to the
project's parity bar, |u0 - reference| <= 1e-3 with every status 0, the reference being
tests/stage_bound_cases.py:solve_spliced on the device's own inputs and the device's vlim. The convoy's distance
conditions are the CPU loop's (tests/separation_cases.py:distances_ok). The cycle comparisons are bit for bit.

Shapes: B = 21 robots on a handle of capacity 24 (two blocks of 16 robot rows, the second partial) at N = 20 (21
stages: two of a lane's three stage slots, the second partial), M = 37 tracks (three chunks of 16, the last partial) with
the own tracks at 5..25; K = 0, 7, 20 and 25 (below, at and above N); M = 300 with B = 5 (19 chunks); N = 80 (81 stages:
two stage tiles of 48, the second partial); M = 0; the cull scene has B = 16 and M = 512.

Measured (MI355X, diff / omni4): convoy |u0 - reference| at most 5.7e-6 / 7.8e-6, smallest centre distance 0.7941 /
0.7646 m, last 40 of 160 ticks in [0.7950, 0.8011] / [0.7646, 0.7723] m. Parity loop (diff / omni4 / tric): |u0 -
reference| at most 1.2e-5 / 1.0e-4 / 2.9e-4, lim_1 < cap on 639 / 627 / 628 of 640 robot-ticks (the seeded fleet starts
within 2 m of itself), every status 0 on both sides. The cull scene keeps 2.1 of 512 tracks per robot."""
import numpy as np
import pytest
import torch

from nmpc_nav_control_amd.batch import BatchSolver, NodeParams, Tracks
from oracle.oracle import Oracle
from tests import node_input_ref as nr
from tests import separation_cases as cs
from tests import separation_ref as sp
from tests import speed_map_cases as mc
from tests import speed_map_ref as sr
from tests import stage_bound_cases as sc
from tests.table_harness import DEV, MODELS, TOL_U, Loop, _pad, t
from tests.test_gpu_node_input import B as RIG_B
from tests.test_gpu_node_input import Rig, host, same_everything, u8
from tests.test_gpu_speed_map import BASE, bits, dev_map, table_bytes

pytestmark = pytest.mark.gpu
F64, U8 = torch.float64, torch.uint8
F32 = np.float32
SEP = dict(clearance=0.3, gain=0.9, range=1.25, ahead_only=1)  # (not the defaults: every member arrives)
RULE = dict(slope=0.7, v_floor=0.06)
STEP = 0.0625  # metres per stage of the writer cases' robots, a dyadic number


def bits64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


# ---- 1. the export -----------------------------------------------------------------------------------------------
def random_state(s, rng, frames):
    """a random iterate and carried refs on the handle, and per-robot origins near BASE when frames: (xbar, carried,
    origin or None)"""
    cap, N, nx = s.capacity, s.N, s.nx
    xbar = rng.uniform(-2, 2, ((N + 1) * nx, cap)).astype(F32)
    carried = rng.uniform(-0.6, 0.6, (s.nbx, cap)).astype(F32)
    origin = None
    if frames:
        origin = np.array(BASE)[:, None] + rng.integers(-2, 3, (2, cap)).astype(np.float64)
        s.set_robot_frame(t(origin, F64))
    s.state()[0].copy_from(t(xbar))
    s.state()[2].copy_from(t(carried))
    return xbar, carried, origin


@pytest.mark.parametrize("frames", [False, True], ids=["origin", "frames"])
@pytest.mark.parametrize("model", MODELS)
def test_export_bit_for_bit(built, model, frames):
    N, B, cap, first, M = 20, 21, 24, 5, 37
    rng = np.random.default_rng(41)
    s = BatchSolver(model, N, cap, device=DEV)
    xbar, _, origin = random_state(s, rng, frames)
    pose = rng.uniform(-2, 2, (3, B)).astype(F32)
    reset = (np.arange(B) % 5 == 0).astype(np.uint8)
    mode = (np.arange(B) % 5).astype(np.uint8)[::-1].copy()  # all five modes, not aligned with reset
    assert set(mode) == {nr.IDLE, nr.GOTO_POSE, nr.FOLLOW_PATH, nr.BREAK, nr.ERROR}
    before = [v.to_tensor() for v in s.state()]
    for K in (7, 20, 25):
        for kw in (dict(), dict(reset=reset), dict(reset=reset, mode=mode)):
            want = np.full((K + 1, 2, M), -7.0)
            sp.export(want, first, xbar, s.nx, N, B, origin, pose if kw else None, **kw)
            xy = torch.full((K + 1, 2, M), -7.0, dtype=F64, device=DEV)
            s.export_tracks(xy, first=first, pose=t(pose) if kw else None, B=B, **{k: u8(v) for k, v in kw.items()})
            torch.cuda.synchronize()
            got = host(xy)
            assert np.array_equal(bits64(got), bits64(want)), (K, list(kw))
            assert (got[:, :, :first] == -7).all() and (got[:, :, first + B:] == -7).all()
    for x, y in zip(before, [v.to_tensor() for v in s.state()]):
        assert torch.equal(x, y)  # the export reads the resident state


# ---- 2. the writer against the restatement ------------------------------------------------------------------------
def scene(N, B, cap, M, K, rng, spread=2.0):
    """Robot horizons [N+1][2][cap] and poses [3][B] less the anchor, and random tracks xy [K+1][2][M] less the anchor.
    Robots 1 and 2 drive exactly along +x (STEP per stage), robot 4 stands in map B's NaN cell."""
    k = np.arange(N + 1)
    start = np.stack([rng.uniform(-1.5, 2.0, cap), rng.uniform(-1.0, 1.0, cap)])
    th = rng.uniform(-np.pi, np.pi, cap)
    q = start[None] + STEP * k[:, None, None] * np.stack([np.cos(th), np.sin(th)])[None]
    q += rng.uniform(-0.01, 0.01, q.shape)
    q[:, :, 1] = np.stack([-1.0 + STEP * k, np.full(N + 1, 0.75)], axis=1)
    q[:, :, 2] = np.stack([0.25 + STEP * k, np.full(N + 1, -0.5)], axis=1)
    q[:, :, 4] = (-1.25 + 9 * 0.25 + 0.1, -0.75 + 2 * 0.25 + 0.1)
    pose = np.stack([rng.uniform(-1.5, 2.2, B), rng.uniform(-1.0, 1.2, B), rng.uniform(-3, 3, B)])
    if M == 0:
        return q, pose, None
    t0 = np.stack([rng.uniform(-spread, spread + 0.5, M), rng.uniform(-spread, spread, M)])
    tv = rng.uniform(-STEP, STEP, (2, M))
    return q, pose, t0[None] + np.arange(K + 1)[:, None, None] * tv[None]


def place_classes(xy, P0, B, own_first):
    """the classes of the by-hand CPU test, placed about the robots' fp64 map positions at stage 0, P0 [2][B] (so the
    differences are exact): a track exactly at range ahead of robot 1; one an ulp of the fp32 difference beyond range
    ahead of robot 2, one exactly abeam of it and one behind it; one 0.5 m from robot 4; a NaN and an infinite track"""
    M = xy.shape[2]
    free = [j for j in range(M) if own_first < 0 or not own_first <= j < own_first + B]
    assert len(free) >= 7
    rg = float(F32(SEP["range"]))
    xy[:, :, free[0]] = P0[:, 1] + (rg, 0.0)
    xy[:, :, free[1]] = P0[:, 2] + (float(np.nextafter(F32(rg), F32(np.inf))), 0.0)
    xy[:, :, free[2]] = P0[:, 2] + (0.0, 1.0)
    xy[:, :, free[3]] = P0[:, 2] + (-1.0, 0.25)
    xy[:, :, free[4]] = P0[:, 4] + (0.5, 0.0)
    xy[xy.shape[0] // 2:, 0, free[5]] = np.nan
    xy[:, 1, free[6]] = np.inf


def writer_case(model, N, B, cap, M, K, own_first, frames, table, with_map, seed, ahead_only=1, spread=2.0):
    rng = np.random.default_rng(seed)
    s, twin = (BatchSolver(model, N, cap, device=DEV) for _ in range(2))
    nx, nbx, nbu = s.nx, s.nbx, s.nbu
    at = np.array(BASE if frames else (0.0, 0.0))
    m = mc.map_b(tuple(at)) if with_map else None
    q, pose, xy = scene(N, B, cap, M, K, rng, spread)
    origin = None
    if frames:  # origins a metre or two from the anchor, robot by robot; the positions are relative to them
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
    if table:  # the per-robot table on, with its own ubx / ubu
        ubx = rng.uniform(0.3, 0.9, (nbx, B)).astype(F32)
        ubu = rng.uniform(0.4, 1.6, (nbu, B)).astype(F32)
        for h in (s, twin):
            h.set_robot_params(ubx=t(ubx), ubu=t(ubu))
        cap_v, acc = ubx[0], ubu[0]
    reset = (np.arange(B) % 5 == 0).astype(np.uint8)
    mask = np.ones(B, np.uint8)
    mask[[i for i in (3, 11) if i < B]] = 0
    pose32 = pose.astype(F32)
    org_b = None if origin is None else origin[:, :B]
    pos = sr.stage_positions(xbar, nx, N, B, pose32, reset)
    if xy is not None:
        xy = xy + at[None, :, None]
        place_classes(xy, pos[0].astype(np.float64) + (0 if org_b is None else org_b), B, own_first)
        if own_first >= 0:  # the own tracks are the robots' own horizons: coincident with them, skipped by index
            sp.export(xy, own_first, xbar, nx, N, B, org_b, pose32, reset=reset)
    sep = dict(SEP, ahead_only=ahead_only)
    want, want_gap = sp.limits(pos, xy, cap_v, acc, o.prm.dt, carried[:, :B], sc.speed_rows(model, nbx), m=m,
                               origin=org_b, reset=reset, own_first=own_first, **sep, **RULE)
    vlim, gap = (torch.full((N + 1, B), 7.0, device=DEV) for _ in range(2))
    before = [v.to_tensor() for v in s.state()]
    tr = Tracks(None if xy is None else t(xy, F64), own_first=own_first)
    s.stage_limits_from_tracks(tr, map=dev_map(m) if m else None, pose=t(pose32), reset=u8(reset), mask=u8(mask),
                               vlim=vlim, gap=gap, **sep, **RULE)
    torch.cuda.synchronize()
    got, got_gap = host(vlim), host(gap)
    on = mask.astype(bool)
    # (the gaps first: they name the stage and the robot)
    assert np.array_equal(bits(got_gap[:, on]), bits(want_gap[:, on])), np.argwhere(got_gap[:, on] != want_gap[:, on])[:8]
    assert np.array_equal(bits(got[:, on]), bits(want[:, on])), np.argwhere(bits(got[:, on]) != bits(want[:, on]))[:8]
    assert (got[:, ~on] == 7.0).all() and (got_gap[:, ~on] == 7.0).all()
    for x, y in zip(before, [v.to_tensor() for v in s.state()]):
        assert torch.equal(x, y)  # the writer reads the resident state
    # the table: a twin that is given the reference's limits through set_stage_limits (the masked robots keep their rows)
    ref_full = np.where(on[None, :], want, F32(7.0)).astype(F32)
    twin.set_stage_limits(v_max=t(ref_full), mask=u8(mask))
    assert torch.equal(table_bytes(s), table_bytes(twin))
    if xy is None:
        assert np.isposinf(want_gap).all()
        return
    # the classes are in the inputs
    d = {}
    h = sp.headings(pos, reset)
    qq, counts = sp.pairs(pos, h, xy, own_first, org_b, sep["range"], ahead_only, details=d)
    r2 = F32(sep["range"]) * F32(sep["range"])
    moving = ((h[:, 0] != 0) | (h[:, 1] != 0))[:, :, None]
    assert (counts & (qq == r2)).any(), "a pair exactly at range"
    assert ((d["dx"] == np.nextafter(F32(sep["range"]), F32(np.inf))) & (d["dy"] == 0) & ~counts).any(), "an ulp beyond"
    assert ((qq <= r2) & (d["dot"] == 0) & moving & (counts == (not ahead_only))).any(), "exactly abeam"
    assert ((qq <= r2) & (d["dot"] < 0) & moving & (counts == (not ahead_only))).any(), "behind"
    assert counts[:, reset[:B].astype(bool)].any() and counts[:, 4].any(), "a standing robot with tracks in range"
    assert np.isnan(qq).any() and np.isinf(qq).any(), "NaN and infinite tracks"
    if own_first >= 0:
        i = np.arange(B)
        assert (qq[0, i, own_first + i] == 0).all() and not counts[:, i, own_first + i].any(), "the own track"
    if m is not None:
        cells = m.cell(pos[:, 0].astype(np.float64) + (0 if org_b is None else org_b[0]),
                       pos[:, 1].astype(np.float64) + (0 if org_b is None else org_b[1]))
        assert np.isnan(cells[:, 4]).all() and np.isfinite(want_gap[:, 4]).all() and (want[:, 4] == F32(RULE["v_floor"])).any()
    assert np.isfinite(want_gap).any()
    assert (want[:, on] < np.broadcast_to(cap_v, (B,))[on][None]).any()  # (the tracks matter)


# (frames, per-robot table, map): the table on for diff, frames on for omni4, map B attached for tric
SETUP = {"diff": (False, True, False), "omni4": (True, False, False), "tric": (False, False, True)}


@pytest.mark.parametrize("model", MODELS)
def test_writer_bit_for_bit(built, model):
    writer_case(model, 20, 21, 24, 37, 20, 5, *SETUP[model], seed=51)


@pytest.mark.parametrize("K", [0, 7])
def test_writer_short_tracks(built, K):
    """K = 0: static obstacles; K = 7: the track's last stage is read from stage 7 on"""
    writer_case("omni4", 20, 21, 24, 37, K, 5, True, False, True, seed=52)


def test_writer_no_own_tracks_and_all_around(built):
    writer_case("diff", 20, 21, 24, 37, 20, -1, False, False, False, seed=53)
    writer_case("diff", 20, 21, 24, 37, 20, -1, True, False, True, seed=54, ahead_only=0)


def test_writer_more_tracks_than_a_chunk(built):
    writer_case("tric", 20, 5, 8, 300, 20, 100, True, True, False, seed=55, spread=12.0)


def test_writer_more_stages_than_a_tile(built):
    writer_case("diff", 80, 5, 8, 20, 25, 5, True, False, True, seed=56)


@pytest.mark.parametrize("with_map", [False, True], ids=["no_map", "map"])
def test_writer_without_tracks_is_the_map_only_writer(built, with_map):
    """M = 0: what the restatement's map-only rule writes; with a map, byte for byte the table of
    nmpc_batch_stage_limits_from_map on a twin"""
    writer_case("omni4", 20, 21, 24, 0, 0, -1, True, False, with_map, seed=57)
    if not with_map:
        return
    rng = np.random.default_rng(58)
    a, b = (BatchSolver("diff", 20, 24, device=DEV) for _ in range(2))
    xbar = rng.uniform(-2, 2, ((20 + 1) * a.nx, 24)).astype(F32)
    carried = rng.uniform(-0.6, 0.6, (a.nbx, 24)).astype(F32)
    for h in (a, b):
        h.state()[0].copy_from(t(xbar))
        h.state()[2].copy_from(t(carried))
    dm = dev_map(mc.map_b())
    pose, reset = t(rng.uniform(-1, 1, (3, 21)).astype(F32)), u8(np.arange(21) % 5 == 0)
    va, vb = (torch.zeros(21, 21, device=DEV) for _ in range(2))
    a.stage_limits_from_tracks(Tracks(None), map=dm, pose=pose, reset=reset, vlim=va, **RULE)
    b.stage_limits_from_map(dm, pose=pose, reset=reset, vlim=vb, **RULE)
    assert torch.equal(table_bytes(a), table_bytes(b)) and torch.equal(va, vb)


# ---- 3. the cull ----------------------------------------------------------------------------------------------------
def test_cull_is_invisible(built):
    """A spread-out scene at UTM-sized coordinates with frames on: most tracks are culled by their boxes, sixteen sit on
    a ring at range (1 +- 2^-20) around the standing robot 0, and track 40's box overlaps robot 1's box although every one
    of its stage positions is out of range. Bit for bit the brute-force reference."""
    N, B, M, rg = 20, 16, 512, 3.0
    rng = np.random.default_rng(61)
    s = BatchSolver("diff", N, B, device=DEV)
    k = np.arange(N + 1)
    start = rng.uniform(-300, 300, (2, B))
    th = rng.uniform(-np.pi, np.pi, B)
    pm = start[None] + 0.1 * k[:, None, None] * np.stack([np.cos(th), np.sin(th)])[None] + np.array(BASE)[None, :, None]
    pm[:, :, 1] = np.stack([BASE[0] + 20 + 0.1 * k, np.full(N + 1, BASE[1] + 20)], axis=1)  # robot 1: along +x, 2 m
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
    t0 = rng.uniform(-500, 500, (2, M))
    near = rng.integers(0, B, M)
    t0[:, ::3] = start[:, near[::3]] + rng.uniform(-12, 12, (2, len(near[::3])))  # a third of them near some robot
    xy = t0[None] + k[:, None, None] * rng.uniform(-0.1, 0.1, (2, M))[None] + np.array(BASE)[None, :, None]
    X0 = q[0, :, 0].astype(np.float64) + origin[:, 0]
    ang = 2 * np.pi * np.arange(16) / 16 + 0.1
    rad = rg * (1 + np.where(np.arange(16) % 2 == 0, 1.0, -1.0) * 2.0 ** -20)
    xy[:, :, 16:32] = (X0[:, None] + rad[None] * np.stack([np.cos(ang), np.sin(ang)]))[None]
    xy[:11, :, 40] = (BASE[0] + 20 - 4, BASE[1] + 20 - 4)
    xy[11:, :, 40] = (BASE[0] + 20 + 6, BASE[1] + 20 + 6)
    pos = sr.stage_positions(xbar, s.nx, N, B, pose, reset)
    o = Oracle("diff", N, rule="batched")
    car = host(s.state()[2].to_tensor())[:, :B]
    want, want_gap = sp.limits(pos, xy, F32(o.prm.ubx[0]), F32(o.prm.ubu[0]), o.prm.dt, car, s.nbx, origin=origin,
                               reset=reset, range=rg)
    vlim, gap = (torch.zeros(N + 1, B, device=DEV) for _ in range(2))
    s.stage_limits_from_tracks(Tracks(t(xy, F64)), pose=t(pose), reset=u8(reset), vlim=vlim, gap=gap, range=rg)
    torch.cuda.synchronize()
    assert np.array_equal(bits(host(gap)), bits(want_gap)), np.argwhere(host(gap) != want_gap)[:8]
    assert np.array_equal(bits(host(vlim)), bits(want))
    # the scene is what it says
    qq, counts = sp.pairs(pos, sp.headings(pos, reset), xy, origin=origin, range=rg)
    ring = counts[0, 0, 16:32]
    assert ring.any() and not ring.all(), ring
    cull = sp.cull_counts(pos, xy, origin=origin, range=rg)
    assert cull["mask"][1, 40] and not counts[:, 1, 40].any() and (qq[:, 1, 40] > F32(rg) * F32(rg)).all()
    print(f"cull: {cull['box_tests']} box tests per robot, kept {cull['kept'].mean():.1f} tracks per robot "
          f"({cull['kept'].min()}..{cull['kept'].max()}), counting pairs {int(counts.sum())}")
    assert cull["kept"].mean() < 0.05 * M and counts.sum() > 50


# ---- 4. closed loops on the device ---------------------------------------------------------------------------------
class FleetLoop(Loop):
    """tests/table_harness.py:Loop on a fleet dict built by hand"""

    def __init__(self, solver, model, fl):
        B = fl["pose"].shape[1]
        self.s, self.model, self.B, self.fl = solver, model, B, fl
        N = solver.N
        solver.state()[2].copy_from(_pad(t(fl["carried"]), solver.capacity))
        self.pose, self.vel, self.steer = t(fl["pose"]), t(fl["vel"]), t(fl["steer"])
        self.path, self.prog = t(fl["path"]), t(fl["s"])
        self.steer_arg = self.steer if model == "tric" else None
        self.traj = torch.zeros(N + 1, 3, B, device=DEV)
        self.tlen = torch.zeros(B, dtype=torch.int32, device=DEV)
        self.out = dict(cmd=torch.zeros(3, B, device=DEV), u0=torch.zeros(solver.nu, B, device=DEV),
                        status=torch.zeros(B, dtype=torch.int32, device=DEV),
                        qp_iter=torch.zeros(B, dtype=torch.int32, device=DEV), qp_res=torch.zeros(3, B, device=DEV))
        solver.fleet_sim_step(self.path, self.prog, self.pose, self.vel, self.steer_arg, None, None, self.traj,
                              self.tlen, advance=False)


def separation_loop(model, loop, fleet, T, B, N, after_tick=None, **sep):
    """per tick: the fleet's own export is the tracks, the writer, run, the spliced fp64 reference on the device's inputs
    and the device's vlim, the plant step. Returns (worst |du0|, robot-ticks with lim_1 < cap)."""
    s, o = loop.s, fleet.os[0]
    fresh = np.ones(B, np.uint8)  # a robot counts as reset until its first successful solve
    xy = torch.zeros(N + 1, 2, B, dtype=F64, device=DEV)
    tr = Tracks(xy, own_first=0)
    vlim = torch.zeros(N + 1, B, device=DEV)
    cap = float(F32(o.prm.ubx[0]))
    worst, binds = 0.0, 0
    for tick in range(T):
        s.export_tracks(xy, first=0, pose=loop.pose, reset=u8(fresh))
        s.stage_limits_from_tracks(tr, pose=loop.pose, reset=u8(fresh), vlim=vlim, **sep)
        inp = loop.host_inputs()
        lim = host(vlim).astype(np.float64)
        loop.run()
        boxes = [mc.box_of(model, o, lim[:, i]) for i in range(B)]
        P = {k: np.stack([b[k] for b in boxes]) for k in sc.FIELDS}
        _, u0_o, st_o, _ = fleet.tick(*inp, P=P)
        st = host(loop.out["status"])
        eu = np.abs(host(loop.out["u0"]).T - u0_o).max()
        assert (st_o == 0).all() and (st == 0).all(), (tick, st_o, st)
        assert eu <= TOL_U, (tick, eu)
        worst = max(worst, eu)
        binds += int((lim[1] < cap).sum())
        fresh[st == 0] = 0
        loop.advance()
        if after_tick:
            after_tick(tick)
    return worst, binds


@pytest.mark.parametrize("model", ["diff", "omni4"])
def test_convoy_on_the_device(built, model):
    """the convoy of tests/separation_cases.py on the harness plant, 160 ticks (the steady gap is reached by tick 120).
    The rule-off run stays on the CPU (tests/test_separation_ref.py)."""
    T, B = 160, 2
    s = BatchSolver(model, cs.N, B, device=DEV)
    fl = cs.convoy_fleet(model)
    loop = FleetLoop(s, model, fl)
    fleet = sc.StageFleet([Oracle(model, cs.N, rule="batched") for _ in range(B)], fl["carried"].T)
    dist = []

    def measure(tick):
        torch.cuda.synchronize()
        p = host(loop.pose)
        dist.append(float(np.hypot(p[0, 0] - p[0, 1], p[1, 0] - p[1, 1])))

    worst, binds = separation_loop(model, loop, fleet, T, B, cs.N, after_tick=measure, **cs.RULE)
    print(f"{model}: |du0| at most {worst:.2e}; smallest centre distance {min(dist):.4f}, last 40 ticks "
          f"[{min(dist[-40:]):.4f}, {max(dist[-40:]):.4f}]; lim_1 < cap on {binds} of {T * B} robot-ticks")
    cs.distances_ok(dist, True)


@pytest.mark.parametrize("model", MODELS)
def test_parity_loop_with_the_fleets_own_tracks(built, model):
    """the seeded fleet of test_gpu_speed_map.py:test_closed_loop_on_the_device, each robot limited by the others'
    exported horizons. No share of binding limits is demanded of this scene (the convoy shows that the rule matters)."""
    N, B, T = 20, 16, 40
    s = BatchSolver(model, N, B, device=DEV)
    loop = Loop(s, model, B, seed=mc.SEED)
    _, fleet = sc.default_fleet(model, N, B, mc.SEED)
    worst, binds = separation_loop(model, loop, fleet, T, B, N)
    print(f"{model}: |du0| at most {worst:.2e}; lim_1 < cap on {binds} of {T * B} robot-ticks")


# ---- 5. the cycle ----------------------------------------------------------------------------------------------------
CYC_M, CYC_FIRST, CYC_K = RIG_B + 8, 4, 12
CYC_SEP = dict(clearance=0.4, gain=0.8, range=2.5, ahead_only=1)
CYC_RULE = dict(slope=0.6, v_floor=0.07)


def cycle_tracks():
    """the cycle tests' buffer: the rig's robots at the columns CYC_FIRST.., eight static tracks around BASE (where
    every fourth robot of the rig has its origin) in the others"""
    rng = np.random.default_rng(71)
    xy = np.full((CYC_K + 1, 2, CYC_M), 1e9)
    other = [j for j in range(CYC_M) if not CYC_FIRST <= j < CYC_FIRST + RIG_B]
    xy[:, :, other] = (np.array(BASE)[:, None] + rng.uniform(-2.5, 2.5, (2, len(other))))[None]
    return t(xy, F64)


def by_parts(r, tr, dm, vlim, gap, **opt):
    """Rig.by_parts with the export and the writer between the stage and the tick: pose from the stage, the cycle's
    reset and mode, mask = the mode at that point is GOTO_POSE or FOLLOW_PATH. Returns that mask."""
    s, strict = r.s, opt.get("strict", 0)
    goal = torch.full((3, RIG_B), 7.0, device=DEV)
    s.node_input(r.node_input(**opt), r.mode, goal_map=r.goal_map, goal_out=goal)
    valid = host(r.buf["valid"])
    if strict:
        r.mode.copy_(u8(nr.strict_gate(valid, host(r.mode))))
    mask = np.isin(host(r.mode), (nr.GOTO_POSE, nr.FOLLOW_PATH)).astype(np.uint8)
    s.export_tracks(tr.xy, first=CYC_FIRST, pose=r.buf["pose"], reset=r.reset, mode=r.mode)
    s.stage_limits_from_tracks(tr, map=dm, pose=r.buf["pose"], reset=r.reset, mask=u8(mask), vlim=vlim, gap=gap,
                               **CYC_SEP, **CYC_RULE)
    tick = dict(steer=r.buf["steer_out"] if r.model == "tric" else None, reset=r.reset, **r.out)
    if r.queue:
        s.node_tick_queue(NodeParams.default(), r.q, r.mode, r.buf["pose"], r.buf["vel"], goal=goal, **tick)
    else:
        s.node_tick(NodeParams.default(), r.mode, r.buf["pose"], r.buf["vel"], goal=goal, **r.paths, **tick)
    torch.cuda.synchronize()
    mode, event = host(r.mode), host(r.out["event"])
    remains = host(r.q.remains) if r.queue else None
    nr.cycle_status(valid, strict, mode, event, remains)
    r.mode.copy_(u8(mode))
    r.out["event"].copy_(u8(event))
    if r.queue:
        r.q.remains.copy_(t(remains, F64))
    return mask


@pytest.mark.parametrize("model,queue,strict", [(mdl, q, 0) for mdl in MODELS for q in (False, True)] +
                         [("diff", False, 1), ("omni4", True, 1), ("tric", False, 1)])
def test_cycle_with_tracks_is_its_parts(built, monkeypatch, model, queue, strict):
    stale = (0, 2, 7) if strict else ()
    a, b = (Rig(monkeypatch, model, queue=queue, stale=stale) for _ in range(2))
    dm = dev_map(mc.map_c(BASE))
    ta, tb = Tracks(cycle_tracks(), own_first=CYC_FIRST), Tracks(cycle_tracks(), own_first=CYC_FIRST)
    a.s.set_speed_map(dm, **CYC_RULE)
    a.s.set_tracks(ta, export_own=True, **CYC_SEP)
    opt = dict(strict=strict, pose_valid_overwritten=0, recentre_radius=8.0)
    N = a.s.N
    fill = torch.full((N + 1, RIG_B), 0.77, device=DEV)
    for r in (a, b):  # a table that holds something else than the handle's box
        r.s.set_stage_limits(v_max=fill)
    filled = table_bytes(a.s).clone()
    vlim, gap = (torch.zeros(N + 1, RIG_B, device=DEV) for _ in range(2))
    for tick in range(2):
        a.cycle(**opt)
        mask = by_parts(b, tb, dm, vlim, gap, **opt)
        same_everything(a.everything(), b.everything(), (tick, "cycle against its parts"))
        assert torch.equal(table_bytes(a.s), table_bytes(b.s)), tick
        assert torch.equal(ta.xy, tb.xy), tick
        if tick:
            continue
        assert 3 <= int(mask.sum()) < RIG_B
        assert not torch.equal(table_bytes(a.s), filled)  # (the writer wrote something)
        g = host(gap)[:, mask.astype(bool)]
        assert (np.isfinite(g) & (g > 0)).any()  # (tracks in range; the rig's unsolved iterates coincide: gap 0)
        own = host(ta.xy)[:, :, CYC_FIRST:CYC_FIRST + RIG_B]
        off = ~mask.astype(bool)  # every robot is exported; one that does not drive stands at its pose
        assert (own != 1e9).all() and (own[:, :, off] == own[:1, :, off]).all()
        if strict:  # the invalid robots are ERROR before the export and the writer
            assert not mask[list(stale)].any() and (host(a.mode)[list(stale)] == nr.ERROR).all()


def test_cycle_without_tracks_is_unchanged(built, monkeypatch):
    """never attached, detached without ever being attached, and attached then detached: node_cycle as on a handle that
    never saw the interface, and no stage table"""
    a, b, c = (Rig(monkeypatch, "diff") for _ in range(3))
    b.s.set_tracks(None)
    c.s.set_tracks(Tracks(cycle_tracks(), own_first=CYC_FIRST), export_own=True)
    c.s.set_tracks(None)
    opt = dict(pose_valid_overwritten=0, recentre_radius=8.0)
    for tick in range(2):
        for r in (a, b, c):
            r.cycle(**opt)
        same_everything(a.everything(), b.everything(), (tick, "never attached"))
        same_everything(a.everything(), c.everything(), (tick, "detached"))
        assert all(r.s.stage_bounds() is None for r in (a, b, c))
    assert int(a.out["n_solved"][0]) >= 3
