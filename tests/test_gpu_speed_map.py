"""The speed map on the device (-m gpu): nmpc_batch_stage_limits_from_map (csrc/speed_map.hip) against
tests/speed_map_ref.py, the closed loop on the harness plant against the spliced fp64 reference, and the cycle with a
map attached against its parts.

Tolerances. vlim is compared with the restatement bit for bit (the same fp32 and fp64 operations in the same order, the
file is compiled without contraction) and stage tables handle to handle, byte for byte (the layout is opaque). The
closed loop is held to the project's parity bar, |u0 - reference| <= 1e-3 with every status 0, the reference being
tests/stage_bound_cases.py:solve_spliced on the device's own inputs and the device's vlim; a robot's commanded speed
may exceed its own cell's limit by one ramp step g = 0.02 (the CPU loop measures 3.9e-3) plus that bar. The cycle
comparisons are bit for bit.

Shapes: B = 21 robots on a handle of capacity 24 (a stride / B mix-up shows; two blocks of 16 robots, the second
partial) at N = 20 (21 stages: two rounds of a robot's 16 lanes, the second partial); N = 80, B = 5 (81 stages: more
than a wave has lanes, and two chunks of a lane's stage loop); N = 1023 and 1024, B = 5, the two sides of the horizon
at which the kernel goes from 16 to 8 robots per block; the loop has 16 robots at N = 20.

Measured (MI355X, diff / omni4 / tric): closed loop |u0 - reference| at most 1.2e-4 / 2.6e-5 / 2.3e-4; from tick 20 on a
robot above its own cell's limit by at most 0 / 3.9e-3 / 3.0e-8; the limit binds on 235 / 299 / 117 of 640 robot-ticks."""
import numpy as np
import pytest
import torch

from nmpc_nav_control_amd.batch import BatchSolver, NodeParams, SpeedMap
from oracle.oracle import Oracle
from tests import frame_cases as fc
from tests import node_input_ref as nr
from tests import speed_map_cases as mc
from tests import speed_map_ref as sr
from tests import stage_bound_cases as sc
from tests.table_harness import DEV, MODELS, TOL_U, Loop, t
from tests.test_gpu_node_input import B as RIG_B
from tests.test_gpu_node_input import Rig, host, same_everything, u8

pytestmark = pytest.mark.gpu
F64, U8 = torch.float64, torch.uint8
BASE = (500000.0, 4649776.0)  # frame_cases.OFFSETS[2]: a UTM-sized projected coordinate


def dev_map(m):
    return SpeedMap(m.x0, m.y0, m.res, t(m.vmax), outside=float(m.outside))


def table_bytes(s):
    torch.cuda.synchronize()
    return s.stage_bounds().to_tensor()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- 3. the writer against the restatement ------------------------------------------------------------------------
def layout(N, B, cap, nx, m, rng):
    """the iterate's positions [N+1][2][cap] relative to the map's low corner region, and the poses [3][B]: random over
    a box somewhat larger than the grid, then whole robots off the grid on each side, on a cell edge and half a cell
    below x0"""
    w, h = m.w * m.res, m.h * m.res  # the grid spans [-1.25, 2] x [-0.75, 1] about its anchor
    q = np.stack([rng.uniform(-1.25 - 0.4, -1.25 + w + 0.4, (N + 1, cap)),
                  rng.uniform(-0.75 - 0.4, -0.75 + h + 0.4, (N + 1, cap))], axis=1)
    k = np.arange(N + 1)
    q[:, 0, 1] = -1.25 - rng.uniform(0.3, 2, N + 1)      # robot 1: left of the grid
    q[:, 0, 2] = -1.25 + w + rng.uniform(0.0, 2, N + 1)  # robot 2: right of it
    q[:, 1, 4] = -0.75 - rng.uniform(0.3, 2, N + 1)      # robot 4: below
    if cap > 10:  # (the handle of five robots has the four above and robot 0's pose)
        q[:, 1, 6] = -0.75 + h + rng.uniform(0.0, 2, N + 1)  # robot 6: above
        q[:, 0, 7] = -1.25 + 0.25 * (k % (m.w + 1))  # robot 7: exactly on the cell edges, the grid's upper edges
        q[:, 1, 7] = -0.75 + 0.25 * (k % (m.h + 1))  # (which are outside) among them
        q[:, :, 8] = (-1.25 - 0.125, 0.0)            # robot 8: half a cell below x0
        q[:, :, 9] = (-1.25 + 9 * 0.25 + 0.1, -0.75 + 2 * 0.25 + 0.1)   # robot 9: in the NaN cell, row 2 column 9
        q[k % 2 == 0, :, 12] = (-1.25 + 3 * 0.25 + 0.1, -0.75 + 5 * 0.25 + 0.1)  # robot 12: in and out of the +inf cell
    pose = np.stack([rng.uniform(-1.5, 2.2, B), rng.uniform(-1.0, 1.2, B), rng.uniform(-3, 3, B)])
    pose[:2, 0] = (-1.25 - 0.125, 0.25)  # robot 0 is reset: its pose is half a cell below x0, on a cell edge in y
    return q, pose


def writer_case(model, N, B, cap, frames, table, seed):
    rng = np.random.default_rng(seed)
    s, twin = (BatchSolver(model, N, cap, device=DEV) for _ in range(2))
    nx, nbx, nbu = s.nx, s.nbx, s.nbu
    at = BASE if frames else (0.0, 0.0)
    m = mc.map_b(at)
    q, pose = layout(N, B, cap, nx, m, rng)
    origin = None
    if frames:  # origins a metre or two from the anchor, robot by robot; the positions are relative to them
        jit = rng.integers(-2, 3, (2, cap)).astype(np.float64)
        origin = np.array(BASE)[:, None] + jit
        q = q - jit[None]
        pose[:2] -= jit[:, :B]
        for h in (s, twin):
            h.set_robot_frame(t(origin, F64))
    xbar = rng.uniform(-2, 2, ((N + 1) * nx, cap)).astype(np.float32)
    xb3 = xbar.reshape(N + 1, nx, cap)
    xb3[:, :2] = q.astype(np.float32)
    carried = rng.uniform(-0.6, 0.6, (nbx, cap)).astype(np.float32)
    for h in (s, twin):
        h.state()[0].copy_from(t(xbar))
        h.state()[2].copy_from(t(carried))
    o = Oracle(model, N, rule="batched")
    cap_v, acc = np.float32(o.prm.ubx[0]), np.float32(o.prm.ubu[0])
    if table:  # the per-robot table on, with its own ubx / ubu
        ubx = rng.uniform(0.3, 0.9, (nbx, B)).astype(np.float32)
        ubu = rng.uniform(0.4, 1.6, (nbu, B)).astype(np.float32)
        for h in (s, twin):
            h.set_robot_params(ubx=t(ubx), ubu=t(ubu))
        cap_v, acc = ubx[0], ubu[0]
    reset = (np.arange(B) % 5 == 0).astype(np.uint8)
    mask = np.ones(B, np.uint8)
    mask[[i for i in (3, 11) if i < B]] = 0
    pose32 = pose.astype(np.float32)
    pos = sr.stage_positions(xbar, nx, N, B, pose32, reset)
    want = sr.limits(m, pos, cap_v, acc, o.prm.dt, carried[:, :B], sc.speed_rows(model, nbx),
                     None if origin is None else origin[:, :B], slope=0.7, v_floor=0.06)
    vlim = torch.full((N + 1, B), 7.0, device=DEV)
    before = [v.to_tensor() for v in s.state()]
    s.stage_limits_from_map(dev_map(m), pose=t(pose32), reset=u8(reset), mask=u8(mask), vlim=vlim, slope=0.7,
                            v_floor=0.06)
    torch.cuda.synchronize()
    got = host(vlim)
    on = mask.astype(bool)
    assert np.array_equal(bits(got[:, on]), bits(want[:, on])), np.argwhere(bits(got[:, on]) != bits(want[:, on]))[:8]
    assert (got[:, ~on] == 7.0).all()
    for x, y in zip(before, [v.to_tensor() for v in s.state()]):
        assert torch.equal(x, y)  # the writer reads the resident state
    # the cases are in the inputs: cells of every kind, and the off-grid value
    cells = m.cell(pos[:, 0].astype(np.float64) + (0 if origin is None else origin[0, :B]),
                   pos[:, 1].astype(np.float64) + (0 if origin is None else origin[1, :B]))
    assert (cells == np.float32(0.3)).any() and (B < 13 or (np.isnan(cells[:, 9]).all() and np.isinf(cells[::2, 12]).all()))
    # the table: a twin that is given the reference's limits through set_stage_limits
    ref_full = np.where(on[None, :], want, np.float32(7.0)).astype(np.float32)
    twin.set_stage_limits(v_max=t(ref_full), mask=u8(mask))
    assert torch.equal(table_bytes(s), table_bytes(twin))
    return want


@pytest.mark.parametrize("frames", [False, True], ids=["origin", "frames"])
@pytest.mark.parametrize("model", MODELS)
def test_writer_bit_for_bit(built, model, frames):
    table = (model, frames) in (("omni4", True), ("tric", False))
    writer_case(model, 20, 21, 24, frames, table, seed=31)


@pytest.mark.parametrize("model", MODELS)
def test_writer_more_stages_than_lanes(built, model):
    writer_case(model, 80, 5, 8, True, model == "diff", seed=32)


@pytest.mark.parametrize("N", [1023, 1024])
def test_writer_long_horizons(built, N):
    """N = 1023 is the last horizon with 16 robots per block (the block's z values fill the 64 KiB of LDS exactly),
    N = 1024 the first with 8 robots per block and 32 lanes per robot"""
    writer_case("diff", N, 5, 8, False, False, seed=33)


def test_writer_edges_by_hand(built):
    """half a cell below x0 is outside (a truncating cast would say cell 0), the upper edge is outside, a lower edge is
    its cell: one robot, reset, standing there; lim_0 = max(z, c) with z = min(cap, cell)"""
    m = mc.map_b()
    s = BatchSolver("diff", 20, 4, device=DEV)
    vlim = torch.zeros(21, 4, device=DEV)
    pose = np.zeros((3, 4), np.float32)
    pose[0] = [-1.25 - 0.125, -1.25 + 13 * 0.25, -1.25 + 0.25, 0.0]
    pose[1] = [0.0, 0.0, -0.75, np.nan]
    s.stage_limits_from_map(dev_map(m), pose=t(pose), reset=u8(np.ones(4)), vlim=vlim)
    torch.cuda.synchronize()
    got = host(vlim)
    assert (got[:, [0, 1, 3]] == np.float32(0.3)).all()  # outside
    assert (got[:, 2] == m.vmax[0, 1]).all() and m.vmax[0, 1] != m.vmax[1, 0]  # row cy = 0, column cx = 1


# ---- 4. closed loop on the device ---------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
def test_closed_loop_on_the_device(built, model):
    N, B, T = 20, 16, 40
    s = BatchSolver(model, N, B, device=DEV)
    loop = Loop(s, model, B, seed=mc.SEED)
    _, fleet = sc.default_fleet(model, N, B, mc.SEED)
    o, m = fleet.os[0], mc.map_a()
    dm = dev_map(m)
    g = float((np.float32(mc.SLOPE) * np.float32(o.prm.ubu[0])) * np.float32(o.prm.dt))
    fresh = np.ones(B, np.uint8)  # a robot counts as reset until its first successful solve
    vlim = torch.zeros(N + 1, B, device=DEV)
    worst_u, worst_zone, binds = 0.0, -np.inf, 0
    for tick in range(T):
        s.stage_limits_from_map(dm, pose=loop.pose, reset=u8(fresh), vlim=vlim, slope=mc.SLOPE, v_floor=mc.V_FLOOR)
        inp = loop.host_inputs()
        lim = host(vlim).astype(np.float64)
        zone = np.array([mc.cell_limit(o, m, inp[0][i]) for i in range(B)])
        loop.run()
        boxes = [mc.box_of(model, o, lim[:, i]) for i in range(B)]
        P = {k: np.stack([b[k] for b in boxes]) for k in sc.FIELDS}
        _, u0_o, st_o, it_o = fleet.tick(*inp, P=P)
        st = host(loop.out["status"])
        eu = np.abs(host(loop.out["u0"]).T - u0_o).max()
        speed = sc.speed_of(model, host(loop.carried()).T)
        print(f"tick {tick}: reference iters <= {it_o.max()}, |du0| {eu:.2e}, speed - cell limit "
              f"{(speed - zone).max():.2e}")
        assert (st_o == 0).all() and (st == 0).all(), (tick, st_o, st)
        assert eu <= TOL_U, (tick, eu)
        worst_u = max(worst_u, eu)
        binds += int((speed >= lim[1] - 1e-3).sum())
        if tick >= 20:
            worst_zone = max(worst_zone, (speed - zone).max())
            assert (speed - zone).max() <= g + 1e-3, tick
        fresh[st == 0] = 0
        loop.advance()
    print(f"{model}: |du0| at most {worst_u:.2e}; speed above the cell's limit from tick 20 at most {worst_zone:.2e}; "
          f"the limit binds on {binds} of {T * B} robot-ticks")
    assert binds >= 0.1 * T * B  # (the map matters in this loop, as in the CPU loop)


# ---- 5. the cycle ----------------------------------------------------------------------------------------------------
RULE = dict(slope=0.6, v_floor=0.07)


def by_parts(r, dm, vlim, **opt):
    """Rig.by_parts with the writer between the stage and the tick: pose from the stage, the cycle's reset, mask = the
    mode at that point is GOTO_POSE or FOLLOW_PATH. Returns that mask."""
    s, strict = r.s, opt.get("strict", 0)
    goal = torch.full((3, RIG_B), 7.0, device=DEV)
    s.node_input(r.node_input(**opt), r.mode, goal_map=r.goal_map, goal_out=goal)
    valid = host(r.buf["valid"])
    if strict:
        r.mode.copy_(u8(nr.strict_gate(valid, host(r.mode))))
    mask = np.isin(host(r.mode), (nr.GOTO_POSE, nr.FOLLOW_PATH)).astype(np.uint8)
    s.stage_limits_from_map(dm, pose=r.buf["pose"], reset=r.reset, mask=u8(mask), vlim=vlim, **RULE)
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
def test_cycle_with_a_map_is_its_parts(built, monkeypatch, model, queue, strict):
    stale = (0, 2, 7) if strict else ()
    a, b, c = (Rig(monkeypatch, model, queue=queue, stale=stale) for _ in range(3))
    dm = dev_map(mc.map_c(BASE))
    a.s.set_speed_map(dm, **RULE)
    opt = dict(strict=strict, pose_valid_overwritten=0, recentre_radius=8.0)
    N = a.s.N
    fill = torch.full((N + 1, RIG_B), 0.77, device=DEV)
    for r in (a, b, c):  # a table that holds something else than the handle's box
        r.s.set_stage_limits(v_max=fill)
    vlim = torch.zeros(N + 1, RIG_B, device=DEV)
    for tick in range(2):
        a.cycle(**opt)
        mask = by_parts(b, dm, vlim, **opt)
        same_everything(a.everything(), b.everything(), (tick, "cycle against its parts"))
        assert torch.equal(table_bytes(a.s), table_bytes(b.s)), tick
        if tick:
            continue
        assert 3 <= int(mask.sum()) < RIG_B
        assert mask[2::4].any() and mask[0::4].any()  # robots on the grid (their origin is BASE) and off it
        if strict:  # the invalid robots are ERROR before the writer: their rows are the 0.77 they held
            assert not mask[list(stale)].any() and (host(a.mode)[list(stale)] == nr.ERROR).all()
        c.s.set_stage_limits(v_max=vlim, mask=u8(mask))
        assert torch.equal(table_bytes(a.s), table_bytes(c.s))
        c.s.set_stage_limits(v_max=fill)
        assert not torch.equal(table_bytes(a.s), table_bytes(c.s))  # (the writer wrote something)


def test_cycle_without_a_map_is_unchanged(built, monkeypatch):
    """never attached, and attached then detached: node_cycle as on a handle that never saw the interface, and no stage
    table"""
    a, b = Rig(monkeypatch, "diff"), Rig(monkeypatch, "diff")
    b.s.set_speed_map(dev_map(mc.map_c(BASE)))
    b.s.set_speed_map(None)
    opt = dict(pose_valid_overwritten=0, recentre_radius=8.0)
    for tick in range(2):
        a.cycle(**opt)
        b.cycle(**opt)
        same_everything(a.everything(), b.everything(), (tick, "detached"))
        assert a.s.stage_bounds() is None and b.s.stage_bounds() is None
    assert int(a.out["n_solved"][0]) >= 3
