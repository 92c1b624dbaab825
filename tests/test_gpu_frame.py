"""Per-robot map frames on the device (-m gpu): the frame table's writers against tests/frame_ref.py bit for bit, run
and solve mode under a frame (they read nothing new), and a fleet that is re-centred while it runs.

Shapes: N in {1, 20}, B = 21 robots in a handle of capacity 37 for the writers (B, the capacity and the block of 256
are three numbers; robots at and past B are part of every comparison); N = 20, B = 21, 6 ticks with a cold tick and
every fifth robot reset before tick 3 for the loops, as tests/test_gpu_far_field.py. The origins are
tests/frame_cases.py's OFFSETS, mixed robot by robot.

The writers add and subtract in fp64 and round once, as frame_ref does in numpy, so those comparisons have no
tolerance. The loops are held to the project's |u0 - u0_oracle|, |cmd - cmd_oracle| <= 1e-3 with every status 0
(tests/table_harness.py:check_tick), the oracle running on the frame values the device is given.
"""
import math

import numpy as np
import pytest
import torch

from nmpc_nav_control_amd.batch import BatchSolver
from tests import frame_cases as fc
from tests import frame_ref as fr
from tests.table_harness import DEV, FORMS, MODELS, Loop, check_tick, make_solver, t
from tests.test_gpu_far_field import BatchOracle, solve_reference

pytestmark = pytest.mark.gpu
B, CAP = 21, 37
T, RESET_TICK = 6, 3
F64 = torch.float64


def bits32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def bits64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def whole_state(s):
    """everything resident: iterate, carried refs, warm flags, scratch records (host copies)"""
    torch.cuda.synchronize()
    return [v.to_tensor().cpu().numpy() for v in s.state() + s.warm_state()]


def same_state(a, b, what, skip=()):
    for k, (x, y) in enumerate(zip(a, b)):
        if k not in skip:
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), (what, k)


def same_resident(on, off, what, form):
    """iterate, carried refs and warm flags of two handles, and in the team form the scratch records whole. The
    row-parallel kernel's records hold slots that no solve reads and that lanes without work store to unconditionally
    (whatever their registers hold, which follows from the launches the handle saw before); the multipliers a warm
    solve does read show in the next tick's outputs, which are compared"""
    same_state(whole_state(on), whole_state(off), what, skip=() if form == "team_plain" else (4,))


class Writers:
    """a handle whose resident state is random, and frame_ref's model of its frame table and iterate"""

    def __init__(self, model, N, seed):
        self.s = s = BatchSolver(model, N, CAP, device=DEV)
        self.N, self.rng = N, np.random.default_rng(seed)
        r = self.rng
        xv, uv, cv = s.state()
        wv, sv = s.warm_state()
        xv.copy_from(t(r.uniform(-2, 2, xv.shape).astype(np.float32)))
        uv.copy_from(t(r.uniform(-1, 1, uv.shape).astype(np.float32)))
        cv.copy_from(t(r.uniform(-1, 1, cv.shape).astype(np.float32)))
        wv.copy_from(torch.from_numpy(r.integers(0, 3, wv.shape).astype(np.uint8)).to(DEV))
        sv.copy_from(t(r.uniform(-1, 1, sv.shape).astype(np.float32)))
        self.before = whole_state(s)
        self.ref = fr.Frames(CAP, N, s.nx, self.before[0].copy())

    def check(self, what):
        s = self.s
        now = whole_state(s)
        assert np.array_equal(bits32(now[0]), bits32(self.ref.xbar)), what
        same_state(now, self.before, what, skip=(0,))  # ubar, carried refs, warm flags, scratch: untouched
        view = s.robot_frame()
        if self.ref.origin is None:
            assert view is None, what
        else:
            got = view.to_tensor().cpu().numpy()
            assert got.shape == (2, CAP) and np.array_equal(bits64(got), bits64(self.ref.origin)), what


@pytest.mark.parametrize("N", [1, 20])
@pytest.mark.parametrize("model", MODELS)
def test_frame_writers(built, model, N):
    w = Writers(model, N, 31 + N)
    s, ref, rng = w.s, w.ref, w.rng
    mask = (np.arange(B) % 2 == 0).astype(np.uint8)
    dmask = torch.from_numpy(mask).to(DEV)
    w.check("off")
    # the first writer fills with (0, 0): the masked-out robots and those at and past B keep that and their iterate
    origin = fc.per_robot(B).T.copy()
    s.set_robot_frame(t(origin, F64), mask=dmask)
    ref.set(origin, mask)
    w.check("set, masked")
    assert (ref.origin[:, B:] == 0).all() and (ref.origin[:, 1:B:2] == 0).all()
    # every robot, from one origin to another: the move is the difference of the two, rounded once
    origin = np.roll(origin, 1, axis=1) + rng.uniform(-40, 40, origin.shape)
    s.set_robot_frame(t(origin, F64))
    ref.set(origin)
    w.check("set, all")
    # to_frame / from_frame for every array the header lists
    nx, ny = s.nx, s.ny
    for n, c in ((1, 3), (N + 1, 3), (1, nx), (N + 1, ny), (N + 1, 3), (N + 1, nx)):
        m = rng.uniform(-3, 3, (n, c, B))
        m[:, :2] += origin[None]
        got = s.to_frame(t(m, F64))
        torch.cuda.synchronize()
        want = ref.to_frame(m)
        assert got.dtype == torch.float32 and np.array_equal(bits32(got.cpu().numpy()), bits32(want)), (n, c)
        back = s.from_frame(got)
        torch.cuda.synchronize()
        assert back.dtype == F64 and np.array_equal(bits64(back.cpu().numpy()), bits64(ref.from_frame(want))), (n, c)
    pose = rng.uniform(-3, 3, (3, B))
    assert np.array_equal(bits32(s.to_frame(t(pose, F64)).cpu().numpy()), bits32(ref.to_frame(pose[None])[0]))
    # recentre at a radius that moves some robots and not others; a NaN robot, an infinite one, a far one masked out
    pm = origin + rng.uniform(-3, 3, origin.shape)
    pm[0, 3], pm[1, 4], pm[:, 6] = math.nan, math.inf, origin[:, 6] + 50.0
    pm = np.concatenate([pm, rng.uniform(-3, 3, (1, B))])  # (a pose array: the heading row is not read)
    rmask = np.ones(B, np.uint8)
    rmask[6] = 0
    moved = torch.full((B,), 9, dtype=torch.uint8, device=DEV)
    s.recentre(t(pm, F64), 2.0, mask=torch.from_numpy(rmask).to(DEV), moved=moved)
    want = ref.recentre(pm, 2.0, rmask)
    w.check("recentre")
    assert moved.cpu().numpy().tolist() == want.tolist()
    assert 0 < want.sum() < B - 3 and want[3] == want[4] == want[6] == 0
    assert np.array_equal(ref.origin[:, :B][:, want == 1], np.rint(pm[:2][:, want == 1]))
    # a NaN radius moves nothing (and is no argument error); neither does a radius nothing exceeds
    for radius in (math.nan, math.inf, 1e9):
        moved.fill_(9)
        s.recentre(t(pm[:2].copy(), F64), radius, moved=moved)
        assert ref.recentre(pm[:2], radius).sum() == 0 and int(moved.sum()) == 0
        w.check(f"recentre, radius {radius}")
    # clear: the iterate back in map coordinates, the table off; then a fresh writer refills with (0, 0)
    s.clear_robot_frame()
    ref.clear()
    w.check("clear")
    m = rng.uniform(-3, 3, (1, 3, B))
    assert np.array_equal(bits32(s.to_frame(t(m, F64)).cpu().numpy()), bits32(m.astype(np.float32)))  # off: origin 0
    origin = fc.per_robot(B).T[:, ::-1].copy()
    s.set_robot_frame(t(origin, F64), mask=dmask)
    ref.set(origin, mask)
    w.check("refill")
    # a writer for no robot still switches the table on
    s2 = BatchSolver(model, N, CAP, device=DEV)
    s2.recentre(t(np.zeros((2, B)), F64), 1.0)
    assert s2.robot_frame() is not None and (s2.robot_frame().to_tensor() == 0).all()
    s2.clear_robot_frame()
    s2.clear_robot_frame()  # (off already: nothing to do)
    assert s2.robot_frame() is None


def plain(monkeypatch, model, N, cap, form):
    """a handle whose scratch records start as zeros (they are allocated and not cleared, and the launches do not write
    every float of them), so that two handles' whole resident state can be compared"""
    s = make_solver(monkeypatch, model, N, cap, form)
    sv = s.warm_state()[1]
    sv.copy_from(torch.zeros(sv.shape, device=DEV))
    return s


def framed(monkeypatch, model, N, cap, form):
    """such a handle with the mixed origins, its robots placed as the header says: the frame, then init_iterate"""
    s = plain(monkeypatch, model, N, cap, form)
    s.set_robot_frame(t(fc.per_robot(cap).T.copy(), F64))
    s.init_iterate()
    return s


@pytest.mark.parametrize("form", ["team_plain", "seg"])
@pytest.mark.parametrize("model", MODELS)
def test_run_mode_does_not_read_the_table(built, monkeypatch, model, form):
    """the same fp32 inputs through a handle with the frame on (mixed origins) and one with it off: every output and
    the whole resident state (same_resident) bit-identical over 6 ticks, the cold tick and a reset included"""
    N = 20
    on, off = framed(monkeypatch, model, N, B, form), plain(monkeypatch, model, N, B, form)
    assert FORMS[form][2](on.plan_ex(B, "run"))
    a, b = Loop(on, model, B), Loop(off, model, B)
    mask = torch.from_numpy((np.arange(B) % 5 == 0).astype(np.uint8)).to(DEV)
    for tick in range(T):
        rs = mask if tick == RESET_TICK else None
        for loop in (a, b):
            loop.run(reset=rs)
        assert (a.out["status"] == 0).all(), (tick, a.out["status"])
        for k in a.out:
            assert torch.equal(a.out[k], b.out[k]), (tick, k)
        same_resident(on, off, tick, form)
        for loop in (a, b):
            loop.advance()
    assert on.robot_frame() is not None and off.robot_frame() is None


@pytest.mark.parametrize("form", ["team_plain", "seg"])
@pytest.mark.parametrize("model", MODELS)
def test_solve_mode_does_not_read_the_table(built, monkeypatch, model, form):
    N = 20
    o, rec, _ = solve_reference(model, (0.0, 0.0))
    on, off = framed(monkeypatch, model, N, B, form), plain(monkeypatch, model, N, B, form)
    assert FORMS[form][2](on.plan_ex(B, "solve"))
    nx, nu = o.nx, o.nu
    outs = []
    for s in (on, off):
        xv, uv, _ = s.state()
        xv.copy_from(t(np.stack([r[3] for r in rec]).reshape(B, -1).T))
        uv.copy_from(t(np.stack([r[4] for r in rec]).reshape(B, -1).T))
        out = dict(u0=torch.zeros(nu, B, device=DEV), x1=torch.zeros(nx, B, device=DEV),
                   xtraj=torch.zeros((N + 1) * nx, B, device=DEV), utraj=torch.zeros(N * nu, B, device=DEV),
                   status=torch.full((B,), -7, dtype=torch.int32, device=DEV),
                   qp_iter=torch.zeros(B, dtype=torch.int32, device=DEV), qp_res=torch.zeros(3, B, device=DEV))
        outs.append(out)
    mask = torch.from_numpy((np.arange(B) % 5 == 0).astype(np.uint8)).to(DEV)
    x0, yref, We = (t(np.stack([r[0] for r in rec]).T), t(np.stack([r[1] for r in rec]).transpose(1, 2, 0)),
                    t(np.stack([r[2] for r in rec]).T))
    for tick, rs in enumerate((None, mask, None)):
        for s, out in zip((on, off), outs):
            s.solve(x0, yref, We=We, reset=rs, **out)
        torch.cuda.synchronize()
        assert (outs[0]["status"] == 0).all(), (tick, outs[0]["status"])
        for k in outs[0]:
            assert torch.equal(outs[0][k], outs[1][k]), (tick, k)
        same_resident(on, off, tick, form)


@pytest.mark.parametrize("model", MODELS)
def test_recentring_a_running_fleet(built, monkeypatch, model):
    """A 6-tick closed loop on the harness plant under mixed origins. Every third robot starts (5, -7) m from its
    origin, the others within 2.5 m, and before tick 3 nmpc_batch_recentre with a radius of 4 m gives exactly those
    their rounded map position as the new origin. The plant does not follow an origin, so the test moves the moved
    robots' plant state and references itself (from_frame before the call, to_frame after it), and the oracle's fp64
    iterate chain by the same difference. Every tick of every robot stays within 1e-3 of the oracle on the frame
    values the device is given; warm flags survive the move; a twin handle that is never re-centred gives the same
    statuses.

    Measured (MI355X): |u0(re-centred) - u0(twin)| over ticks 3..5 at most 1.43e-06 (diff), 6.11e-07 (omni4),
    1.79e-07 (tric); 0 on ticks 0..2. Printed, not asserted: both are held to the oracle.
    """
    N = 20
    third = np.arange(B) % 3 == 0
    start = np.where(third[:, None], np.array([[5.0, -7.0]]), 0.0)  # where each robot stands in its frame
    origin0 = fc.per_robot(B) - start
    loops, fleets, solvers = [], [], []
    for _ in range(2):
        s = make_solver(monkeypatch, model, N, B, "team_plain")
        s.set_robot_frame(t(origin0.T.copy(), F64))
        s.init_iterate()
        loop = Loop(s, model, B, offset=start)
        solvers.append(s)
        loops.append(loop)
        fleets.append(BatchOracle(model, loop.fl["carried"].T))
    worst = 0.0
    for tick in range(T):
        if tick == RESET_TICK:
            s, loop, fleet = solvers[0], loops[0], fleets[0]
            warm = s.warm_state()[0].to_tensor()
            pose_map, path_map, traj_map = s.from_frame(loop.pose), s.from_frame(loop.path), s.from_frame(loop.traj)
            moved = torch.zeros(B, dtype=torch.uint8, device=DEV)
            s.recentre(pose_map, 4.0, moved=moved)
            assert moved.cpu().numpy().astype(bool).tolist() == third.tolist()
            loop.pose, loop.path, loop.traj = s.to_frame(pose_map), s.to_frame(path_map), s.to_frame(traj_map)
            torch.cuda.synchronize()
            assert torch.equal(s.warm_state()[0].to_tensor(), warm) and int((warm[0, :B] != 0).sum()) > B // 2
            new = s.robot_frame().to_tensor().cpu().numpy()[:, :B].T
            assert np.array_equal(new[third], np.rint(pose_map.cpu().numpy()[:2].T[third]))
            assert np.array_equal(new[~third], origin0[~third])
            fleet.xbar[:, :, :2] += (origin0 - new)[:, None, :]
            assert (np.abs(loop.pose.cpu().numpy()[:2, third]) <= 0.5).all()
        for s, loop, fleet in zip(solvers, loops, fleets):
            inp = loop.host_inputs()
            loop.run()
            check_tick(loop, fleet, inp, tick)
        assert torch.equal(loops[0].out["status"], loops[1].out["status"]), tick
        d = float((loops[0].out["u0"] - loops[1].out["u0"]).abs().max())
        print(f"{model} tick {tick}: |u0(re-centred) - u0(twin)| {d:.2e}")
        if tick >= RESET_TICK:
            worst = max(worst, d)
        for loop in loops:
            loop.advance()
    print(f"{model}: |u0(re-centred) - u0(twin)| over ticks {RESET_TICK}..{T - 1} at most {worst:.2e}")
