"""GPU tests of the nearest-point search (nmpc_path_nearest, csrc/path_nearest.hip) and of the whole FollowPath tick
built on it (nmpc_batch_follow_path), against the fp64 numpy oracle of tests/path_nearest_ref.py.

Bars (bar 1 below), for every robot: d_gpu <= d_ref + 1e-9 m and d_gpu >= d_ref - 1e-12 m, where d_gpu is the distance
from the robot to the path point at the returned parameter, evaluated on the host; |U_gpu - U_ref| <= 1e-9 on the
robots whose answer is separated (distance gap to any other candidate >= 1e-6 m) and well conditioned (g'/|P'|^2 >=
0.05), a filter that may drop at most 2 % of the robots; near and err equal the oracle's at U_gpu to 1e-12.
"""
import functools
import math

import numpy as np
import pytest
import torch

from nmpc_nav_control_amd._lib import check, lib
from nmpc_nav_control_amd.batch import BatchSolver
from nmpc_nav_control_amd.path import PathMinDist, PathSegment, nearest, pack_paths
from tests.path_cases import _line, edge_paths, random_paths
from tests.path_nearest_ref import dist_at, near_err, nearest_one, nearest_ref, path_point

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def dev(a, dtype=None):
    t = torch.from_numpy(np.array(a, order="C")).to(DEV)  # (a writable, contiguous copy)
    return t if dtype is None else t.to(dtype)


def gpu_nearest(segs, nseg, pose, u_range=None, holo=False):
    """pose [B][3] float32 -> U [B], near [B][4], err [B][2] (numpy)"""
    B = len(nseg)
    near = torch.empty((4, B), dtype=torch.float64, device=DEV)
    err = torch.empty((2, B), dtype=torch.float64, device=DEV)
    U = nearest(dev(segs), dev(nseg), dev(pose.T), None if u_range is None else dev(u_range), holo, near, err)
    torch.cuda.synchronize()
    return U.cpu().numpy(), near.cpu().numpy().T, err.cpu().numpy().T


def wrap_diff(a, b):
    return np.abs(np.angle(np.exp(1j * (a - b))))


def check_bar1(segs, nseg, pose, got, ref, u_range=None, holo=False, max_excluded=0.02):
    U, near, err = got
    Ur, dr, gap, cond = ref
    pos = pose[:, :2].astype(np.float64)
    d = dist_at(segs, nseg, U, pos)
    print("d_gpu - d_ref: max %.3e min %.3e" % ((d - dr).max(), (d - dr).min()))
    assert (d <= dr + 1e-9).all(), (d - dr).max()
    assert (d >= dr - 1e-12).all(), (d - dr).min()
    ok = (gap >= 1e-6) & (cond >= 0.05)
    print("excluded %d of %d; |U_gpu - U_ref| max %.3e" % ((~ok).sum(), len(ok), np.abs(U - Ur)[ok].max(initial=0.0)))
    assert (~ok).sum() <= max_excluded * len(ok)
    assert (np.abs(U - Ur)[ok] <= 1e-9).all()
    if u_range is not None:
        lo = np.where(np.isnan(u_range[0]), 0.0, u_range[0])
        assert (U >= lo).all()
    for i in range(len(nseg)):
        en, ee = near_err(segs[i], int(nseg[i]), U[i], pose[i].astype(np.float64), holo)
        assert np.abs(near[i, :2] - en[:2]).max() <= 1e-12 and abs(near[i, 3] - en[3]) <= 1e-12, i
        assert wrap_diff(near[i, 2], en[2]) <= 1e-12, i
        assert abs(err[i, 0] - ee[0]) <= 1e-12 and wrap_diff(err[i, 1], ee[1]) <= 1e-12, i


@functools.lru_cache(maxsize=None)
def parity_case(which):
    """the 1500 seeded robots: 'far' anywhere in [-3, 3]^2, 'near' within 0.15 m of their path around the seeded
    nearest_u; poses (fp32) and the oracle's answer, computed once"""
    B = 1500
    segs, nseg, nu = random_paths(B, seed=33)
    rng = np.random.default_rng(5)
    pos = rng.uniform(-3, 3, (B, 2))
    if which == "near":
        pos = np.array([path_point(segs[i], int(nseg[i]), nu[i]) for i in range(B)]) + rng.uniform(-0.15, 0.15, (B, 2))
    pose = np.concatenate([pos, rng.uniform(-math.pi, math.pi, (B, 1))], 1).astype(np.float32)
    ref = nearest_ref(segs, nseg, pose[:, :2].astype(np.float64))
    for a in (segs, nseg, nu, pose) + ref:
        a.setflags(write=False)
    return segs, nseg, nu, pose, ref


@pytest.mark.parametrize("which", ["far", "near"])
def test_parity(built, which):
    segs, nseg, _, pose, ref = parity_case(which)
    check_bar1(segs, nseg, pose, gpu_nearest(segs, nseg, pose), ref)


@pytest.mark.parametrize("one_seg", [False, True])
def test_small_shapes(built, one_seg):
    """B in {1, 3, 5, 64, 257}, every robot checked; a segment stride beyond every nseg (the records past a robot's
    own are NaN: reading one would spoil its answer); results bit-identical across B and with the batch reversed."""
    Bmax = 257
    s4, nseg, _ = random_paths(Bmax, seed=71, max_segs=4)
    if one_seg:
        nseg = np.ones(Bmax, np.int32)
    segs = np.full((Bmax, 6, 16), np.nan)
    for i in range(Bmax):
        segs[i, :nseg[i]] = s4[i, :nseg[i]]
    rng = np.random.default_rng(72)
    pose = np.concatenate([rng.uniform(-3, 3, (Bmax, 2)), rng.uniform(-3, 3, (Bmax, 1))], 1).astype(np.float32)
    ref = nearest_ref(segs, nseg, pose[:, :2].astype(np.float64))
    full = gpu_nearest(segs, nseg, pose)
    check_bar1(segs, nseg, pose, full, ref)
    for B in (1, 3, 5, 64):
        got = gpu_nearest(segs[:B], nseg[:B], pose[:B])
        for g, f in zip(got, full):
            np.testing.assert_array_equal(g, f[:B], err_msg=f"B={B}")
    rev = gpu_nearest(segs[::-1], nseg[::-1], pose[::-1])
    for g, f in zip(rev, full):
        np.testing.assert_array_equal(g[::-1], f)


def test_empty_batch(built):
    assert lib().nmpc_path_nearest(0, None, 1, None, None, None, 0, None, None, None, None) == 0


def test_edge_paths(built):
    segs, nseg, _, names = edge_paths()
    B = len(nseg)
    pose = np.tile(np.array([[0.6, 0.2, 0.3]], np.float32), (B, 1))
    ref = nearest_ref(segs, nseg, pose[:, :2].astype(np.float64))
    got = gpu_nearest(segs, nseg, pose)
    check_bar1(segs, nseg, pose, got, ref)
    x, y = float(pose[0, 0]), float(pose[0, 1])  # the fp32 pose
    i = names.index("speed_change")
    assert abs(got[0][i] - (1.0 + y / 0.5)) <= 1e-9 and abs(got[2][i, 0] - (x - 0.5)) <= 1e-9
    i = names.index("degenerate_point")  # a point at (1, 2), then the straight line
    assert abs(got[0][i] - (1.0 + x / 2.0)) <= 1e-9
    i = names.index("zero_speed")
    assert abs(got[0][i] - (x + y) / 2.0) <= 1e-9


def test_range_lower_bound(built):
    """u_range = {seeded nearest_u, NaN}: never behind the bound, and bar 1 against the oracle in that range"""
    segs, nseg, nu, pose, _ = parity_case("near")
    B = 400
    segs, nseg, nu, pose = segs[:B], nseg[:B], nu[:B], pose[:B]
    ur = np.stack([nu, np.full(B, np.nan)])
    ref = nearest_ref(segs, nseg, pose[:, :2].astype(np.float64), ur)
    got = gpu_nearest(segs, nseg, pose, ur)
    assert (got[0] >= nu).all()
    check_bar1(segs, nseg, pose, got, ref, ur)


def test_range_upper_bound_and_lo_above_hi(built):
    segs, nseg, _, names = edge_paths()
    i = names.index("speed_change")
    S, n = np.tile(segs[i], (4, 1, 1)), np.full(4, nseg[i], np.int32)
    pose = np.tile(np.array([[0.6, 0.2, 0.0]], np.float32), (4, 1))
    ur = np.array([[2.0, math.nan, 2.5, -1.0], [math.nan, 0.9, 1.0, 7.0]])
    U, _, err = gpu_nearest(S, n, pose, ur)
    x, y = float(pose[0, 0]), float(pose[0, 1])  # the fp32 pose
    assert abs(U[0] - (2.0 + (x - 0.5) / 1.5)) <= 1e-9 and abs(err[0, 0] - (0.5 - y)) <= 1e-9
    assert U[1] == 0.9 and abs(err[1, 0] - math.hypot(x - 0.45, y)) <= 1e-9
    assert U[2] == 2.5  # lo > hi: hi = lo
    assert abs(U[3] - (1.0 + y / 0.5)) <= 1e-9  # bounds clamped into [0, n]


def test_tie_goes_to_the_smaller_parameter(built):
    """the robot on the bisector of a symmetric V is equally far from both legs (every operation is exact here)"""
    V = np.zeros((1, 2, 16))
    V[0, 0], V[0, 1] = _line((-1, 1), (0, 0), 0.5), _line((0, 0), (1, 1), 0.5)
    U, _, err = gpu_nearest(V, np.array([2], np.int32), np.array([[0.0, 1.0, 0.0]], np.float32))
    assert U[0] == 0.5 and abs(err[0, 0] - math.sqrt(0.5)) <= 1e-12
    # from U = 0.75 on, the second leg's foot point is the nearer one
    ur = np.array([[0.75], [math.nan]])
    U, _, _ = gpu_nearest(V, np.array([2], np.int32), np.array([[0.0, 1.0, 0.0]], np.float32), ur)
    assert U[0] == 1.5


def test_nan_pose_stays_on_its_robot(built):
    segs, nseg, nu, pose, _ = parity_case("near")
    B = 8
    segs, nseg, pose = segs[:B], nseg[:B], pose[:B].copy()
    ur = np.stack([nu[:B] * 0.5, np.full(B, np.nan)])
    clean = gpu_nearest(segs, nseg, pose, ur)
    for col in range(3):
        bad = pose.copy()
        bad[2, col] = np.nan
        got = gpu_nearest(segs, nseg, bad, ur)
        assert got[0][2] == ur[0, 2] and np.isnan(got[2][2]).all(), col
        keep = np.arange(B) != 2
        for g, c in zip(got, clean):
            np.testing.assert_array_equal(g[keep], c[keep])
    # NaN coefficients, and a robot without a path
    S = segs.copy()
    S[3, :, 5] = np.nan
    n = nseg.copy()
    n[5] = 0
    got = gpu_nearest(S, n, pose, ur)
    assert got[0][3] == ur[0, 3] and np.isnan(got[2][3]).all()
    assert got[0][5] == 0.0 and np.isnan(got[2][5]).all() and np.isnan(got[1][5]).all()
    keep = (np.arange(B) != 3) & (np.arange(B) != 5)
    for g, c in zip(got, clean):
        np.testing.assert_array_equal(g[keep], c[keep])


def test_reverse_and_holonomic_heading(built):
    """a segment driven backwards (v < 0) adds pi to the heading of the orientation error; holonomic_heading takes
    GetThetaHolomonic instead"""
    fwd, rev = _line((0, 0), (2, 0), 0.5, 0.7, 0.9), _line((0, 0), (2, 0), -0.5, 0.7, 0.9)
    S = np.array([[fwd], [rev]])
    n = np.ones(2, np.int32)
    pose = np.array([[0.5, 0.3, 0.25], [0.5, 0.3, 0.25]], np.float32)
    th = float(pose[0, 2])
    U, near, err = gpu_nearest(S, n, pose)
    assert np.abs(U - 0.25).max() <= 1e-9 and np.abs(near[:, 2]).max() <= 1e-15  # the raw theta: no pi
    assert abs(err[0, 1] - th) <= 1e-12 and abs(err[1, 1] - (math.pi - th)) <= 1e-12
    U, near, err = gpu_nearest(S, n, pose, holo=True)
    assert np.abs(near[:, 3] - 0.75).max() <= 1e-9 and np.abs(err[:, 1] - (0.75 - th)).max() <= 1e-9
    segs, nseg, _, pose, ref = parity_case("near")
    B = 300  # seeded paths, a fifth of them reversed
    check_bar1(segs[:B], nseg[:B], pose[:B], gpu_nearest(segs[:B], nseg[:B], pose[:B], holo=True),
               tuple(r[:B] for r in ref), holo=True)


def test_reference_mirror_GetMinDist(built):
    path = [PathSegment.line((0, 0), (1, 0), 0.5), PathSegment.arc(1, 0.5, 0.5, -math.pi / 2, 0.0, 0.5)]
    x, y, th = np.float32(1.3), np.float32(0.3), 0.1
    u, nx, ny, nth, nthh = PathMinDist().GetMinDist(path, x, y, th)
    segs, nseg = pack_paths([path])
    Ur, dr, _, _ = nearest_one(segs[0], 2, (float(x), float(y)))
    assert abs(u - Ur) <= 1e-9 and 1.0 < u < 2.0
    en, _ = near_err(segs[0], 2, u, (float(x), float(y), th))
    assert max(abs(nx - en[0]), abs(ny - en[1]), abs(nth - en[2]), abs(nthh - en[3])) <= 1e-12
    assert abs(math.hypot(nx - float(x), ny - float(y)) - dr) <= 1e-9


def follow_case(B, seed, max_segs=4):
    """robots near the start of seeded forward paths, heading along them (as test_gpu_path.py's tick tests)"""
    rng = np.random.default_rng(seed)
    segs, nseg, nu = random_paths(B, seed=seed, max_segs=max_segs, reverse_frac=0.0)
    nu[:] = rng.uniform(0, 0.3, B)
    pose = np.zeros((B, 3))
    for i in range(B):
        en, _ = near_err(segs[i], int(nseg[i]), nu[i], (0.0, 0.0, 0.0))
        pose[i] = en[:3]
    normal = np.stack([-np.sin(pose[:, 2]), np.cos(pose[:, 2])], 1)
    pose[:, :2] += rng.uniform(-0.1, 0.1, (B, 2))
    pose[:, 2] += rng.uniform(-0.2, 0.2, B)
    vel = np.zeros((B, 3))
    vel[:, 0] = rng.uniform(0.0, 0.5, B)
    return segs, nseg, pose, vel, normal


class Outs:
    def __init__(self, B, nu=2):
        z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=DEV)  # noqa: E731
        self.u0, self.cmd, self.traj = z(nu, B), z(3, B), z(41, 3, B)
        self.status, self.qp_iter = z(B, dt=torch.int32), z(B, dt=torch.int32)
        self.path_u, self.err, self.off = z(B, dt=torch.float64), z(2, B, dt=torch.float64), z(B, dt=torch.uint8)

    def kw(self):
        return dict(traj_out=self.traj, cmd=self.cmd, u0=self.u0, status=self.status, qp_iter=self.qp_iter)

    def same(self, o, rows=None):
        r = slice(None) if rows is None else rows
        return all(torch.equal(a[..., r], b[..., r]) for a, b in
                   ((self.path_u, o.path_u), (self.traj, o.traj), (self.u0, o.u0), (self.cmd, o.cmd),
                    (self.status, o.status), (self.qp_iter, o.qp_iter)))


def test_follow_path_equals_its_parts(built):
    """diff N = 40, B = 256, three ticks: follow_path with the checks off against nearest + run_path on a second
    handle, bit for bit; with max_pos_err = 0.5 the eight robots put 1 m beside their path are flagged and stopped
    and every other robot is untouched."""
    N, B = 40, 256
    segs, nseg, pose, vel, normal = follow_case(B, 5)
    moved = np.arange(8) * 31 + 3
    for i in moved:  # to the side that is further from the whole path
        side = [nearest_one(segs[i], int(nseg[i]), np.float32(pose[i, :2] + s * normal[i]).astype(np.float64))[1]
                for s in (1.0, -1.0)]
        pose[i, :2] += (1.0 if side[0] >= side[1] else -1.0) * normal[i]
        assert max(side) >= 0.6
    pose32 = pose.astype(np.float32)
    d_ref = nearest_ref(segs, nseg, pose32[:, :2].astype(np.float64))[1]
    assert ((d_ref >= 0.5) == np.isin(np.arange(B), moved)).all()
    P, V, S, NS = dev(pose32.T), dev(vel.T, torch.float32), dev(segs), dev(nseg)
    whole, parts, guarded = (BatchSolver("diff", N, B, device=DEV) for _ in range(3))
    ow, op, og = Outs(B), Outs(B), Outs(B)
    nan_hi = torch.full((B,), math.nan, dtype=torch.float64, device=DEV)
    others = torch.from_numpy(np.flatnonzero(~np.isin(np.arange(B), moved))).to(DEV)
    for tick in range(3):
        whole.follow_path(P, V, S, NS, ow.path_u, 1 / 40, err=ow.err, off_path=ow.off, **ow.kw())
        op.path_u = nearest(S, NS, P, torch.stack([op.path_u, nan_hi]), err=op.err)
        parts.run_path(P, V, S, NS, op.path_u, 1 / 40, **op.kw())
        guarded.follow_path(P, V, S, NS, og.path_u, 1 / 40, max_pos_err=0.5, err=og.err, off_path=og.off, **og.kw())
        torch.cuda.synchronize()
        assert ow.same(op) and torch.equal(ow.err, op.err), tick
        assert (ow.off == 0).all(), tick
        off = og.off.cpu().numpy()
        assert (off == np.isin(np.arange(B), moved)).all(), tick
        assert (og.cmd[:, dev(moved)] == 0).all() and (ow.cmd[:, dev(moved)] != 0).any(), tick
        assert og.same(ow, others) and torch.equal(og.err, ow.err), tick
        assert torch.equal(og.u0, ow.u0) and torch.equal(og.traj, ow.traj), tick  # only the command is stopped
    assert (ow.status[others] == 0).all()
    np.testing.assert_allclose(ow.err[0].cpu().numpy(), d_ref, rtol=0, atol=1e-9)


def test_follow_path_omni4_uses_the_holonomic_heading(built):
    N, B = 40, 16
    segs, nseg, pose, vel, _ = follow_case(B, 17)
    pose32 = pose.astype(np.float32)
    s = BatchSolver("omni4", N, B, device=DEV)
    o = Outs(B, nu=4)
    s.follow_path(dev(pose32.T), dev(vel.T, torch.float32), dev(segs), dev(nseg), o.path_u, 1 / 40, err=o.err,
                  max_ori_err=math.nan, **o.kw())
    torch.cuda.synchronize()
    U, err = o.path_u.cpu().numpy(), o.err.cpu().numpy()
    differs = 0
    for i in range(B):
        _, eh = near_err(segs[i], int(nseg[i]), U[i], pose32[i].astype(np.float64), True)
        _, et = near_err(segs[i], int(nseg[i]), U[i], pose32[i].astype(np.float64), False)
        assert abs(err[0, i] - eh[0]) <= 1e-12 and wrap_diff(err[1, i], eh[1]) <= 1e-12, i
        differs += abs(eh[1] - et[1]) > 1e-3
    assert differs >= B // 2


def test_closed_loop_without_a_host_parameter(built):
    """diff N = 40, 64 robots on three-segment paths, 40 ticks of follow_path with path_u fed back and the unicycle
    integrated on the device from cmd: no path parameter ever comes from the host."""
    N, B, dt = 40, 64, 1 / 40
    rng = np.random.default_rng(23)
    segs, nseg, _ = random_paths(400, seed=23, max_segs=3, reverse_frac=0.0)
    pick = np.flatnonzero(nseg == 3)[:B]
    assert len(pick) == B
    segs, nseg = np.ascontiguousarray(segs[pick]), nseg[pick]
    u_start = rng.uniform(0, 0.3, B)
    pose = np.array([near_err(segs[i], 3, u_start[i], (0.0, 0.0, 0.0))[0][:3] for i in range(B)])
    P, V = dev(pose.T, torch.float32), torch.zeros(3, B, device=DEV)
    S, NS = dev(segs), dev(nseg)
    s = BatchSolver("diff", N, B, device=DEV)
    o = Outs(B)
    failed = torch.zeros((), dtype=torch.bool, device=DEV)
    back = torch.zeros((), dtype=torch.bool, device=DEV)
    for tick in range(1, 41):
        before = o.path_u.clone()
        s.follow_path(P, V, S, NS, o.path_u, dt, err=o.err, **o.kw())
        failed |= (o.status != 0).any()
        back |= (o.path_u < before).any()
        if tick % 10 == 0:
            torch.cuda.synchronize()
            pose_h, lo = P.cpu().numpy().T.copy(), before.cpu().numpy()
            ur = np.stack([lo, np.full(B, np.nan)])
            ref = nearest_ref(segs, nseg, pose_h[:, :2].astype(np.float64), ur)
            U = o.path_u.cpu().numpy()
            d = dist_at(segs, nseg, U, pose_h[:, :2].astype(np.float64))
            assert (d <= ref[1] + 1e-9).all() and (d >= ref[1] - 1e-12).all(), tick
            ok = (ref[2] >= 1e-6) & (ref[3] >= 0.05)
            assert (~ok).sum() <= 0.02 * B and (np.abs(U - ref[0])[ok] <= 1e-9).all(), tick
            np.testing.assert_allclose(o.err[0].cpu().numpy(), d, rtol=0, atol=1e-12)
        v, w = o.cmd[0], o.cmd[1]
        P = torch.stack([P[0] + v * torch.cos(P[2]) * dt, P[1] + v * torch.sin(P[2]) * dt, P[2] + w * dt])
        V = torch.stack([v, torch.zeros_like(v), w])
    torch.cuda.synchronize()
    assert not bool(failed) and not bool(back)
    assert (o.path_u.cpu().numpy() > u_start).all()


def test_argument_errors(built):
    B = 4
    S = torch.zeros((B, 2, 16), dtype=torch.float64, device=DEV)
    n = torch.ones(B, dtype=torch.int32, device=DEV)
    P = torch.zeros((3, B), dtype=torch.float32, device=DEV)
    U = torch.zeros(B, dtype=torch.float64, device=DEV)
    vp = lambda t: t.data_ptr()  # noqa: E731
    L = lib()
    with pytest.raises(RuntimeError, match="seg_stride"):
        check(L.nmpc_path_nearest(B, vp(S), 0, vp(n), vp(P), None, 0, vp(U), None, None, None))
    with pytest.raises(RuntimeError, match="nearest_u"):
        check(L.nmpc_path_nearest(B, vp(S), 2, vp(n), vp(P), None, 0, None, None, None, None))
    s = BatchSolver("diff", 40, B, device=DEV)
    for bad in (math.nan, math.inf):
        with pytest.raises(RuntimeError, match="sample_period"):
            s.follow_path(P, P.clone(), S, n, U, bad)
    with pytest.raises(RuntimeError, match="seg_stride"):
        check(L.nmpc_batch_follow_path(s._h, B, vp(P), vp(P), None, vp(S), 0, vp(n), vp(U), 0.025, 0, math.inf,
                                       math.inf, None, None, None, None, None, None, None, None, None, None))
    with pytest.raises(RuntimeError, match="path_u"):
        check(L.nmpc_batch_follow_path(s._h, B, vp(P), vp(P), None, vp(S), 2, vp(n), None, 0.025, 0, math.inf,
                                       math.inf, None, None, None, None, None, None, None, None, None, None))
