"""The restatement of fleet separation (tests/separation_ref.py) by hand: one robot that drives along +x from the
origin, 0.1 m per stage (or stands), and a few static tracks (K = 0) placed on each edge of the rule; and the rule in
the fp64 oracle's closed loop on the convoy of tests/separation_cases.py. CPU only."""
import numpy as np
import pytest

from tests import separation_cases as cs
from tests import separation_ref as sp
from tests import speed_map_ref as sr

F32 = np.float32
N = 4
CAP, ACC, DT = F32(1.0), F32(1.0), 0.05  # g = 0.8 * 1 * 0.05 = 0.04


def robot(moving=True):
    pos = np.zeros((N + 1, 2, 1), F32)
    if moving:
        pos[:, 0, 0] = F32(0.1) * np.arange(N + 1, dtype=F32)
    return pos


def tracks(*points):
    return np.array(points, np.float64).T[None].copy()  # [1][2][M]


def counts_at0(points, moving=True, **kw):
    pos = robot(moving)
    _, c = sp.pairs(pos, sp.headings(pos), tracks(*points), **kw)
    return c[0, 0].tolist()


def lim_gap(xy, m=None, moving=True, carried=0.0, **kw):
    pos = robot(moving)
    return sp.limits(pos, xy, CAP, ACC, DT, np.full((1, 1), carried, F32), 1, m=m, **kw)


def test_range_edge():
    """a track exactly at range counts, one ulp (of the fp32 difference) beyond does not"""
    beyond = float(np.nextafter(F32(3.0), F32(np.inf)))
    assert counts_at0([(3.0, 0.0), (beyond, 0.0)]) == [True, False]
    assert counts_at0([(0.0, 3.0), (0.0, -beyond)], moving=False) == [True, False]


def test_half_plane():
    """exactly abeam (dot = 0) does not count; behind does not count, and does with ahead_only = 0"""
    pts = [(0.0, 1.0), (-1.0, 0.5), (1.0, 0.5)]
    assert counts_at0(pts) == [False, False, True]
    assert counts_at0(pts, ahead_only=0) == [True, True, True]


def test_standing_robot_counts_everything():
    pts = [(0.0, 1.0), (-1.0, 0.5), (1.0, 0.5)]
    assert counts_at0(pts, moving=False) == [True, True, True]
    pos = robot()
    h = sp.headings(pos, reset=np.ones(1))  # a reset robot has no direction either
    assert (h == 0).all()
    assert sp.pairs(pos, h, tracks(*pts))[1][0, 0].tolist() == [True, True, True]


def test_headings_clamp_at_both_ends():
    p = robot()
    h = sp.headings(p)
    assert np.array_equal(h[:N], p[1:] - p[:-1]) and np.array_equal(h[N], p[N] - p[N - 1])


def test_own_track_is_skipped():
    """coincident with the robot (q = 0, which a standing robot would count) and skipped by its index"""
    xy = tracks((0.0, 0.0), (2.0, 0.0))
    _, gap = lim_gap(xy, moving=False, own_first=0)
    assert gap[0, 0] == F32(2.0)
    _, gap = lim_gap(xy, moving=False, own_first=-1)
    assert gap[0, 0] == F32(0.0)


def test_nan_and_infinite_tracks_never_count():
    xy = tracks((np.nan, 0.0), (1.0, np.nan), (np.inf, 0.0), (0.0, -np.inf), (1e300, 0.0))
    lim, gap = lim_gap(xy, moving=False)
    assert np.isposinf(gap).all()
    assert (lim == CAP).all()


def test_cap_and_floor_by_hand():
    """one track 1 m ahead of a standing robot: s = 1 * (1 - 0.6) = 0.4 at every stage; at 0.5 m: below the floor"""
    lim, gap = lim_gap(tracks((1.0, 0.0)), moving=False)
    assert (gap == F32(1.0)).all() and (lim == F32(1.0) * (F32(1.0) - F32(0.6))).all()
    lim, _ = lim_gap(tracks((0.5, 0.0)), moving=False)
    assert (lim == F32(0.05)).all()
    # the carried speed stays reachable: lim_k = max(r_k, c - k g)
    lim, _ = lim_gap(tracks((0.5, 0.0)), moving=False, carried=0.5)
    g = (F32(0.8) * ACC) * F32(DT)
    assert np.array_equal(lim[:, 0], np.fmax(F32(0.05), F32(0.5) - np.arange(N + 1, dtype=F32) * g))


def test_nan_cell_with_a_near_track_is_the_floor():
    m = sr.Map(-1.0, -1.0, 2.0, np.full((1, 1), np.nan, F32))
    lim, gap = lim_gap(tracks((1.0, 0.0)), m=m, moving=False)
    assert (gap == F32(1.0)).all() and (lim == F32(0.05)).all()
    # and a cell below the separation cap wins, one above it loses
    for cell, want in ((0.2, 0.2), (0.7, F32(1.0) * (F32(1.0) - F32(0.6)))):
        lim, _ = lim_gap(tracks((1.0, 0.0)), m=sr.Map(-1.0, -1.0, 2.0, np.full((1, 1), cell, F32)), moving=False)
        assert (lim == F32(want)).all()


def test_no_tracks_is_the_map_only_rule():
    rng = np.random.default_rng(5)
    B = 7
    pos = rng.uniform(-2, 2, (N + 1, 2, B)).astype(F32)
    cap, acc = rng.uniform(0.3, 0.9, B).astype(F32), rng.uniform(0.5, 1.5, B).astype(F32)
    car = rng.uniform(-0.6, 0.6, (2, B)).astype(F32)
    v = rng.uniform(0.1, 0.9, (5, 6)).astype(F32)
    v[1, 2] = np.nan
    m = sr.Map(-1.5, -1.25, 0.5, v, outside=0.3)
    want = sr.limits(m, pos, cap, acc, DT, car, 2)
    for xy in (None, np.zeros((3, 2, 0))):
        lim, gap = sp.limits(pos, xy, cap, acc, DT, car, 2, m=m)
        assert np.array_equal(lim.view(np.uint32), want.view(np.uint32)) and np.isposinf(gap).all()
    far = np.full((1, 2, 3), 50.0)  # tracks, but none in range
    lim, _ = sp.limits(pos, far, cap, acc, DT, car, 2, m=m)
    assert np.array_equal(lim.view(np.uint32), want.view(np.uint32))
    lim, _ = sp.limits(pos, None, cap, acc, DT, car, 2)  # no map either: the cap, corrected by c
    c = np.abs(car).max(axis=0)
    g = (F32(0.8) * acc) * F32(DT)
    assert np.array_equal(lim, np.fmax(cap[None], c[None] - np.arange(N + 1, dtype=F32)[:, None] * g[None]))


def test_export_by_hand():
    nx, B, cap = 3, 4, 5
    xbar = np.arange((N + 1) * nx * cap, dtype=F32).reshape((N + 1) * nx, cap)
    origin = np.array([[100.0] * cap, [200.0] * cap])
    pose = np.full((3, B), -1.0, F32)
    xy = np.full((7, 2, 9), -7.0)
    sp.export(xy, 2, xbar, nx, N, B, origin, pose, reset=[0, 1, 0, 0], mode=[1, 1, 2, 0])
    assert (xy[:, :, :2] == -7).all() and (xy[:, :, 6:] == -7).all()
    assert xy[1, 0, 2] == float(xbar[nx, 0]) + 100 and xy[1, 1, 2] == float(xbar[nx + 1, 0]) + 200
    assert (xy[5:, 0, 4] == float(xbar[N * nx, 2]) + 100).all()          # stages past N repeat stage N
    assert (xy[:, 0, 3] == 99).all() and (xy[:, 1, 5] == 199).all()      # reset, and IDLE: the pose


# ---- the rule in the fp64 oracle's closed loop: the convoy ---------------------------------------------------------
@pytest.mark.parametrize("model", ["diff", "omni4"])
def test_convoy_in_closed_loop(built, model):
    """Measured: smallest centre distance 0.0005 (diff) / 0.003 (omni4) with the rule off, 0.794 / 0.765 with it on; the
    last 40 ticks lie in [0.801, 0.806] / [0.773, 0.785] around clearance + 0.2 / gain = 0.8."""
    off, on = cs.closed_loop(model, False), cs.closed_loop(model, True)
    print(f"{model}: rule off min {off['dist'].min():.4f}; on min {on['dist'].min():.4f}, last 40 ticks "
          f"[{on['dist'][-40:].min():.4f}, {on['dist'][-40:].max():.4f}]")
    assert (off["status"] == 0).all() and (on["status"] == 0).all()
    cs.distances_ok(off["dist"], False)
    cs.distances_ok(on["dist"], True)
    assert (on["lim1"][-40:, 1] < 0.5).all() and np.isfinite(on["lim1"]).all()  # (the follower's limit binds)
