"""The numpy oracle of the nearest-point search (tests/path_nearest_ref.py) against brute force and against hand
cases with known answers. CPU only: this checks the checker of tests/test_gpu_path_nearest.py."""
import math

import numpy as np

from tests.path_cases import _line, edge_paths, random_paths
from tests.path_nearest_ref import nearest_one, nearest_ref


def test_oracle_against_brute_force():
    """200 seeded robots anywhere in [-3, 3]^2, 20001 samples per segment: the oracle is never worse than the best
    sample, and the best sample is never worse than the oracle by more than half a sample step of path."""
    B, M = 200, 20001
    segs, nseg, _ = random_paths(B, seed=33)
    pos = np.random.default_rng(5).uniform(-3, 3, (B, 2))
    _, d_or, _, _ = nearest_ref(segs, nseg, pos)
    u = np.linspace(0.0, 1.0, M)
    h = 1.0 / (M - 1)
    pw = np.stack([u ** 0, u, u ** 2, u ** 3])  # [4][M]
    for i in range(B):
        S = segs[i, :nseg[i]]
        x, y = S[:, 0:4] @ pw, S[:, 4:8] @ pw
        d_brute = np.sqrt((x - pos[i, 0]) ** 2 + (y - pos[i, 1]) ** 2).min()
        # |P'| <= |c1| + 2 |c2| + 3 |c3| per coordinate on [0, 1]
        w = np.array([1.0, 2.0, 3.0])
        speed = np.hypot(np.abs(S[:, 1:4]) @ w, np.abs(S[:, 5:8]) @ w).max()
        assert d_or[i] <= d_brute + 1e-12, i
        assert d_brute <= d_or[i] + 0.5 * h * speed, i


def test_point_beside_a_line():
    seg = np.array([_line((0, 0), (2, 0), 0.5)])
    for x in (0.0, 0.3, 1.0, 1.7, 2.0):
        U, d, _, _ = nearest_one(seg, 1, (x, 0.4))
        assert abs(U - x / 2) <= 1e-15 and abs(d - 0.4) <= 1e-15


def test_before_start_and_beyond_end():
    seg = np.array([_line((0, 0), (2, 0), 0.5), _line((2, 0), (4, 0), 0.5)])
    U, d, _, _ = nearest_one(seg, 2, (-1.0, 0.5))
    assert U == 0.0 and abs(d - math.hypot(1.0, 0.5)) <= 1e-15
    U, d, _, _ = nearest_one(seg, 2, (5.0, -0.5))
    assert U == 2.0 and abs(d - math.hypot(1.0, 0.5)) <= 1e-15


def test_l_shaped_path():
    segs, nseg, _, names = edge_paths()
    i = names.index("speed_change")
    U, d, _, _ = nearest_one(segs[i], int(nseg[i]), (0.6, 0.2))
    assert abs(U - 1.4) <= 1e-15 and abs(d - 0.1) <= 1e-15


def test_range_excludes_the_global_minimum():
    segs, nseg, _, names = edge_paths()
    i = names.index("speed_change")
    # the third leg from x = 0.5: beyond U = 2 the nearest point is the start of that leg
    U, d, _, _ = nearest_one(segs[i], int(nseg[i]), (0.6, 0.2), (2.0, math.nan))
    assert abs(U - (2.0 + 0.1 / 1.5)) <= 1e-15 and abs(d - 0.3) <= 1e-15
    # only the first leg: its end is the nearest point in range
    U, d, _, _ = nearest_one(segs[i], int(nseg[i]), (0.6, 0.2), (math.nan, 0.9))
    assert abs(U - 0.9) <= 1e-15 and abs(d - math.hypot(0.15, 0.2)) <= 1e-15
    # lo > hi collapses to lo
    U, _, _, _ = nearest_one(segs[i], int(nseg[i]), (0.6, 0.2), (2.5, 1.0))
    assert U == 2.5
