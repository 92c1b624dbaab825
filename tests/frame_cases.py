"""Offsets and moved tables of the per-robot map frame tests (nmpc_batch_set_robot_frame): tests/test_frame_cases.py
shows on the CPU that they are a valid instrument, tests/test_gpu_frame*.py run them on the device. Host side only.

A robot's origin is its offset: its fp32 positions are the origin fleet's own values (frame values), its fp64 path
segments are the origin fleet's moved by the offset in fp64 (map coordinates). OFFSETS reaches a UTM-sized projected
coordinate and, in x, the last binade in which fp32 still counts whole metres; the four are mixed robot by robot, so
every wave and every 16-lane row holds all of them.
"""
import math

import numpy as np

from tests.path_cases import edge_paths
from tests.path_nearest_ref import near_err

OFFSETS = [(0.0, 0.0), (131072.0, -65536.0), (500000.0, 4649776.0), (-8388608.0, 3.0)]
LARGEST = OFFSETS[2:]  # the two largest


def off_id(off):
    return f"{off[0]:g}_{off[1]:g}"


def per_robot(B):
    """[B][2]: robot i's offset, OFFSETS[i mod 4]"""
    return np.array([OFFSETS[i % len(OFFSETS)] for i in range(B)], np.float64)


def move_segs(segs, off):
    """nmpc_path_segment records [...][16] moved by off ([2], or [B][2] for records [B][S][16]): the constant
    coefficients of x and y, in fp64; everything else (and every NaN record) stays"""
    off = np.asarray(off, np.float64)
    out = np.array(segs, np.float64, copy=True)
    if off.ndim == 2:
        off = off[:, None, :]
    out[..., 0] += off[..., 0]
    out[..., 4] += off[..., 1]
    return out


def to_map(pose, off):
    """fp32 frame poses [B][3] (or [3]) at the map: the fp32 value widened, plus the offset, in fp64: what the device
    forms as (double)pose + origin"""
    out = np.asarray(pose, np.float32).astype(np.float64)
    off = np.asarray(off, np.float64)
    out[..., 0] += off[..., 0]
    out[..., 1] += off[..., 1]
    return out


def fleet64(fl, off):
    """A scenario.make_fleet dict in fp64 map coordinates at offset off: pose x and y and path x0 and y0 moved, every
    array widened (an fp32 fleet cannot stand at these offsets: the ulp is 0.5 m at 4.6e6 m)"""
    out = {k: np.asarray(v, np.float64 if np.issubdtype(np.asarray(v).dtype, np.floating) else None).copy()
           for k, v in fl.items()}
    for k in ("pose", "path"):
        out[k][0] += off[0]
        out[k][1] += off[1]
    return out


def edge_fleet(copies=2):
    """path_cases.edge_paths() with a robot for every path, 3 cm beside the path point at the case's nearest_u, its
    heading 0.1 rad off, 0.2 m/s; `copies` times over, so that with an odd number of paths (11) every path meets two
    offsets. Returns segs [B][3][16], nseg [B], nearest_u [B], names, pose [B][3] (fp32), vel [B][3] (fp32)."""
    segs, nseg, nu, names = edge_paths()
    n = len(nseg)
    pose = np.zeros((n, 3), np.float32)
    for i in range(n):
        near, _ = near_err(segs[i], int(nseg[i]), min(max(nu[i], 0.0), float(nseg[i])), (0.0, 0.0, 0.0))
        pose[i] = (near[0] + 0.03 * math.sin(0.7 * i), near[1] + 0.03 * math.cos(0.7 * i), near[2] + 0.1)
    vel = np.zeros((n, 3), np.float32)
    vel[:, 0] = 0.2
    k = copies
    return (np.tile(segs, (k, 1, 1)), np.tile(nseg, k), np.tile(nu, k), names * k, np.tile(pose, (k, 1)),
            np.tile(vel, (k, 1)))
