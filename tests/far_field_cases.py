"""Fleets and edge-case tables far from the map origin, for tests/test_far_field_cases.py (CPU: the shift is a valid
instrument) and tests/test_gpu_far_field.py (every kernel form against the fp64 oracle at distance). Pure numpy.

The solve kernels carry x and y as absolute fp32 values from the input to the stored iterate, and every other fleet
of the suite sits within two metres of (0, 0). OFFSETS moves a fleet to where a warehouse robot is in the map frame;
x and y lie in different binades on purpose. A shifted value is built in fp64 (the fp32 input widened, plus the
offset) and rounded to fp32 once: the device gets the fp32 value, the oracle the same value widened. Only positions
move: headings, velocities, curvatures, lengths and the carried refs are translation-invariant.

The tolerance rule (DESIGN.md "Coordinate range"): the error's only legitimate source at distance is ulp(D), linear in
D = max(|x|, |y|) of the offset. Up to the supported radius R the project's tolerances hold unchanged; beyond it they
grow by D / R. R is measured (test_gpu_far_field.py's docstring has the table): the largest swept D at which the worst
|u0| and |cmd| error over all models and forms is at most half of 1e-3.
"""
import copy

import numpy as np

from run_edge_cases import f32

OFFSETS = [(0.0, 0.0), (64.0, -32.0), (512.0, -256.0), (4096.0, 2048.0)]
R = 64.0  # supported radius in metres


def distance(off):
    return float(np.abs(np.asarray(off, np.float64)).max())


def tol_scale(off):
    """the factor on TOL_U / TOL_X / TOL_UTRAJ at this offset: 1 up to R, D / R beyond"""
    return max(1.0, distance(off) / R)


def off_id(off):
    return f"{off[0]:g}_{off[1]:g}"


def shift_fleet(fl, off):
    """A scenario.make_fleet dict moved by off: [2], or [B][2] for one offset per robot. Pose x and y and path x0 and
    y0 move (a goal robot keeps its goal in those rows); every array keeps make_fleet's dtype and layout, so the moved
    values are fp32."""
    off = np.asarray(off, np.float64)
    out = {k: np.array(v, copy=True) for k, v in fl.items()}
    d = off[:, None] if off.ndim == 1 else off.T  # [2][1] or [2][B]
    for k in ("pose", "path"):
        out[k][:2] = (fl[k][:2].astype(np.float64) + d).astype(np.float32)
    return out


def shift_cases(cs, off):
    """A run_edge_cases.cases() table moved by off: poses, every trajectory row and the garbage rows, so garbage stays
    50 m from the shifted lines. Values are fp32-valued float64, as the table's."""
    off = np.asarray(off, np.float64)
    out = []
    for c in cs:
        c = copy.copy(c)
        c.ticks = [dict(tk) for tk in c.ticks]
        for tk in c.ticks:
            pose, traj = tk["pose"].copy(), tk["traj"].copy()
            pose[:2] = f32(pose[:2] + off)
            traj[:, :2] = f32(traj[:, :2] + off)
            tk["pose"], tk["traj"] = pose, traj
        out.append(c)
    return out
