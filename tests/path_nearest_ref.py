"""fp64 numpy oracle of the nearest-point search (nmpc_path_nearest), independent of the kernel's method.

Per segment the stationary points of |P(u) - r|^2 are the real roots of the quintic g(u) = (P - r) . P' (numpy's
companion-matrix polyroots on the trimmed coefficients, each polished by two Newton steps); the candidates are those
roots inside the clipped search range plus the range ends, the answer is the candidate of least distance over all
segments, the smallest U on ties. The definitions (U, segment index, search range, near pose, errors) are those of
include/nmpc_amd/nmpc_path.h.
"""
import math

import numpy as np
from numpy.polynomial import polynomial as npoly

U_SEP = 1e-6  # candidates further than this from the answer (in U) count for the distance gap


def seg_xy(seg, u):
    return npoly.polyval(u, seg[0:4]), npoly.polyval(u, seg[4:8])


def seg_dxy(seg, u):
    return npoly.polyval(u, npoly.polyder(seg[0:4])), npoly.polyval(u, npoly.polyder(seg[4:8]))


def split_u(U, n):
    """segment index and local parameter of the path parameter U (k = min(floor(U), n - 1), u = U - k)"""
    k = min(int(math.floor(U)), n - 1) if U >= 0 else 0
    return k, U - k


def path_point(segs, n, U):
    k, u = split_u(U, n)
    return seg_xy(segs[k], u)


def norm_ang(a):
    """normAngRad, the fmod form"""
    a = math.fmod(a + math.pi, 2 * math.pi)
    if a < 0:
        a += 2 * math.pi
    return a - math.pi


def near_err(segs, n, U, pose, holonomic_heading=False):
    """near {x, y, theta, theta_holonomic} and err {pos, ori} at the path parameter U"""
    k, u = split_u(U, n)
    x, y = seg_xy(segs[k], u)
    dx, dy = seg_dxy(segs[k], u)
    th = math.atan2(dy, dx)
    thh = float(npoly.polyval(u, segs[k][8:12]))
    head = thh if holonomic_heading else (th + math.pi if segs[k][12] < 0.0 else th)
    pos = math.sqrt((x - pose[0]) ** 2 + (y - pose[1]) ** 2)
    ori = abs(norm_ang(head - pose[2]))
    return np.array([x, y, th, thh]), np.array([pos, ori])


def clip_range(n, u_range=None):
    lo, hi = 0.0, float(n)
    if u_range is not None:
        if not math.isnan(u_range[0]):
            lo = min(max(float(u_range[0]), 0.0), float(n))
        if not math.isnan(u_range[1]):
            hi = min(max(float(u_range[1]), 0.0), float(n))
    return lo, max(hi, lo)


def _candidates(seg, r, a, b):
    """local parameters in [a, b] where |P - r| may be least on one segment: the ends and the real roots of g"""
    cx, cy = seg[0:4].copy(), seg[4:8].copy()
    cx[0] -= r[0]
    cy[0] -= r[1]
    g = npoly.polyadd(npoly.polymul(cx, npoly.polyder(cx)), npoly.polymul(cy, npoly.polyder(cy)))
    g = np.trim_zeros(np.atleast_1d(g), "b")
    out = [a, b]
    if len(g) >= 2:
        dg = npoly.polyder(g)
        for z in npoly.polyroots(g):
            if abs(z.imag) > 1e-6:
                continue
            u = float(z.real)
            out.append(min(max(u, a), b))
            for _ in range(2):  # polish
                d = npoly.polyval(u, dg)
                if d == 0.0:
                    break
                u = u - npoly.polyval(u, g) / d
            if math.isfinite(u):
                out.append(min(max(u, a), b))
    return out


def nearest_one(segs, n, r, u_range=None):
    """(U, d, gap, cond) of one robot: the answer, its distance, the distance gap to the best candidate more than
    U_SEP away in U (inf if none) and the conditioning g'(u*) / |P'|^2 of the answer (inf at a range end whose
    derivative is not zero; 0 on a degenerate segment)."""
    lo, hi = clip_range(n, u_range)
    cand = []
    for k in range(n):
        if lo > k + 1 or hi < k:
            continue
        a, b = min(max(lo - k, 0.0), 1.0), min(max(hi - k, 0.0), 1.0)
        for u in _candidates(segs[k], r, a, b):
            x, y = seg_xy(segs[k], u)
            cand.append((math.hypot(x - r[0], y - r[1]), k + u, k, u))
    cand.sort(key=lambda c: (c[0], c[1]))
    d, U, k, u = cand[0]
    far = [c[0] - d for c in cand if abs(c[1] - U) > U_SEP]
    gap = min(far) if far else math.inf
    dx, dy = seg_dxy(segs[k], u)
    s2 = dx * dx + dy * dy
    if s2 == 0.0:
        cond = 0.0
    else:
        x, y = seg_xy(segs[k], u)
        ddx = npoly.polyval(u, npoly.polyder(segs[k][0:4], 2))
        ddy = npoly.polyval(u, npoly.polyder(segs[k][4:8], 2))
        g = (x - r[0]) * dx + (y - r[1]) * dy
        at_end = (U == lo and g > 0.0) or (U == hi and g < 0.0)
        cond = math.inf if at_end and abs(g) > 1e-6 * s2 else (s2 + (x - r[0]) * ddx + (y - r[1]) * ddy) / s2
    return U, d, gap, cond


def nearest_ref(segs, nseg, pos, u_range=None):
    """nearest_one for B robots: segs [B][S][16], nseg [B], pos [B][2], u_range [2][B] or None.
    Returns U, d, gap, cond, each [B]."""
    B = len(nseg)
    out = np.zeros((4, B))
    for i in range(B):
        ur = None if u_range is None else (u_range[0][i], u_range[1][i])
        out[:, i] = nearest_one(segs[i], int(nseg[i]), pos[i], ur)
    return out[0], out[1], out[2], out[3]


def dist_at(segs, nseg, U, pos):
    """|P(U_i) - r_i| for every robot"""
    d = np.zeros(len(nseg))
    for i in range(len(nseg)):
        x, y = path_point(segs[i], int(nseg[i]), U[i])
        d[i] = math.hypot(x - pos[i][0], y - pos[i][1])
    return d
