"""numpy restatement of the separation guard (nmpc_sep_guard, nmpc_batch_stage_limits_from_tracks_ex,
nmpc_batch_sep_hold; csrc/separation.hip), in the operation order of include/nmpc_amd/nmpc_batch.h "The separation
guard", on top of tests/separation_ref.py: the pairs and what counts are that file's, brute force over all pairs; this
one restates qy and qa, the standing / direction selection and the hold. Every fp32 value is a numpy float32 and every
operation one rounding, so the device's vlim, gap, gap_all and held are compared bit for bit."""
import numpy as np

from tests import separation_ref as sp
from tests import speed_map_ref as sr

F32 = np.float32
GOTO_POSE, FOLLOW_PATH = sp.GOTO_POSE, sp.FOLLOW_PATH
EV_HELD = 9
GUARD = dict(stop_gap=0.45, release_gap=0.55, hold_stages=4, hold=1)
INT_MAX, INT_MIN = np.iinfo(np.int32).max, np.iinfo(np.int32).min


def _flags(B, a):
    return np.zeros(B, bool) if a is None else np.asarray(a)[:B].astype(bool)


def positions(xbar, nx, N, B, pose=None, reset=None, held=None):
    """(pos, h) [N+1][2][B] fp32: a robot that stands (reset or held) has its pose at every stage; h_k is the iterate's
    direction of travel, 0 for a reset robot only"""
    stand = _flags(B, reset) | _flags(B, held)
    pos = sr.stage_positions(xbar, nx, N, B, pose, stand if stand.any() else None)
    return pos, sp.headings(sr.stage_positions(xbar, nx, N, B), reset)


def export(xy, first, xbar, nx, N, B, origin=None, pose=None, reset=None, mode=None, held=None):
    """separation_ref.export in which a held robot is a standing obstacle at its pose, like a reset one"""
    sp.export(xy, first, xbar, nx, N, B, origin, pose, reset=_flags(B, reset) | _flags(B, held), mode=mode)


def minima(pos, h, xy, own_first=-1, origin=None, range=3.0, ahead_only=1, priority=None, own_priority=None):
    """(qy, qa) [N+1][B] fp32: the minimum q over the counting pairs whose track has priority[j] >= own_i, and over
    every counting pair (+inf: none). priority int [M] or None (qy == qa), own_priority int [B] or None
    (priority[own_first + i])"""
    q, counts = sp.pairs(pos, h, xy, own_first, origin, range, ahead_only)
    inf = F32(np.inf)
    qa = np.where(counts, q, inf).min(axis=2, initial=inf).astype(F32)
    if priority is None:
        return qa.copy(), qa
    B = q.shape[1]
    pr = np.asarray(priority, np.int64)
    own = pr[own_first + np.arange(B)] if own_priority is None else np.asarray(own_priority, np.int64)[:B]
    yields = pr[None, None, :] >= own[None, :, None]
    qy = np.where(counts & yields, q, inf).min(axis=2, initial=inf).astype(F32)
    return qy, qa


def limits(xbar, nx, N, B, xy, cap, a, dt, carried, nv, pose=None, reset=None, held=None, m=None, origin=None,
           own_first=-1, clearance=0.6, gain=1.0, range=3.0, ahead_only=1, slope=0.8, v_floor=0.05, priority=None,
           own_priority=None):
    """(lim, gap, gap_all) [N+1][B] fp32 of the guarded writer. xbar [(N+1)*nx][>= B] fp32, pose [3][B] fp32; the map
    is looked up at the positions the unguarded writer uses (the pose for a reset robot only)"""
    pos, h = positions(xbar, nx, N, B, pose, reset, held)
    qy, qa = minima(pos, h, xy, own_first, origin, range, ahead_only, priority, own_priority)
    gap, gap_all = np.sqrt(qy).astype(F32), np.sqrt(qa).astype(F32)
    with np.errstate(invalid="ignore"):
        s = F32(gain) * (gap - F32(clearance))
    assert s.dtype == F32
    fresh = _flags(B, reset)
    pos_map = sr.stage_positions(xbar, nx, N, B, pose, fresh if fresh.any() else None)
    lim = sr.limits(sp._Capped(m, np.fmax(F32(v_floor), s)), pos_map, cap, a, dt, carried, nv, origin, slope=slope,
                    v_floor=v_floor)
    return lim, gap, gap_all


def hold(gap_all, held, reset=None, mode=None, stop_gap=0.45, release_gap=0.55, hold_stages=4, hold=1):
    """held' [B] uint8 from gap_all [N+1][B] fp32: m = min over the stages 0..min(hold_stages, N) (a NaN never counts,
    +inf when nothing counts); held' = reset ? 0 : (held ? m < release_gap : m < stop_gap); 0 for a robot whose mode
    (when given) is neither GOTO_POSE nor FOLLOW_PATH, and for everyone with hold == 0"""
    g = np.asarray(gap_all, F32)
    S, B = g.shape
    last = min(int(hold_stages), S - 1)
    m = np.fmin.reduce(np.vstack([np.full((1, B), np.inf, F32), g[:last + 1]]), axis=0)
    was = _flags(B, held)
    now = np.where(was, m < F32(release_gap), m < F32(stop_gap)) & ~_flags(B, reset)
    if mode is not None:
        now &= np.isin(np.asarray(mode)[:B], (GOTO_POSE, FOLLOW_PATH))
    if not hold:
        now[:] = False
    return now.astype(np.uint8)
