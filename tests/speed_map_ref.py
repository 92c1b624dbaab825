"""numpy restatement of the speed map's rule (nmpc_batch_stage_limits_from_map, csrc/speed_map.hip), in the operation
order of include/nmpc_amd/nmpc_batch.h "Speed zones": every fp32 value is a numpy float32 and every operation one
rounding, so the device's vlim is compared bit for bit."""
import numpy as np

F32 = np.float32


class Map:
    """nmpc_speed_map on the host: vmax [h][w] float32 (row cy, column cx)"""

    def __init__(self, x0, y0, res, vmax, outside=np.inf):
        self.x0, self.y0, self.res = float(x0), float(y0), float(res)
        self.vmax = np.ascontiguousarray(vmax, F32)
        self.h, self.w = self.vmax.shape
        self.outside = F32(outside)

    def cell(self, X, Y):
        """m: the cell's limit at the fp64 map positions X, Y (any shape); outside off the grid and where not finite"""
        with np.errstate(invalid="ignore"):
            fx, fy = np.floor((X - self.x0) / self.res), np.floor((Y - self.y0) / self.res)
            inside = (fx >= 0) & (fx < self.w) & (fy >= 0) & (fy < self.h)
        cx, cy = np.where(inside, fx, 0).astype(np.int64), np.where(inside, fy, 0).astype(np.int64)
        return np.where(inside, self.vmax[cy, cx], self.outside).astype(F32)


def stage_positions(xbar, nx, N, B, pose=None, reset=None):
    """the fp32 stage positions [N+1][2][B]: rows k*nx, k*nx+1 of xbar ([(N+1)*nx][>= B]); pose[0..1] at every stage of
    a robot with reset != 0"""
    xb = np.asarray(xbar, F32)[:, :B].reshape(N + 1, nx, B)
    pos = xb[:, :2].copy()
    if reset is not None:
        r = np.asarray(reset).astype(bool)
        pos[:, :, r] = np.asarray(pose, F32)[None, :2][:, :, r]
    return pos


def limits(m, pos, cap, a, dt, carried, nv, origin=None, slope=0.8, v_floor=0.05):
    """lim [N+1][B] float32. pos [N+1][2][B] fp32 stage positions, cap and a [B] (or scalars) fp32, carried [nbx][B]
    fp32 of which the first nv rows are speed reference states, origin [2][B] fp64 or None."""
    pos = np.asarray(pos, F32)
    S, _, B = pos.shape
    cap, a = np.broadcast_to(np.asarray(cap, F32), (B,)), np.broadcast_to(np.asarray(a, F32), (B,))
    g = (F32(slope) * a) * F32(dt)
    assert g.dtype == F32
    c = np.zeros(B, F32)
    for j in range(nv):
        c = np.fmax(c, np.abs(np.asarray(carried, F32)[j, :B]))
    X, Y = pos[:, 0].astype(np.float64), pos[:, 1].astype(np.float64)
    if origin is not None:
        X, Y = X + np.asarray(origin, np.float64)[0, :B], Y + np.asarray(origin, np.float64)[1, :B]
    z = np.fmin(cap[None, :], np.fmax(F32(v_floor), m.cell(X, Y)))
    assert z.dtype == F32
    lim = np.empty((S, B), F32)
    with np.errstate(invalid="ignore"):
        for k in range(S):
            # the candidates j = k..N, each one multiply and one add (j = k: z_k + 0 g = z_k); min is exact
            cand = z[k:] + np.arange(S - k, dtype=F32)[:, None] * g[None, :]
            assert cand.dtype == F32
            lim[k] = np.fmax(np.fmin.reduce(cand, axis=0), c - F32(k) * g)
    return lim
