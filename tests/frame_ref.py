"""numpy model of the frame table's writers (csrc/robot_tables.hip: k_frame_set, k_frame_map), in the operation order
include/nmpc_amd/nmpc_batch.h gives, so that the device's results can be compared bit for bit.

The table is origin [2][cap] float64 (None while it is off); the resident iterate xbar is [(N+1)*nx][cap] float32, of
which the writers touch rows k*nx (x) and k*nx + 1 (y) of the masked robots and nothing else.
"""
import numpy as np


class Frames:
    """The frame table of a handle of capacity `cap`, and its iterate xbar ([(N+1)*nx][cap] float32, moved in place)."""

    def __init__(self, cap, N, nx, xbar):
        self.cap, self.N, self.nx = cap, N, nx
        self.origin = None  # off
        self.xbar = xbar
        assert xbar.dtype == np.float32 and xbar.shape == ((N + 1) * nx, cap)

    def _ready(self):
        if self.origin is None:
            self.origin = np.zeros((2, self.cap))  # the first writer's fill

    def _move(self, go, new):
        """the robots `go` (bool [B]) take the origins new [2][B]; every stage's x and y row becomes
        (float)((double)x + (o_old - o_new))"""
        B = len(go)
        idx = np.flatnonzero(go)
        for c in range(2):
            d = self.origin[c, idx] - new[c, idx]
            rows = np.arange(self.N + 1) * self.nx + c
            self.xbar[np.ix_(rows, idx)] = (self.xbar[np.ix_(rows, idx)].astype(np.float64) + d[None, :]).astype(
                np.float32)
            self.origin[c, idx] = new[c, idx]
        assert B <= self.cap

    def set(self, origin, mask=None):
        """nmpc_batch_set_robot_frame: origin [2][B] float64, mask [B] or None"""
        origin = np.asarray(origin, np.float64)
        B = origin.shape[1]
        self._ready()
        go = np.ones(B, bool) if mask is None else np.asarray(mask) != 0
        self._move(go, origin)

    def recentre(self, pose_map, radius, mask=None):
        """nmpc_batch_recentre: pose_map [2 or 3][B] float64; returns moved [B] uint8"""
        pose_map = np.asarray(pose_map, np.float64)
        B = pose_map.shape[1]
        self._ready()
        x, y = pose_map[0], pose_map[1]
        go = np.ones(B, bool) if mask is None else np.asarray(mask) != 0
        with np.errstate(invalid="ignore"):
            far = (np.abs(x - self.origin[0, :B]) > radius) | (np.abs(y - self.origin[1, :B]) > radius)
        go = go & far & np.isfinite(x) & np.isfinite(y)
        self._move(go, np.stack([np.rint(x), np.rint(y)]))
        return go.astype(np.uint8)

    def clear(self):
        """nmpc_batch_clear_robot_frame: the writer with origin 0 for the whole capacity, then off"""
        if self.origin is not None:
            self._move(np.ones(self.cap, bool), np.zeros((2, self.cap)))
            self.origin = None

    def _o(self, B, c):
        o = np.zeros((c, B))
        if self.origin is not None:
            o[:2] = self.origin[:, :B]
        return o

    def to_frame(self, values):
        """nmpc_batch_to_frame: values [n][c][B] float64 -> float32, components 0 and 1 (float)(v - origin)"""
        values = np.asarray(values, np.float64)
        n, c, B = values.shape
        out = values.copy()
        out[:, :2] = values[:, :2] - self._o(B, c)[None, :2]
        return out.astype(np.float32)

    def from_frame(self, values):
        """nmpc_batch_from_frame: values [n][c][B] float32 -> float64, components 0 and 1 (double)v + origin"""
        assert np.asarray(values).dtype == np.float32
        out = np.asarray(values).astype(np.float64)
        n, c, B = out.shape
        out[:, :2] = out[:, :2] + self._o(B, c)[None, :2]
        return out
