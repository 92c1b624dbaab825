"""Reference-pose generation on the device: PathDiscretizer::getNextNPoses for B robots in one launch.

Mirrors include/nmpc_nav_control/PathDiscretizer.h:12-51 (constructor arguments, getNextNPoses) on top of
``nmpc_path_discretize`` (include/nmpc_amd/nmpc_path.h). The march itself runs only in the HIP kernel
(csrc/path_discretizer.hip); this module builds and packs path segments and owns the device buffers.
``nearest`` / ``PathMinDist`` are the step before it, each robot's nearest path point (``nmpc_path_nearest``,
csrc/path_nearest.hip), by this project's own search rule: the reference's lives in the same un-vendored library.

Path segments restate the part of parametric_trajectories_common::TPath that PathDiscretizer uses (the
library is not vendored by the reference): cubic polynomials x(u), y(u), theta_h(u) on u in [0, 1] plus a
signed speed. ``PathSegment.line / bezier / arc`` build the usual shapes.
"""
import ctypes
import math

import numpy as np
import torch

from ._lib import PathQueueStruct, check, lib
from .controller import Pose

SEG_DOUBLES = 16  # sizeof(nmpc_path_segment) / sizeof(double)


class PathSegment:
    """One parametric segment: GetX/GetY/GetThetaHolomonic are cubics in u (ascending coefficients),
    GetVelocity() = v (negative: the robot drives the segment backwards)."""

    def __init__(self, x, y, th=(0.0, 0.0, 0.0, 0.0), v=0.0):
        self.x = np.asarray(x, np.float64).reshape(4)
        self.y = np.asarray(y, np.float64).reshape(4)
        self.th = np.asarray(th, np.float64).reshape(4)
        self.v = float(v)

    def GetVelocity(self):
        return self.v

    def pack(self):
        rec = np.zeros(SEG_DOUBLES)
        rec[0:4], rec[4:8], rec[8:12], rec[12] = self.x, self.y, self.th, self.v
        return rec

    @staticmethod
    def _heading(th0, th1, default):
        th0 = default if th0 is None else th0
        th1 = th0 if th1 is None else th1
        return (th0, th1 - th0, 0.0, 0.0)  # linear holonomic heading

    @classmethod
    def line(cls, p0, p1, v, th0=None, th1=None):
        (x0, y0), (x1, y1) = p0, p1
        d = math.atan2(y1 - y0, x1 - x0)
        return cls((x0, x1 - x0, 0, 0), (y0, y1 - y0, 0, 0), cls._heading(th0, th1, d), v)

    @classmethod
    def bezier(cls, p0, p1, p2, p3, v, th0=None, th1=None):
        """Cubic Bezier with control points p0..p3 in power form."""
        P = np.asarray([p0, p1, p2, p3], np.float64)
        c = np.stack([P[0], 3 * (P[1] - P[0]), 3 * (P[2] - 2 * P[1] + P[0]), P[3] - 3 * P[2] + 3 * P[1] - P[0]])
        d = math.atan2(*(P[1] - P[0])[::-1]) if np.any(P[1] != P[0]) else 0.0
        return cls(c[:, 0], c[:, 1], cls._heading(th0, th1, d), v)

    @classmethod
    def arc(cls, cx, cy, r, a0, a1, v, th0=None, th1=None):
        """Circular arc (centre, radius, polar angles a0 -> a1, |a1 - a0| <= pi/2) as its standard cubic
        Bezier approximation (radial error < 3e-4 r for a quarter circle)."""
        k = 4.0 / 3.0 * math.tan((a1 - a0) / 4.0)
        p0 = (cx + r * math.cos(a0), cy + r * math.sin(a0))
        p3 = (cx + r * math.cos(a1), cy + r * math.sin(a1))
        p1 = (p0[0] - k * r * math.sin(a0), p0[1] + k * r * math.cos(a0))
        p2 = (p3[0] + k * r * math.sin(a1), p3[1] - k * r * math.cos(a1))
        return cls.bezier(p0, p1, p2, p3, v, th0, th1)


def pack_paths(path_lists, max_segs=None):
    """[B][S][16] float64 segment records and int32 [B] counts of B path lists (S = longest list)."""
    S = max(max(len(p) for p in path_lists), 1) if max_segs is None else int(max_segs)
    segs = np.zeros((len(path_lists), S, SEG_DOUBLES))
    nseg = np.zeros(len(path_lists), np.int32)
    for i, pl in enumerate(path_lists):
        if not 1 <= len(pl) <= S:
            raise ValueError(f"path {i}: {len(pl)} segments (1..{S} allowed)")
        for j, s in enumerate(pl):
            segs[i, j] = s.pack()
        nseg[i] = len(pl)
    return segs, nseg


class PathQueue:
    """The path sets of B robots on the device, for BatchSolver.node_tick_queue (nmpc_path_queue): segs float64
    [B][S][16] every robot's whole part list, npart int32 [B], and the window the tick keeps over it, head / tail
    int32 [B] (active parts [head, tail), queued parts [tail, npart)) with path_u float64 [B], the progress relative
    to part head. frames / lengths: also own frame int32 [B][S] (frame ids as numbers; a part joins the window only
    behind a part of the same frame) and length float64 [B][S] (GetPathLength(); without it every part counts
    part_length, the node's SetPathLength(1000)). remains float64 [B]: patch_remains of the robots in FOLLOW_PATH."""

    def __init__(self, B, S, device="cuda", frames=False, lengths=False, remains=True, part_length=None,
                 max_active_len=None):
        self.B, self.S = int(B), int(S)
        if self.S < 1:
            raise ValueError("S must be >= 1")
        self.device = torch.device(device)
        z = lambda *shape, dt: torch.zeros(*shape, dtype=dt, device=self.device)  # noqa: E731
        self.segs = z(self.B, self.S, SEG_DOUBLES, dt=torch.float64)
        self.npart, self.head, self.tail = (z(self.B, dt=torch.int32) for _ in range(3))
        self.path_u = z(self.B, dt=torch.float64)
        self.frame = z(self.B, self.S, dt=torch.int32) if frames else None
        self.length = z(self.B, self.S, dt=torch.float64) if lengths else None
        self.remains = torch.full((self.B,), math.nan, dtype=torch.float64, device=self.device) if remains else None
        d = PathQueueStruct()
        check(lib().nmpc_path_queue_default(ctypes.byref(d)), "nmpc_path_queue_default")
        self.part_length = d.part_length if part_length is None else float(part_length)
        self.max_active_len = d.max_active_len if max_active_len is None else float(max_active_len)

    def set_path_set(self, i, parts, frames=None, lengths=None):
        """Give robot i a new path set: parts is a list of PathSegment or an array [n][16] of segment records
        (1 <= n <= S), frames / lengths its per-part frame ids and lengths (required when the queue owns those
        arrays). Zeroes the robot's window and progress; the caller sets mode[i] = NODE_FOLLOW_PATH and
        reset[i] = 1, as the node's path callbacks do."""
        recs = np.stack([p.pack() if isinstance(p, PathSegment) else np.asarray(p, np.float64) for p in parts]) \
            if len(parts) else np.zeros((0, SEG_DOUBLES))
        n = len(recs)
        if n > self.S or recs.shape[1:] != (SEG_DOUBLES,):
            raise ValueError(f"robot {i}: {n} parts of shape {recs.shape[1:]} ({self.S} records of 16 doubles allowed)")
        for name, own, given, dt in (("frames", self.frame, frames, np.int32), ("lengths", self.length, lengths,
                                                                              np.float64)):
            if (own is None) != (given is None):
                raise ValueError(f"robot {i}: {name} must be given exactly when the queue owns them")
            if own is not None:
                a = np.asarray(given, dt)
                if a.shape != (n,):
                    raise ValueError(f"robot {i}: {name} must have one entry per part")
                own[i, :n] = torch.from_numpy(a).to(self.device)
        self.segs[i] = 0.0
        if n:
            self.segs[i, :n] = torch.from_numpy(recs).to(self.device)
        self.npart[i] = n
        self.head[i] = 0
        self.tail[i] = 0
        self.path_u[i] = 0.0

    def struct(self):
        """the nmpc_path_queue of this queue's tensors"""
        p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        return PathQueueStruct(npart=p(self.npart), head=p(self.head), tail=p(self.tail), frame=p(self.frame),
                               length=p(self.length), part_length=self.part_length,
                               max_active_len=self.max_active_len, remains=p(self.remains))


def _dev_ptr(t, dtype):
    if t is None:
        return None
    if not t.is_cuda or not t.is_contiguous() or t.dtype != dtype:
        raise ValueError(f"expected a contiguous {dtype} device tensor")
    return ctypes.c_void_p(t.data_ptr())


def discretize(segs, nseg, nearest_u, sample_period, num_poses, is_holonomic=False, traj=None, traj64=None,
               stream=None):
    """nmpc_path_discretize on device tensors: segs float64 [B][S][16], nseg int32 [B], nearest_u float64 [B].
    Writes traj float32 [num_poses][3][B] (allocated if None; the traj input of BatchSolver.run) and, if
    given, traj64 float64 [num_poses][3][B]. Returns traj."""
    B, S = int(segs.shape[0]), int(segs.shape[1])
    if segs.dim() != 3 or segs.shape[2] != SEG_DOUBLES:
        raise ValueError("segs must be [B][S][16]")
    if nseg.shape != (B,) or nearest_u.shape != (B,):
        raise ValueError("nseg and nearest_u must be [B]")
    if traj is None:
        traj = torch.empty((num_poses, 3, B), dtype=torch.float32, device=segs.device)
    for t in (traj, traj64):
        if t is not None and tuple(t.shape) != (num_poses, 3, B):
            raise ValueError("traj / traj64 must be [num_poses][3][B]")
    s = stream if stream is not None else torch.cuda.current_stream(segs.device)
    check(lib().nmpc_path_discretize(B, _dev_ptr(segs, torch.float64), S, _dev_ptr(nseg, torch.int32),
                                     _dev_ptr(nearest_u, torch.float64), float(sample_period), int(num_poses),
                                     1 if is_holonomic else 0, _dev_ptr(traj, torch.float32),
                                     _dev_ptr(traj64, torch.float64), ctypes.c_void_p(s.cuda_stream)),
          "nmpc_path_discretize")
    return traj


def nearest(segs, nseg, pose, u_range=None, holonomic_heading=False, near=None, err=None, stream=None):
    """nmpc_path_nearest on device tensors: segs float64 [B][S][16], nseg int32 [B], pose float32 [3][B],
    u_range float64 [2][B] {lo, hi} or None (the whole path; a NaN bound leaves its side open). Writes, if given,
    near float64 [4][B] {x, y, theta, theta_holonomic} and err float64 [2][B] {pos_error_to_path,
    ori_error_to_path}. Returns nearest_u float64 [B]. The search rule is this project's own (nmpc_path.h)."""
    B, S = int(segs.shape[0]), int(segs.shape[1])
    if segs.dim() != 3 or segs.shape[2] != SEG_DOUBLES:
        raise ValueError("segs must be [B][S][16]")
    if nseg.shape != (B,) or tuple(pose.shape) != (3, B):
        raise ValueError("nseg must be [B] and pose [3][B]")
    for t, rows, name in ((u_range, 2, "u_range"), (near, 4, "near"), (err, 2, "err")):
        if t is not None and tuple(t.shape) != (rows, B):
            raise ValueError(f"{name} must be [{rows}][B]")
    nearest_u = torch.empty(B, dtype=torch.float64, device=segs.device)
    s = stream if stream is not None else torch.cuda.current_stream(segs.device)
    check(lib().nmpc_path_nearest(B, _dev_ptr(segs, torch.float64), S, _dev_ptr(nseg, torch.int32),
                                  _dev_ptr(pose, torch.float32), _dev_ptr(u_range, torch.float64),
                                  1 if holonomic_heading else 0, _dev_ptr(nearest_u, torch.float64),
                                  _dev_ptr(near, torch.float64), _dev_ptr(err, torch.float64),
                                  ctypes.c_void_p(s.cuda_stream)), "nmpc_path_nearest")
    return nearest_u


class PathMinDist:
    """One-robot mirror of the call NMPCNavControlROS.cpp:599-601 makes, TPathProcessMinDist::GetMinDist, on the
    device search (nmpc_path_nearest). The reference's constructor arguments (10, 0.01) belong to the un-vendored
    library's own search and are accepted and ignored: the search rule is this project's."""

    def __init__(self, num_iterations=10, tolerance=0.01, device="cuda"):
        self.device = torch.device(device)

    def GetMinDist(self, path_list, x, y, theta):
        """(u, x, y, theta, theta_holonomic) of the path point nearest to the robot at (x, y)."""
        segs, nseg = pack_paths([list(path_list)])
        dev = self.device
        near = torch.empty((4, 1), dtype=torch.float64, device=dev)
        pose = torch.tensor([[x], [y], [theta]], dtype=torch.float32, device=dev)
        u = nearest(torch.from_numpy(segs).to(dev), torch.from_numpy(nseg).to(dev), pose, near=near)
        n = near.cpu().numpy()[:, 0]
        return float(u.cpu()[0]), float(n[0]), float(n[1]), float(n[2]), float(n[3])


class PathDiscretizer:
    """PathDiscretizer(sample_period, num_poses, is_holonomic) (PathDiscretizer.cpp:5-12). getNextNPoses runs
    one robot on the device; discretize_batch runs many."""

    def __init__(self, sample_period, num_poses, is_holonomic=False, device="cuda"):
        self.sample_period = float(sample_period)
        self.num_poses = int(num_poses)
        self.is_holonomic = bool(is_holonomic)
        self.device = torch.device(device)

    def discretize_batch(self, path_lists, nearest_u):
        """[B][num_poses][3] float64 poses of B robots (path lists of PathSegment, nearest path parameters)."""
        segs, nseg = pack_paths(path_lists)
        dev = self.device
        t64 = torch.empty((self.num_poses, 3, len(path_lists)), dtype=torch.float64, device=dev)
        discretize(torch.from_numpy(segs).to(dev), torch.from_numpy(nseg).to(dev),
                   torch.as_tensor(np.asarray(nearest_u, np.float64)).to(dev), self.sample_period, self.num_poses,
                   self.is_holonomic, traj64=t64)
        return t64.permute(2, 0, 1).cpu().numpy()

    def getNextNPoses(self, path_list, nearest_sample_u, next_poses=None):
        """Appends num_poses poses to next_poses (a list; created if None) and returns it (PathDiscretizer.cpp:14)."""
        out = self.discretize_batch([list(path_list)], [nearest_sample_u])[0]
        next_poses = [] if next_poses is None else next_poses
        next_poses.extend(Pose(float(p[0]), float(p[1]), float(p[2])) for p in out)
        return next_poses
