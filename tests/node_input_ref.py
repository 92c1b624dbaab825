"""numpy restatement of the node's input stage (include/nmpc_amd/nmpc_batch.h: nmpc_batch_push_samples,
nmpc_batch_node_input and the status rule of nmpc_batch_node_cycle; csrc/node_input.hip), in fp64 with int64 stamps and
the operation order the header gives, one robot at a time in plain scalar code. No product-sum is fused here, as none
is on the device, so the ring, held x, y and theta, valid, dropped and moved compare bit for bit; v, vn and w go through
cos and sin and compare to 1e-12. Host side only.

The state is the device's: stamp [depth][cap] int64, sample [depth][3][cap], count / newest [cap] int32, held [7][cap]
(x, y, theta, v, vn, w, steer), all 0 at the start. The frame table and the resident iterate are tests/frame_ref.py's
Frames, whose recentre the stage calls (one statement of that rule on the host, as on the device).
"""
import math

import numpy as np

IDLE, GOTO_POSE, FOLLOW_PATH, BREAK, ERROR = range(5)
EV_INPUT_INVALID = 8
NS = 1000000000
TWO_PI = 2.0 * math.pi
HX, HY, HTH, HV, HVN, HW, HSTEER = range(7)

DEFAULTS = dict(period_ns=25000000, transform_timeout=0.1, pose_valid_overwritten=1, strict=0,
                recentre_radius=math.inf)


def sec(d):
    """ros::Duration::toSec of d nanoseconds"""
    q = int(d) // NS  # floor
    r = int(d) - q * NS
    return float(q) + 1e-9 * float(r)


def norm_ang(a):
    """normAngRad (utils.h:41-47, the fmod form)"""
    a = math.fmod(a + math.pi, TWO_PI)
    if a < 0.0:
        a += TWO_PI
    return a - math.pi


def unwrap_hack(last_theta, curr_theta, why=None):
    """NMPCNavControlROS.cpp:414-423 on (robot_pose_.theta, the new yaw); each loop coded for two trips. why: a set that
    receives which branches fired"""
    why = set() if why is None else why
    delta = curr_theta - last_theta
    if delta > math.pi:
        curr_theta -= TWO_PI
        why.add("unwrap_down")
    elif delta < -math.pi:
        curr_theta += TWO_PI
        why.add("unwrap_up")
    for _ in range(2):
        if curr_theta >= TWO_PI:
            curr_theta -= TWO_PI
            why.add("clamp_pos")
    for _ in range(2):
        if curr_theta <= -TWO_PI:
            curr_theta += TWO_PI
            why.add("clamp_neg")
    return curr_theta


def body_velocity(p1, p2, dt):
    """NMPCNavControlROS.cpp:456-476: (v, vn, w) from two samples (x, y, yaw) dt seconds apart"""
    dx = p2[0] - p1[0]
    dy = p2[1] - p1[1]
    dyaw = norm_ang(p2[2] - p1[2])
    mid_yaw = p1[2] + dyaw / 2.0
    vx_global = dx / dt
    vy_global = dy / dt
    cos_yaw = math.cos(-mid_yaw)
    sin_yaw = math.sin(-mid_yaw)
    return (vx_global * cos_yaw - vy_global * sin_yaw, vx_global * sin_yaw + vy_global * cos_yaw, dyaw / dt)


class InputRef:
    """The input state of a handle of capacity cap. frames: a tests/frame_ref.py Frames (the handle's frame table and
    iterate) or None (a stage with a finite recentre_radius needs one)."""

    def __init__(self, cap, depth, tric=False, frames=None):
        assert 2 <= depth <= 64
        self.cap, self.depth, self.tric, self.frames = cap, depth, tric, frames
        self.stamp = np.zeros((depth, cap), np.int64)
        self.sample = np.zeros((depth, 3, cap), np.float64)
        self.count = np.zeros(cap, np.int32)
        self.newest = np.zeros(cap, np.int32)
        self.held = np.zeros((7, cap), np.float64)

    def arrays(self):
        return dict(stamp=self.stamp, sample=self.sample.reshape(3 * self.depth, self.cap), count=self.count[None],
                    newest=self.newest[None], held=self.held)

    # ---- the listener ----
    def push(self, stamp_ns, sample, mask=None, why=None):
        """nmpc_batch_push_samples: stamp_ns [B] int64, sample [3][B]; returns dropped [B] uint8. why: a list of B sets
        that receive 'wrap' when a robot's push overwrites its oldest sample"""
        B = len(stamp_ns)
        dropped = np.zeros(B, np.uint8)
        for i in range(B):
            if mask is not None and not mask[i]:
                continue
            c, nw = int(self.count[i]), int(self.newest[i])
            if not np.isfinite(sample[:, i]).all() or (c > 0 and stamp_ns[i] <= self.stamp[nw, i]):
                dropped[i] = 1
                continue
            s = (nw + 1) % self.depth if c > 0 else 0
            if c == self.depth and why is not None:
                why[i].add("wrap")
            self.stamp[s, i] = stamp_ns[i]
            self.sample[s, :, i] = sample[:, i]
            self.newest[i] = s
            self.count[i] = min(c + 1, self.depth)
        return dropped

    # ---- the stage ----
    def stored(self, i):
        """robot i's samples, oldest first: [(stamp, (x, y, yaw))]"""
        c, nw = int(self.count[i]), int(self.newest[i])
        slots = [(nw - k) % self.depth for k in range(c)][::-1]
        return [(int(self.stamp[s, i]), tuple(float(v) for v in self.sample[s, :, i])) for s in slots]

    def lookup(self, i, t, why=None):
        """(x, y, yaw) at stamp t, or None when t is outside the stored stamps (the project's rule)"""
        why = set() if why is None else why
        st = self.stored(i)
        if not st or t < st[0][0] or t > st[-1][0]:
            if st and t < st[0][0]:
                why.add("before_oldest")
            return None
        for ts, p in st:
            if ts == t:
                return p
        k = max(j for j, (ts, _) in enumerate(st) if ts < t)
        (ta, a), (tb, b) = st[k], st[k + 1]
        why.add("interp")
        if k + 1 < len(st) - 1:
            why.add("interp_older_pair")  # the bracketing pair is not the newest two
        r = sec(t - ta) / sec(tb - ta)
        return ((1.0 - r) * a[0] + r * b[0], (1.0 - r) * a[1] + r * b[1], a[2] + r * norm_ang(b[2] - a[2]))

    def stage(self, now_ns, mode, steer=None, steer_ok=None, goal_map=None, **opt):
        """nmpc_batch_node_input for the robots of mode [B]. opt: the scalars of nmpc_node_input (DEFAULTS). Returns a
        dict: valid, moved [B] uint8, pose, vel [3][B] float32, steer_out [B] float32, goal_out [3][B] float32 or None,
        pose_ok, vel_ok [B] bool (True for a robot that did not run) and why, a list of B sets naming what each robot
        met."""
        o = dict(DEFAULTS, **opt)
        B = len(mode)
        held = self.held
        valid, pose_ok, vel_ok = np.ones(B, np.uint8), np.ones(B, bool), np.ones(B, bool)
        ran = np.array([int(m) in (GOTO_POSE, FOLLOW_PATH, BREAK) for m in mode])
        why = [set() for _ in range(B)]
        for i in np.flatnonzero(ran):
            w = why[i]
            st = self.stored(i)
            pose_ok[i] = vel_ok[i] = False
            if not st:
                w.add("empty")
            else:
                t2, p2 = st[-1]
                held[HX, i], held[HY, i] = p2[0], p2[1]
                held[HTH, i] = unwrap_hack(float(held[HTH, i]), p2[2], w)
                pose_ok[i] = not (sec(now_ns - t2) > o["transform_timeout"])
                if not pose_ok[i]:
                    w.add("stale")
                t1 = t2 - o["period_ns"]
                w1 = set()
                p1, q2 = self.lookup(i, t1, w1), self.lookup(i, t2)
                w |= w1
                if p1 is not None and q2 is not None:
                    if "interp" not in w1:
                        w.add("exact")
                    dt = sec(t2 - t1)
                    if not (dt <= 0.0 or dt > o["transform_timeout"]):
                        held[HV, i], held[HVN, i], held[HW, i] = body_velocity(p1, q2, dt)
                        vel_ok[i] = True
            ok = vel_ok[i] if o["pose_valid_overwritten"] else (pose_ok[i] and vel_ok[i])
            if self.tric:
                s_ok = steer_ok is None or bool(steer_ok[i])
                if s_ok:
                    held[HSTEER, i] = float(steer[i]) if steer is not None else 0.0
                else:
                    w.add("steer_bad")
                ok = ok and s_ok
            valid[i] = 1 if ok else 0
        moved = np.zeros(B, np.uint8)
        if math.isfinite(o["recentre_radius"]):
            moved = self.frames.recentre(held[:2, :B].copy(), o["recentre_radius"], ran.astype(np.uint8))
            for i in np.flatnonzero(moved):
                why[i].add("moved")
        origin = np.zeros((2, B))
        if self.frames is not None and self.frames.origin is not None:
            origin = self.frames.origin[:, :B]
        pose = np.stack([held[HX, :B] - origin[0], held[HY, :B] - origin[1], held[HTH, :B]]).astype(np.float32)
        goal_out = None
        if goal_map is not None:
            goal_out = np.stack([goal_map[0] - origin[0], goal_map[1] - origin[1], goal_map[2]]).astype(np.float32)
        return dict(valid=valid, moved=moved, pose=pose, vel=held[HV:HW + 1, :B].astype(np.float32),
                    steer_out=held[HSTEER, :B].astype(np.float32), goal_out=goal_out, pose_ok=pose_ok, vel_ok=vel_ok,
                    why=why, ran=ran)


def strict_gate(valid, mode):
    """nmpc_batch_node_cycle with strict = 1, before the tick: an invalid robot's mode becomes ERROR (in place)"""
    mode[np.asarray(valid) == 0] = ERROR
    return mode


def cycle_status(valid, strict, mode, event, remains=None):
    """the status rule after the tick, in place: strict: event INPUT_INVALID for the invalid robots; else an invalid
    robot whose mode is still GOTO_POSE or FOLLOW_PATH goes to ERROR (remains NaN)"""
    bad = np.asarray(valid) == 0
    if strict:
        event[bad] = EV_INPUT_INVALID
    else:
        hit = bad & ((mode == GOTO_POSE) | (mode == FOLLOW_PATH))
        mode[hit] = ERROR
        if remains is not None:
            remains[hit] = math.nan
    return mode, event
