"""The case stream of the node input tests: 12 control cycles of jittered localisation samples for B = 21 robots at
tests/frame_cases.py's offsets (a UTM-sized map), with the listener's and the stage's edge cases planted robot by
robot. tests/test_node_input_ref.py asserts on the CPU that every planted case really occurs; tests/test_gpu_node_input.py
runs the stream on the device. Host side only, seeded.

A cycle is dict(now_ns, pushes=[(stamp [B] int64, sample [3][B], mask [B] uint8), ...], mode [B] uint8, steer [B]
float32, steer_ok [B] uint8, goal_map [3][B]). Robots by role (every other robot: jittered stamps, 40 or 80 Hz):
   0  never pushed: an empty ring              1  pushes stop after cycle 5: a stale newest sample
   2  stamps exactly one period apart          3  turns left through +pi and on past 2 pi (unwrap, then the clamp)
   4  turns right through -pi and past -2 pi   5  cycle 4: a second push with an older stamp (dropped)
   6  cycle 5: a push with a NaN x (dropped)   7  steer_ok = 0 in cycles 3 and 4
   8  drives 1.5 m per cycle: crosses the recentre radius again and again
   9  IDLE, 10 ERROR, 11 a mode value of 7, 12 BREAK: the first three do not run the stage
  13  masked off in cycles 6..8 (a gap in its ring)
"""
import math

import numpy as np

from tests.frame_cases import per_robot

B, CAP, CYCLES = 21, 37, 12
PERIOD_NS = 25000000
T0 = 1700000000123456789  # an epoch stamp: the whole-second part of sec() is not 0
SEED = 20240611
RADIUS = 4.0
IDLE, GOTO_POSE, FOLLOW_PATH, BREAK, ERROR = range(5)


def modes():
    m = np.where(np.arange(B) % 2 == 0, GOTO_POSE, FOLLOW_PATH).astype(np.uint8)
    m[9], m[10], m[11], m[12] = IDLE, ERROR, 7, BREAK
    return m


def truth(i, t_ns):
    """robot i's (x, y, yaw) in map coordinates at stamp t_ns, yaw within [-pi, pi] as tf2::getYaw gives it"""
    ox, oy = per_robot(B)[i]
    s = (t_ns - T0) / PERIOD_NS  # cycles since T0, a float
    if i == 3 or i == 4:
        sign = 1.0 if i == 3 else -1.0
        yaw = sign * (2.9 + 0.55 * s)
        x, y = ox + 0.3 * i + 0.02 * s, oy - 0.2 * i
    elif i == 8:
        yaw = 0.1
        x, y = ox + 1.5 * s, oy + 0.15 * s
    else:
        w = 0.02 + 0.004 * i  # rad per cycle
        yaw = 0.3 * i + w * s
        x, y = ox + 0.5 * i + 2.0 * math.cos(yaw), oy - 0.25 * i + 2.0 * math.sin(yaw)
    yaw = math.fmod(yaw + math.pi, 2.0 * math.pi)
    yaw = (yaw + 2.0 * math.pi if yaw < 0.0 else yaw) - math.pi
    return x, y, yaw


def stream():
    rng = np.random.default_rng(SEED)
    lag = rng.integers(2000000, 9000000, B)  # localisation latency per robot, ns
    cycles = []
    for c in range(CYCLES):
        now = T0 + c * PERIOD_NS
        jit = rng.integers(-3000000, 3000001, B)
        stamp = now - lag + jit
        stamp[2] = now - lag[2]  # robot 2: no jitter
        pushes = []
        # the 80 Hz robots get a sample half a period earlier first
        fast = (np.arange(B) % 4 == 1) & (np.arange(B) > 13)
        if fast.any():
            early = stamp - PERIOD_NS // 2 + rng.integers(-1000000, 1000001, B)
            pushes.append((early, fast.astype(np.uint8)))
        mask = np.ones(B, np.uint8)
        mask[0] = 0
        if c > 5:
            mask[1] = 0
        if 6 <= c <= 8:
            mask[13] = 0
        pushes.append((stamp, mask))
        if c == 4:  # robot 5: out of order
            late = stamp.copy()
            late[5] = stamp[5] - 7000000
            pushes.append((late, (np.arange(B) == 5).astype(np.uint8)))
        out = []
        for st, mk in pushes:
            st = st.astype(np.int64)
            smp = np.array([truth(i, int(st[i])) for i in range(B)]).T.copy()
            out.append((st, smp, mk))
        if c == 5:  # robot 6: a NaN sample with a good stamp (one more push, so the good one of this cycle is stored)
            st = (stamp + 1000000).astype(np.int64)
            smp = np.array([truth(i, int(st[i])) for i in range(B)]).T.copy()
            smp[0, 6] = math.nan
            out.append((st, smp, (np.arange(B) == 6).astype(np.uint8)))
        steer = (0.01 * np.arange(B) + 0.002 * c).astype(np.float32)
        steer_ok = np.ones(B, np.uint8)
        if c in (3, 4):
            steer_ok[7] = 0
        goal = np.array([truth(i, now + 40 * PERIOD_NS) for i in range(B)]).T.copy()
        cycles.append(dict(now_ns=int(now), pushes=out, mode=modes(), steer=steer, steer_ok=steer_ok, goal_map=goal))
    return cycles
