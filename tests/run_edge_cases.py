"""The edge-case table of run mode's pre-solve (x0 packing, reference unwrap, padding past traj_len, diff's
terminal-weight hack, resets), for tests/test_run_edge_cases.py (CPU: the table is a valid instrument) and
tests/test_gpu_run_edges.py (every kernel form against the fp64 oracle). Pure numpy.

A case is one robot over T = 4 ticks of (pose, vel, steer, traj [N+1][3], traj_len, reset). The pose advances a
little each tick (as tests/ref_wrappers.py:edge_robots), so the iterate is warm from tick 1 on. Every value is built
in fp64 and rounded to fp32 once: the device gets the fp32 value, the oracle the same value widened.

`cases(model, N)` returns the table for any N >= 1 (rows that N makes impossible or that repeat another row are
dropped). The groups:
  len_*    a curving line (0.05 m, 0.03 rad per pose) with traj_len in {1, 2, 3, N//2, N-1, N, N+1, N+5}; the rows of
           traj past traj_len hold a far-away garbage pose (a kernel that reads them is visibly wrong), N+5 says more
           poses are valid than the buffer holds;
  hack_*   full lists at the boundary of diff's terminal-weight hack: the last pose a copy of the one before (on), only
           x equal, x and y equal, x and y equal with the two headings on either side of the +-pi cut (off);
  cut_*    headings across the +-pi cut: the four (theta0, turn) pairs of edge_robots and (pi - 0.2, 0.5) (three of the
           five cross it many times per list), one of those cut short, a go-to-pose goal across it, a pose heading
           outside [-pi, pi], and two exact rows on which fp32 and fp64 must decide alike (delta 3.125: no unwrap;
           delta 3.25: unwrap);
  vel_*    velocities with every component nonzero and of both signs; tric: steer inside and outside the alpha
           bounds, and steer=None;
  reset    the iterate reset at tick 2.
Each case carries what the margins test needs: `hack` ("on": its last two references are equal, by a copy or by
padding; "off": they are distinct), `exact` (one of the two exact rows), and the `marks` the GPU placement uses
("len_N", "multi").
"""
import numpy as np

T = 4
WARM_TICK = 3  # the tick the sensitivity matrix is taken at: warm for every case, the reset case included
RESET_TICK = 2
GARBAGE = (50.0, -50.0, 2.5)
STEP, TURN = 0.05, 0.03
ADVANCE = np.array([0.01, 0.003, 0.002])  # per tick, as edge_robots


def f32(a):
    """round to fp32 once; the widened value is what the oracle gets"""
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def wrap(a):
    return (np.asarray(a, np.float64) + np.pi) % (2.0 * np.pi) - np.pi


def line(p0, heading, n, step=STEP, turn=TURN):
    """n poses from p0 along a curving line, headings wrapped into [-pi, pi)"""
    th = heading + turn * np.arange(1, n + 1)
    xy = np.cumsum(np.stack([step * np.cos(th), step * np.sin(th)], 1), 0) + np.asarray(p0[:2])
    return np.concatenate([xy, wrap(th)[:, None]], 1)


def default_vel(model):
    return [0.3, 0.05 if model == "omni4" else 0.0, 0.2]


class Case:
    """name, ticks (dicts of fp32-valued float64 arrays), hack ('on' / 'off'), exact, marks"""

    def __init__(self, name, ticks, hack, exact=False, marks=()):
        self.name, self.ticks, self.hack, self.exact, self.marks = name, ticks, hack, exact, tuple(marks)


def _tick(N, pose, vel, traj, traj_len, steer, reset):
    buf = np.tile(np.array(GARBAGE), (N + 1, 1))
    n = min(traj_len, N + 1, len(traj))
    buf[:n] = traj[:n]
    return dict(pose=f32(pose), vel=f32(vel), steer=None if steer is None else float(f32(steer)), traj=f32(buf),
                traj_len=int(traj_len), reset=int(reset))


def _case(model, N, name, pose0, make_traj, traj_len=None, vel=None, steer=0.1, advance=ADVANCE, reset_at=None,
          pose_of=None, **kw):
    """make_traj(pose) -> [>= min(traj_len, N+1)][3] for each tick's pose; steer reaches tric alone (the other models'
    ticks carry None, as their callers pass no steer)"""
    ticks = []
    for t in range(T):
        pose = np.asarray(pose0, np.float64) + t * np.asarray(advance)
        if pose_of is not None:
            pose = pose_of(pose)
        ticks.append(_tick(N, pose, default_vel(model) if vel is None else vel, make_traj(pose),
                           N + 1 if traj_len is None else traj_len, steer if model == "tric" else None, reset_at == t))
    return Case(name, ticks, **kw)


def cases(model, N):
    assert N >= 1
    out = []
    # ---- list length -------------------------------------------------------------------------------------------
    seen = set()
    for tag, n in (("1", 1), ("2", 2), ("3", 3), ("half", N // 2), ("N-1", N - 1), ("N", N), ("N+1", N + 1),
                   ("N+5", N + 5)):
        if n < 1 or (n in seen and tag != "N"):
            continue  # traj_len <= 0 is excluded: the reference reads yref[i - 1] at i = 0 there
        if n in seen:  # (small N: traj_len = N repeats an earlier row; keep one row, under the name the placement uses)
            out = [c for c in out if c.ticks[0]["traj_len"] != n]
        seen.add(n)
        out.append(_case(model, N, f"len_{tag}", [0.5, -0.2, 0.3], lambda p: line(p, p[2], N + 1), traj_len=n,
                         hack="on" if n <= N else "off", marks=("len_N",) if tag == "N" else ()))
    # ---- the terminal-weight hack's boundary (full lists) ------------------------------------------------------------
    def hack_list(kind):
        def make(p):
            # the cut case: the line's last two headings are pi - 0.01 and (wrapped) -pi + 0.02
            th0 = np.pi - 0.01 - TURN * N if kind == "xy_cut" else p[2]
            tr = line(p, th0, N + 1)
            if kind == "dup":
                tr[-1] = tr[-2]
            elif kind == "x":
                tr[-1, 0] = tr[-2, 0]
            elif kind in ("xy", "xy_cut"):
                tr[-1, :2] = tr[-2, :2]
            return tr
        return make
    for kind in ("dup", "x", "xy", "xy_cut"):
        p0 = [-1.0, 0.5, wrap(np.pi - 0.01 - TURN * (N + 1))] if kind == "xy_cut" else [-1.0, 0.5, -2.0]
        out.append(_case(model, N, f"hack_{kind}", p0, hack_list(kind),
                         advance=ADVANCE * [1, 1, 0] if kind == "xy_cut" else ADVANCE,
                         hack="on" if kind == "dup" else "off"))
    # ---- the heading cut -----------------------------------------------------------------------------------------
    # edge_robots' four (theta0, turn) pairs, and (pi - 0.2, 0.5); the lists that turn 0.5 rad per pose or more cross the
    # cut several times ((-pi + 0.4, -0.7) is edge_robots' fourth pair already)
    pairs = ((np.pi - 0.03, 0.01), (-np.pi + 0.02, -0.01), (np.pi - 0.001, 0.5), (-np.pi + 0.4, -0.7), (np.pi - 0.2, 0.5))
    for i, (th0, turn) in enumerate(pairs):
        multi = abs(turn) >= 0.5
        out.append(_case(model, N, f"cut_{i}", [1.0, 2.0, th0], lambda p, turn=turn: line(p, p[2], N + 1, turn=turn),
                         steer=-0.2, pose_of=lambda p: np.array([p[0], p[1], float(wrap(p[2]))]),
                         hack="off", marks=("multi",) if multi else ()))
    # a short list whose last valid heading was unwrapped: the padded stages must keep the unwrapped value
    out.append(_case(model, N, "cut_short", [1.0, 2.0, np.pi - 0.2], lambda p: line(p, p[2], N + 1, turn=0.5),
                     traj_len=max(1, N // 2), steer=-0.2, hack="on"))
    goal = np.array([[1.3, 2.1, -3.0]])
    out.append(_case(model, N, "cut_goal", [1.0, 2.0, 3.0], lambda p: goal, traj_len=1, advance=ADVANCE * [1, 1, 0],
                     hack="on"))
    out.append(_case(model, N, "cut_pose_7", [1.0, 2.0, 7.0], lambda p: line(p, p[2], N + 1), hack="off"))
    # exact rows: 3.125, 0.125 and their sums are fp32 numbers, so both precisions see delta = 3.125 < pi (no unwrap)
    # and delta = 3.25 > pi (unwrap)
    for tag, th in (("keep", 0.0), ("unwrap", -0.125)):
        def make(p):
            tr = line(p, 0.0, N + 1, turn=0.0)
            tr[:, 2] = 3.125
            return tr
        out.append(_case(model, N, f"cut_exact_{tag}", [0.2, 0.1, th], make, advance=ADVANCE * [1, 1, 0], hack="off",
                         exact=True))
    # ---- x0 packing --------------------------------------------------------------------------------------------------
    for i, v in enumerate(([0.3, 0.05, 0.2], [-0.2, 0.07, -0.3], [0.25, -0.06, 0.15], [-0.1, -0.04, -0.25])):
        out.append(_case(model, N, f"vel_{i}", [0.0, 0.0, 0.4], lambda p: line(p, p[2], N + 1), vel=v, hack="off"))
    if model == "tric":
        for st in (0.3, 0.785, 1.2, None):
            out.append(_case(model, N, f"steer_{st}", [0.0, 0.0, -0.4], lambda p: line(p, p[2], N + 1),
                             vel=[0.2, 0.0, 0.0], steer=st, hack="off"))
    # ---- reset -------------------------------------------------------------------------------------------------------
    out.append(_case(model, N, "reset", [-0.3, 0.7, 1.0], lambda p: line(p, p[2], N + 1), reset_at=RESET_TICK,
                     hack="off"))
    return out


def batch_inputs(cs, tick, order=None):
    """AoS fp64 inputs of one tick for Oracle.batch_tick (and, transposed and narrowed, the device): pose [B][3],
    vel [B][3], steer [B] (None entries as 0), traj [B][N+1][3], traj_len int32 [B], reset uint8 [B]; order: indices
    into cs (the placement)"""
    order = range(len(cs)) if order is None else order
    tk = [cs[i].ticks[tick] for i in order]
    return (np.ascontiguousarray([t["pose"] for t in tk], np.float64),
            np.ascontiguousarray([t["vel"] for t in tk], np.float64),
            np.ascontiguousarray([0.0 if t["steer"] is None else t["steer"] for t in tk], np.float64),
            np.ascontiguousarray([t["traj"] for t in tk], np.float64),
            np.ascontiguousarray([t["traj_len"] for t in tk], np.int32),
            np.ascontiguousarray([t["reset"] for t in tk], np.uint8))


def placements(cs, min_B=0):
    """The batches of the GPU test: one list of indices into cs per marked case m ("len_N", "multi"). In batch m, case
    m sits in slot 0 and in the last slot, every marked case sits once on each side of a 16-robot boundary (slots
    16 i - 1 and 16 i), every case of the table appears, and B is at least min_B and no multiple of 4 (so none of 16)."""
    marked = [i for i, c in enumerate(cs) if c.marks]
    rest = [i for i in range(len(cs)) if i not in marked]
    out = []
    for j, m in enumerate(marked):
        nf = [0]

        def fill(n):
            got = [rest[(nf[0] + i) % len(rest)] for i in range(n)]
            nf[0] += n
            return got
        o = [m] + fill(14)
        for q in [m] + marked[j + 1:] + marked[:j]:
            assert len(o) % 16 == 15
            o += [q, q] + fill(14)
        while nf[0] < len(rest) or len(o) + 1 < min_B or (len(o) + 1) % 4 == 0:
            o += fill(1)
        out.append(o + [m])
    return out
