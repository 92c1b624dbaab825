"""A numpy fp64 restatement of run mode's pre-solve (oc_prepare, oracle/nmpc_oracle.c, itself pinned bit for bit to the
reference's executed run() by tests/test_reference_wrappers.py) with switchable mistakes, each of the kind a kernel's
loop can make. tests/test_run_edge_cases.py shows with it that the case table of tests/run_edge_cases.py would see
every one of them: with mistake=None prepare() equals Oracle.prepare bit for bit on every case, and with a mistake
the oracle's solve from the mistaken (x0, yref, We) moves by at least ten times the GPU test's tolerance on some case.

  pad_prev        pad with the pose before the last valid one
  pad_raw         read past traj_len, no padding
  hack_xy         the terminal-weight hack compares x and y only
  hack_never      the hack never fires
  hack_always     the hack always fires
  no_unwrap       no unwrap at all
  unwrap_vs_pose  every reference is unwrapped against the pose heading instead of the previous reference
  unwrap_pad      the padded stages are unwrapped again: the last valid pose's raw heading is compared with the previous
                  (unwrapped) reference and the 2 pi step it calls for is applied to that reference once more. (Unwrapping
                  the raw heading itself again is idempotent, so a loop that does that is right.)
  kin_swap        left and right (diff), the wheel order (omni4), speed and steering angle (tric) swapped in the
                  direct kinematics
  carry_stale     x0's reference states from the resident iterate's stage 1 (x1_prev) instead of the carried values
"""
import numpy as np

MISTAKES = ("pad_prev", "pad_raw", "hack_xy", "hack_never", "hack_always", "no_unwrap", "unwrap_vs_pose", "unwrap_pad",
            "kin_swap", "carry_stale")
HACK_MISTAKES = ("hack_xy", "hack_never", "hack_always")  # diff only: the other models have no hack


def applies(model, mistake):
    """whether the model has the step the mistake is made in"""
    return model == "diff" or mistake not in HACK_MISTAKES


def unwrap_angle(current, previous):
    delta = current - previous
    if delta > np.pi:
        current -= 2 * np.pi
    elif delta < -np.pi:
        current += 2 * np.pi
    return current


def direct_kinematics(model, p, vel, steer, swap=False):
    if model == "diff":
        hl = 0.5 * p[0] * vel[2]
        xv = [vel[0] - hl, vel[0] + hl]
        return xv[::-1] if swap else xv
    if model == "omni4":
        hl = 0.5 * p[0] * vel[2]
        xv = [vel[0] - vel[1] - hl, -vel[0] - vel[1] - hl, vel[0] + vel[1] - hl, -vel[0] + vel[1] - hl]
        return [xv[1], xv[0], xv[3], xv[2]] if swap else xv
    return [steer, vel[0]] if swap else [vel[0], steer]


def prepare(model, prm, pose, vel, steer, traj, carried, mistake=None, traj_len=None, x1_prev=None):
    """(x0, yref, We) of one robot. traj: the reference buffer [n][3]; traj_len: poses valid (None: all n; more than
    n says so and only the buffer is read, as the device API's traj_len > N + 1). x1_prev [nx]: the resident
    iterate's stage 1, read by carry_stale alone."""
    assert mistake is None or mistake in MISTAKES, mistake
    N, nx, ny, nbx = prm.N, prm.nx, prm.ny, prm.nbx
    traj = np.asarray(traj, np.float64).reshape(-1, 3)
    ntraj = len(traj) if traj_len is None else int(traj_len)
    steer = 0.0 if steer is None else float(steer)
    x0 = np.zeros(nx)
    x0[:3] = pose
    xv = direct_kinematics(model, prm.p, vel, steer, swap=mistake == "kin_swap")
    x0[3:3 + len(xv)] = xv
    for i in range(nbx):
        x0[prm.idxbx[i]] = x1_prev[prm.idxbx[i]] if mistake == "carry_stale" else carried[i]
    yref = np.zeros((N + 1, ny))
    prev = float(pose[2])
    for k in range(N + 1):
        inside = k < ntraj or (mistake == "pad_raw" and k < len(traj))
        if inside:
            th = traj[k, 2]
            if mistake == "no_unwrap":
                pass
            elif mistake == "unwrap_vs_pose":
                th = unwrap_angle(th, float(pose[2]))
            else:
                th = unwrap_angle(th, prev)
            yref[k, :3] = traj[k, 0], traj[k, 1], th
            prev = th
        else:
            src = k - 1
            if mistake == "pad_prev":
                src = max(ntraj - 2, 0)
            yref[k, :3] = yref[src, :3]
            if mistake == "unwrap_pad":
                raw = traj[ntraj - 1, 2]
                yref[k, 2] = yref[k - 1, 2] + (unwrap_angle(raw, yref[k - 1, 2]) - raw)
    We = np.array(prm.W_e[:nx], np.float64)
    if prm.terminal_hack:
        a, b = yref[N], yref[N - 1]
        eq = a[0] == b[0] and a[1] == b[1] and (a[2] == b[2] or mistake == "hack_xy")
        if mistake == "hack_never":
            eq = False
        elif mistake == "hack_always":
            eq = True
        for i in range(3):
            We[i] = 100.0 * prm.W[i] if eq else prm.W[i]
    return x0, yref, We


def unwrap_deltas(pose, traj, traj_len):
    """the deltas |current - previous| of every unwrap decision of a correct pre-solve (stages inside the list)"""
    traj = np.asarray(traj, np.float64).reshape(-1, 3)
    prev, out = float(pose[2]), []
    for k in range(min(int(traj_len), len(traj))):
        out.append(traj[k, 2] - prev)
        prev = unwrap_angle(traj[k, 2], prev)
    return np.array(out)
