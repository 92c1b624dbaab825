#!/usr/bin/env python3
"""Time the batched PathDiscretizer (nmpc_path_discretize) on the device: seeded multi-segment paths
(lines and cubic Beziers, 1-4 segments per robot), N+1 = 41 poses per robot at dt = 1/40 s, inputs resident in
HBM. Prints one JSON line: robots/s, ms per launch (HIP events on the launch stream), bytes moved per launch.

With --nearest: the nearest-point search (nmpc_path_nearest) on the same paths, one JSON line of the same form,
with the discretize launch timed in the same process next to it.

With --tick: a whole path-following tick of diff robots (N = num_poses - 1), the two-launch form
(nmpc_path_discretize + nmpc_batch_run) against the one-launch nmpc_batch_run_path and against
nmpc_batch_follow_path (nearest point + run_path + path-error check), ms per tick each.

With --node: nmpc_batch_node_tick on a mixed fleet of diff robots (N = num_poses - 1) at B = 4096 and 1024 with 100 %,
50 % and 25 % of the robots active (half of them following a seeded path, half driving to a seeded goal 0.3-1 m
away), the others Idle and scattered uniformly over the indices. In the same process, on the same references:
nearest + discretize + run over the full B, and over a batch holding just the active robots. Three interleaved
rounds of each, the median; one JSON line per (B, fraction).

With --mission: nmpc_batch_node_tick_queue, the node tick that keeps each robot's path-set queue on the device, on
--node's fleet with every robot active (B = 4096 and 1024, diff): the queue tick on one-part sets against
nmpc_batch_node_tick on the same paths (the cost of the queue), and the queue tick on three-part sets (each robot's
path as the first part of a forward / reverse / forward set, so that the window logic has parts to look at). Five
interleaved timed windows of each after a warm-up, median and spread; one JSON line per B.

With --cycle: nmpc_batch_node_cycle (the input stage, the node tick and the status rule in one call, from fp64 map
samples) on --node's mixed fleet, against nmpc_batch_node_tick on a twin handle fed the inputs the stage emitted
(prepared beforehand: what a caller with a host-side getInputData hands over), and the stage's and the listener's
launches alone. Three interleaved rounds of each, the median; one JSON line per (B, fraction). With --speed-map as
well: two more handles of the same sizes run node_cycle in the same rounds, one with a seeded speed map attached
(256 x 256 cells of 0.25 m about the fleet, limits in [0.15, 1), a fifth of the cells without one) and one with a map
that holds no limit (the writer runs and the stage table is on, but the QPs are those without a map), and the map's
writer (nmpc_batch_stage_limits_from_map) is timed alone: node_cycle_map_ms, node_cycle_open_map_ms and writer_ms next
to the figures without a map. With --dump-failed OUT.npz as well: no timings; the B = 1024, all-active handle with the seeded map
runs one node_cycle at a time with host copies of what each solve reads, stops at the first nonzero solver status and
writes that robot's whole history since its cold start to OUT.npz (tests/golden/make_saturated_fixture.md).

Poses of --nearest and --tick: the path points at the seeded nearest_u, displaced by a seeded offset of up to 0.1 m.

usage: python tools/bench_path.py [--B 4096] [--num-poses 41] [--iters 50] [--nearest | --tick | --node | --mission |
                                                                                     --cycle [--speed-map
                                                                                     [--dump-failed OUT.npz]]]
"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nmpc_nav_control_amd.path import SEG_DOUBLES, discretize  # noqa: E402


def seeded_paths(B, max_segs=4, seed=20250824):
    rng = np.random.default_rng(seed)
    segs = np.zeros((B, max_segs, SEG_DOUBLES))
    nseg = rng.integers(1, max_segs + 1, B).astype(np.int32)
    p = rng.uniform(-2, 2, (B, 2))
    h = rng.uniform(-math.pi, math.pi, B)
    for j in range(max_segs):
        L = rng.uniform(0.5, 1.5, B)
        turn = rng.uniform(-1.0, 1.0, B)
        q = p + L[:, None] * np.stack([np.cos(h + turn / 2), np.sin(h + turn / 2)], 1)
        a = (L / 3)[:, None]
        P1 = p + a * np.stack([np.cos(h), np.sin(h)], 1)
        P2 = q - a * np.stack([np.cos(h + turn), np.sin(h + turn)], 1)
        c = [p, 3 * (P1 - p), 3 * (P2 - 2 * P1 + p), q - 3 * P2 + 3 * P1 - p]
        for k in range(4):
            segs[:, j, k], segs[:, j, 4 + k] = c[k][:, 0], c[k][:, 1]
        segs[:, j, 8] = h
        segs[:, j, 12] = rng.uniform(0.2, 0.8, B)
        p, h = q, h + turn
    nearest_u = rng.uniform(0, 1, B) * 0.5
    return segs, nseg, nearest_u


def seeded_poses(segs, nseg, nearest_u, seed=20250825):
    """[3][B] float32: each robot at the point of its path at nearest_u, moved by up to 0.1 m per axis"""
    rng = np.random.default_rng(seed)
    B = len(nseg)
    k = np.minimum(np.floor(nearest_u).astype(int), nseg - 1)
    u = nearest_u - k
    c = segs[np.arange(B), k]
    pw = np.stack([u ** 0, u, u ** 2, u ** 3], 1)
    x, y = (c[:, 0:4] * pw).sum(1), (c[:, 4:8] * pw).sum(1)
    dx, dy = (c[:, 1:4] * pw[:, :3] * [1, 2, 3]).sum(1), (c[:, 5:8] * pw[:, :3] * [1, 2, 3]).sum(1)
    off = rng.uniform(-0.1, 0.1, (2, B))
    return np.stack([x + off[0], y + off[1], np.arctan2(dy, dx)]).astype(np.float32)


def timed(fn, iters, stream):
    """ms per call of fn: 5 warm-up calls, then `iters` calls between two HIP events on the launch stream"""
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(iters):
        fn()
    e1.record(stream)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def nearest_bench(a):
    from nmpc_nav_control_amd.path import nearest
    dev = torch.device("cuda:0")
    segs, nseg, nu = seeded_paths(a.B)
    S, NS, U = (torch.from_numpy(x).to(dev) for x in (segs, nseg, nu))
    P = torch.from_numpy(seeded_poses(segs, nseg, nu)).to(dev)
    err = torch.empty((2, a.B), dtype=torch.float64, device=dev)
    traj = torch.empty((a.num_poses, 3, a.B), dtype=torch.float32, device=dev)
    stream = torch.cuda.current_stream()
    # three interleaved rounds of both launches in one process; the median of each
    ms_n, ms_d = [], []
    for _ in range(3):
        ms_n.append(timed(lambda: nearest(S, NS, P, err=err), a.iters, stream))
        ms_d.append(timed(lambda: discretize(S, NS, U, 1 / 40, a.num_poses, traj=traj), a.iters, stream))
    ms, msd = sorted(ms_n)[1], sorted(ms_d)[1]
    # compulsory bytes: the segment records, nseg and the pose in, nearest_u and the two errors out
    nbytes = int(nseg.sum()) * SEG_DOUBLES * 8 + a.B * (4 + 12) + a.B * 3 * 8
    print(json.dumps(dict(metric="nearest path point robots/s", value=round(a.B / (ms * 1e-3), 1), B=a.B,
                          ms_per_launch=round(ms, 4), ms_rounds=[round(m, 4) for m in ms_n],
                          discretize_ms_per_launch=round(msd, 4), num_poses=a.num_poses,
                          bytes_per_launch=nbytes, achieved_GBs=round(nbytes / (ms * 1e-3) / 1e9, 2),
                          bound="fp64 issue (16 lanes per robot: 16 samples + 8 Newton steps per segment)")),
          flush=True)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=4096)
    ap.add_argument("--num-poses", type=int, default=41)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--tick", action="store_true")
    ap.add_argument("--nearest", action="store_true")
    ap.add_argument("--node", action="store_true")
    ap.add_argument("--mission", action="store_true")
    ap.add_argument("--cycle", action="store_true")
    ap.add_argument("--speed-map", action="store_true", help="with --cycle: node_cycle with a speed map attached too")
    ap.add_argument("--dump-failed", metavar="OUT.npz", help="with --cycle --speed-map: no timings; run the B = 1024 "
                    "all-active map handle tick by tick and write the first failing robot's history")
    a = ap.parse_args(argv)
    if a.dump_failed:
        if not (a.cycle and a.speed_map):
            ap.error("--dump-failed needs --cycle --speed-map")
        return dump_failed(a)
    if a.cycle:
        return cycle_bench(a)
    if a.mission:
        return mission_bench(a)
    if a.node:
        return node_bench(a)
    if a.nearest:
        return nearest_bench(a)
    if a.tick:
        return tick(a)
    dev = torch.device("cuda:0")
    segs, nseg, nu = seeded_paths(a.B)
    S, NS, U = (torch.from_numpy(x).to(dev) for x in (segs, nseg, nu))
    traj = torch.empty((a.num_poses, 3, a.B), dtype=torch.float32, device=dev)
    stream = torch.cuda.current_stream()
    for _ in range(5):
        discretize(S, NS, U, 1 / 40, a.num_poses, traj=traj)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(a.iters):
        discretize(S, NS, U, 1 / 40, a.num_poses, traj=traj)
    e1.record(stream)
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / a.iters
    # compulsory bytes: each robot's segment records + nseg + nearest_u in, the fp32 poses out
    nbytes = int(nseg.sum()) * SEG_DOUBLES * 8 + a.B * (4 + 8) + a.num_poses * 3 * 4 * a.B
    print(json.dumps(dict(metric="getNextNPoses robots/s", value=round(a.B / (ms * 1e-3), 1), B=a.B,
                          num_poses=a.num_poses, ms_per_launch=round(ms, 4), bytes_per_launch=nbytes,
                          achieved_GBs=round(nbytes / (ms * 1e-3) / 1e9, 2),
                          bound="latency (sequential fp64 march per robot)")), flush=True)


def tick(a):
    """Path-following tick: discretize + run (two launches) vs run_path (one launch) vs follow_path (nearest point +
    run_path + path-error check), same robots and state. Each variant runs its own solver handle through `iters`
    warm-started ticks on fixed measurements; follow_path feeds its path_u back (0 at the first tick)."""
    from nmpc_nav_control_amd.batch import BatchSolver
    from nmpc_nav_control_amd.path import discretize as disc
    dev = torch.device("cuda:0")
    N, B = a.num_poses - 1, a.B
    segs, nseg, nu = seeded_paths(B)
    S, NS, U = (torch.from_numpy(x).to(dev) for x in (segs, nseg, nu))
    traj = torch.empty((N + 1, 3, B), dtype=torch.float32, device=dev)
    disc(S, NS, U, 1 / 40, N + 1, traj=traj)
    pose = torch.from_numpy(seeded_poses(segs, nseg, nu)).to(dev)
    vel = torch.zeros(3, B, device=dev)
    path_u = torch.zeros(B, dtype=torch.float64, device=dev)
    err = torch.empty((2, B), dtype=torch.float64, device=dev)
    off = torch.empty(B, dtype=torch.uint8, device=dev)
    res = {}
    for name in ("two_launch", "one_launch", "follow_path"):
        s = BatchSolver("diff", N, B, device=dev)
        u0 = torch.zeros(2, B, device=dev)
        st = torch.zeros(B, dtype=torch.int32, device=dev)

        def step():
            if name == "two_launch":
                disc(S, NS, U, 1 / 40, N + 1, traj=traj)
                s.run(pose, vel, traj, u0=u0, status=st)
            elif name == "one_launch":
                s.run_path(pose, vel, S, NS, U, 1 / 40, traj_out=None, u0=u0, status=st)
            else:
                s.follow_path(pose, vel, S, NS, path_u, 1 / 40, max_pos_err=1.0, max_ori_err=math.pi, err=err,
                              off_path=off, u0=u0, status=st)
        for _ in range(5):
            step()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            step()
        e1.record()
        torch.cuda.synchronize()
        res[name] = round(e0.elapsed_time(e1) / a.iters, 4)
        res[name + "_failed"] = int((st != 0).sum())
    print(json.dumps(dict(metric="path-following tick ms (diff N=%d, B=%d)" % (N, B), **res)), flush=True)


def node_bench(a):
    """node_tick against nearest + discretize + run (see the module docstring). Every handle runs warm-started ticks
    on fixed measurements; path_u is fed back. `dropped` counts robots whose mode changed during the run (a failed
    solve sends a robot to Error, which would shrink the active set)."""
    from nmpc_nav_control_amd._lib import NODE_FOLLOW_PATH, NODE_GOTO_POSE
    from nmpc_nav_control_amd.batch import BatchSolver, NodeParams
    from nmpc_nav_control_amd.path import nearest
    dev = torch.device("cuda:0")
    N = a.num_poses - 1
    npar = NodeParams.default()
    stream = torch.cuda.current_stream()
    i32, f64 = torch.int32, torch.float64
    for B in (4096, 1024):
        segs, nseg, nu = seeded_paths(B)
        pose = seeded_poses(segs, nseg, nu)
        rng = np.random.default_rng(B)
        ang, r = rng.uniform(-math.pi, math.pi, B), rng.uniform(0.3, 1.0, B)
        goal = np.stack([pose[0] + r * np.cos(ang), pose[1] + r * np.sin(ang),
                         pose[2] + rng.uniform(0.2, 1.0, B)]).astype(np.float32)
        perm = rng.permutation(B)
        for frac in (1.0, 0.5, 0.25):
            k = int(B * frac)
            act = np.sort(perm[:k])
            mode = np.zeros(B, np.uint8)
            mode[act[0::2]] = NODE_FOLLOW_PATH
            mode[act[1::2]] = NODE_GOTO_POSE
            t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731

            def fleet(idx):
                """device inputs of the robots idx (a compact batch) and their outputs"""
                n = len(idx)
                d = dict(S=t(segs[idx]), NS=t(nseg[idx]), P=t(pose[:, idx]), V=torch.zeros(3, n, device=dev),
                         G=t(goal[:, idx]), M=t(mode[idx]), U=torch.zeros(n, dtype=f64, device=dev),
                         err=torch.empty((2, n), dtype=f64, device=dev), traj=torch.empty((N + 1, 3, n), device=dev),
                         u0=torch.zeros(2, n, device=dev), st=torch.zeros(n, dtype=i32, device=dev),
                         nan=torch.full((n,), math.nan, dtype=f64, device=dev))
                d["solver"] = BatchSolver("diff", N, n, device=dev)
                return d

            node, full, small = fleet(np.arange(B)), fleet(np.arange(B)), fleet(act)
            nsolved = torch.zeros(1, dtype=i32, device=dev)
            tref = torch.empty((N + 1, 3, B), device=dev)

            def node_step():
                d = node
                d["solver"].node_tick(npar, d["M"], d["P"], d["V"], goal=d["G"], segs=d["S"], nseg=d["NS"],
                                      path_u=d["U"], err=d["err"], traj_out=tref, n_solved=nsolved, u0=d["u0"],
                                      status=d["st"])

            # the references of the parts: what the node tick solved on (the goal repeated, or the path poses)
            node_step()
            torch.cuda.synchronize()
            node["solver"].init_iterate()
            node["U"].zero_()
            ref_full = torch.where(torch.isnan(tref), node["P"][None].expand(N + 1, 3, B), tref).contiguous()
            len_full = torch.where(node["M"] == NODE_GOTO_POSE, 1, N + 1).to(i32)
            ai = t(act)
            ref_small, len_small = ref_full[:, :, ai].contiguous(), len_full[ai].contiguous()

            def parts_step(d, ref, ln):
                d["U"] = nearest(d["S"], d["NS"], d["P"], torch.stack([d["U"], d["nan"]]), err=d["err"])
                discretize(d["S"], d["NS"], d["U"], 1 / 40, N + 1, traj=d["traj"])
                d["solver"].run(d["P"], d["V"], ref, traj_len=ln, u0=d["u0"], status=d["st"])

            ms = {"node_tick": [], "parts_full": [], "parts_active": []}
            for _ in range(3):
                ms["node_tick"].append(timed(node_step, a.iters, stream))
                ms["parts_full"].append(timed(lambda: parts_step(full, ref_full, len_full), a.iters, stream))
                ms["parts_active"].append(timed(lambda: parts_step(small, ref_small, len_small), a.iters, stream))
            med = {k_: sorted(v)[1] for k_, v in ms.items()}
            dropped = int((node["M"].cpu() != t(mode).cpu()).sum())
            plan_b, plan_k = node["solver"].plan_ex(B, "run"), small["solver"].plan_ex(k, "run")
            print(json.dumps(dict(
                metric="node tick ms (diff N=%d)" % N, B=B, active=k, n_solved=int(nsolved.cpu()), dropped=dropped,
                node_tick_ms=round(med["node_tick"], 4), parts_full_ms=round(med["parts_full"], 4),
                parts_active_ms=round(med["parts_active"], 4),
                node_over_parts_full=round(med["node_tick"] / med["parts_full"], 3),
                node_over_parts_active=round(med["node_tick"] / med["parts_active"], 3),
                rounds={k_: [round(x, 4) for x in v] for k_, v in ms.items()},
                failed=dict(node=int((node["st"] != 0).sum()), full=int((full["st"] != 0).sum()),
                            active=int((small["st"] != 0).sum())),
                form_B="%s w%d" % (plan_b["kernel"], plan_b["waves_per_robot"]),
                form_active="%s w%d" % (plan_k["kernel"], plan_k["waves_per_robot"]))), flush=True)


def cycle_bench(a):
    """node_cycle against node_tick on host-prepared inputs (see the module docstring). Both handles run warm-started
    ticks on fixed samples with path_u fed back, as --node does; the rings (depth 4) hold two samples per robot one
    period apart, so every active robot's pose and velocity are valid."""
    from nmpc_nav_control_amd._lib import NODE_FOLLOW_PATH, NODE_GOTO_POSE
    from nmpc_nav_control_amd.batch import BatchSolver, NodeInput, NodeParams
    dev = torch.device("cuda:0")
    N = a.num_poses - 1
    npar = NodeParams.default()
    stream = torch.cuda.current_stream()
    i32, f64, now, period = torch.int32, torch.float64, 1700000000000000000, 25000000
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    smap = None
    if a.speed_map:
        from nmpc_nav_control_amd.batch import SpeedMap
        rng = np.random.default_rng(20250826)
        grid = rng.uniform(0.15, 1.0, (256, 256)).astype(np.float32)
        grid[rng.uniform(size=grid.shape) < 0.2] = np.inf
        smap = SpeedMap(-32.0, -32.0, 0.25, t(grid))
        smap_open = SpeedMap(-32.0, -32.0, 0.25, t(np.full((256, 256), np.inf, np.float32)))
    for B in (4096, 1024):
        segs, nseg, nu = seeded_paths(B)
        pose = seeded_poses(segs, nseg, nu).astype(np.float64)
        rng = np.random.default_rng(B)
        ang, r = rng.uniform(-math.pi, math.pi, B), rng.uniform(0.3, 1.0, B)
        goal = np.stack([pose[0] + r * np.cos(ang), pose[1] + r * np.sin(ang), pose[2] + rng.uniform(0.2, 1.0, B)])
        perm = rng.permutation(B)
        for frac in (1.0, 0.5, 0.25):
            k = int(B * frac)
            act = np.sort(perm[:k])
            mode = np.zeros(B, np.uint8)
            mode[act[0::2]] = NODE_FOLLOW_PATH
            mode[act[1::2]] = NODE_GOTO_POSE

            def handle():
                return dict(solver=BatchSolver("diff", N, B, device=dev), S=t(segs), NS=t(nseg), M=t(mode),
                            U=torch.zeros(B, dtype=f64, device=dev), u0=torch.zeros(2, B, device=dev),
                            st=torch.zeros(B, dtype=i32, device=dev))

            cyc, tick = handle(), handle()
            stamp, smp = t(np.full(B, now - 2000000, np.int64)), t(pose)
            s = cyc["solver"]
            s.enable_input(4)
            s.push_samples(stamp - period, smp)
            s.push_samples(stamp, smp)
            buf = dict(pose=torch.zeros(3, B, device=dev), vel=torch.zeros(3, B, device=dev),
                       valid=torch.zeros(B, dtype=torch.uint8, device=dev))
            nin, G = NodeInput.default(now_ns=now, **buf), t(goal)
            gout = torch.zeros(3, B, device=dev)
            nsolved = torch.zeros(1, dtype=i32, device=dev)

            def stage_step():
                s.node_input(nin, cyc["M"], goal_map=G, goal_out=gout)

            def push_step():  # (the same stamp again: every sample is dropped, after the same reads)
                s.push_samples(stamp, smp)

            def cycle_step():
                d = cyc
                s.node_cycle(npar, nin, d["M"], goal_map=G, segs=d["S"], nseg=d["NS"], path_u=d["U"],
                             n_solved=nsolved, u0=d["u0"], status=d["st"])

            stage_step()  # the host-prepared inputs of the twin: what the stage emits
            torch.cuda.synchronize()
            P, V, G32 = buf["pose"].clone(), buf["vel"].clone(), gout.clone()

            def tick_step():
                d = tick
                d["solver"].node_tick(npar, d["M"], P, V, goal=G32, segs=d["S"], nseg=d["NS"], path_u=d["U"],
                                      u0=d["u0"], status=d["st"])

            steps = {"node_cycle": cycle_step, "node_tick": tick_step, "stage": stage_step, "push": push_step}
            mapped = {}
            if smap is not None:
                # two more handles on the same fleet and samples: the seeded map attached, and a map without a limit
                # (the table is on and the writer runs, but every box is the handle's: the same QPs as without a map)
                vlim = torch.zeros(N + 1, B, device=dev)

                def attach(m, fresh):
                    d = handle()
                    d["solver"].enable_input(4)
                    d["solver"].push_samples(stamp - period, smp)
                    d["solver"].push_samples(stamp, smp)
                    d["solver"].set_speed_map(m)
                    d["nin"] = NodeInput.default(now_ns=now, **{k_: torch.zeros_like(v) for k_, v in buf.items()})
                    # the robots have no iterate yet, which the caller of a map flags: consumed by the first solve.
                    # (Not on the handle whose map holds no limit: its ticks are to be those of the handle without one)
                    d["fresh"] = torch.ones(B, dtype=torch.uint8, device=dev) if fresh else None
                    return d

                def map_cycle(d):
                    d["solver"].node_cycle(npar, d["nin"], d["M"], goal_map=G, segs=d["S"], nseg=d["NS"],
                                           path_u=d["U"], reset=d["fresh"], u0=d["u0"], status=d["st"])

                mapped = dict(node_cycle_map=attach(smap, True), node_cycle_open_map=attach(smap_open, False))
                for k_, d in mapped.items():
                    steps[k_] = lambda d=d: map_cycle(d)
                steps["writer"] = lambda: mapped["node_cycle_map"]["solver"].stage_limits_from_map(smap, pose=P,
                                                                                                    vlim=vlim)
            ms = {k_: [] for k_ in steps}
            for _ in range(3):
                for k_, fn in steps.items():
                    ms[k_].append(timed(fn, a.iters, stream))
            med = {k_: sorted(v)[1] for k_, v in ms.items()}
            same = all(torch.equal(cyc[k_], tick[k_]) for k_ in ("u0", "st", "M", "U"))
            extra = {}
            if smap is not None:
                mp, op = mapped["node_cycle_map"], mapped["node_cycle_open_map"]
                extra = dict(node_cycle_map_ms=round(med["node_cycle_map"], 4),
                             node_cycle_open_map_ms=round(med["node_cycle_open_map"], 4),
                             writer_ms=round(med["writer"], 4),
                             open_map_minus_cycle_ms=round(med["node_cycle_open_map"] - med["node_cycle"], 4),
                             map_minus_open_map_ms=round(med["node_cycle_map"] - med["node_cycle_open_map"], 4),
                             limited_stages=round(float((vlim[:, t(act)] < 1.0).float().mean()), 3),
                             open_map_equals_cycle=all(torch.equal(cyc[k_], op[k_]) for k_ in ("u0", "st", "M", "U")),
                             failed_map=int((mp["st"] != 0).sum()),
                             dropped_map=int((mp["M"].cpu() != t(mode).cpu()).sum()),
                             error_map=int((mp["M"] == 4).sum()))
            print(json.dumps(dict(
                metric="node cycle ms (diff N=%d)" % N, B=B, active=k, n_solved=int(nsolved.cpu()),
                node_cycle_ms=round(med["node_cycle"], 4), node_tick_ms=round(med["node_tick"], 4),
                stage_ms=round(med["stage"], 4), push_ms=round(med["push"], 4),
                cycle_minus_tick_ms=round(med["node_cycle"] - med["node_tick"], 4), **extra,
                rounds={k_: [round(x, 4) for x in v] for k_, v in ms.items()},
                invalid=int((buf["valid"] == 0).sum()), cycle_equals_tick=bool(same),
                dropped=int((cyc["M"].cpu() != t(mode).cpu()).sum()),
                failed=dict(cycle=int((cyc["st"] != 0).sum()), tick=int((tick["st"] != 0).sum())))), flush=True)


def dump_failed(a, B=1024, max_ticks=165):
    """cycle_bench's B = 1024, all-active handle with the seeded speed map, one node_cycle at a time (165 ticks at the
    most: what three rounds of 5 + 50 calls are). Before each cycle: the iterate and the carried refs of the fleet, and
    the limits the map's writer gives on them (the cycle's own writer runs on the same inputs; the table's bytes are
    compared after the cycle). After it: the references the gate made and the solve's outputs. At the first nonzero
    status the robot's history goes to a.dump_failed, float32, and one JSON line says what was found."""
    from nmpc_nav_control_amd._lib import NODE_FOLLOW_PATH, NODE_GOTO_POSE
    from nmpc_nav_control_amd.batch import BatchSolver, NodeInput, NodeParams, SpeedMap
    dev = torch.device("cuda:0")
    N = a.num_poses - 1
    npar = NodeParams.default()
    i32, f64, now, period = torch.int32, torch.float64, 1700000000000000000, 25000000
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    rng = np.random.default_rng(20250826)
    grid = rng.uniform(0.15, 1.0, (256, 256)).astype(np.float32)
    grid[rng.uniform(size=grid.shape) < 0.2] = np.inf
    smap = SpeedMap(-32.0, -32.0, 0.25, t(grid))
    segs, nseg, nu = seeded_paths(B)
    pose = seeded_poses(segs, nseg, nu).astype(np.float64)
    rng = np.random.default_rng(B)
    ang, r = rng.uniform(-math.pi, math.pi, B), rng.uniform(0.3, 1.0, B)
    goal = np.stack([pose[0] + r * np.cos(ang), pose[1] + r * np.sin(ang), pose[2] + rng.uniform(0.2, 1.0, B)])
    act = np.sort(rng.permutation(B))
    mode = np.zeros(B, np.uint8)
    mode[act[0::2]] = NODE_FOLLOW_PATH
    mode[act[1::2]] = NODE_GOTO_POSE
    s = BatchSolver("diff", N, B, device=dev)
    S, NS, M, G = t(segs), t(nseg), t(mode), t(goal)
    U = torch.zeros(B, dtype=f64, device=dev)
    stamp, smp = t(np.full(B, now - 2000000, np.int64)), t(pose)
    s.enable_input(4)
    s.push_samples(stamp - period, smp)
    s.push_samples(stamp, smp)
    s.set_speed_map(smap)
    nin = NodeInput.default(now_ns=now, pose=torch.zeros(3, B, device=dev), vel=torch.zeros(3, B, device=dev),
                            valid=torch.zeros(B, dtype=torch.uint8, device=dev))
    fresh = torch.ones(B, dtype=torch.uint8, device=dev)
    out = dict(cmd=torch.zeros(3, B, device=dev), u0=torch.zeros(2, B, device=dev),
               status=torch.zeros(B, dtype=i32, device=dev), qp_iter=torch.zeros(B, dtype=i32, device=dev),
               qp_res=torch.zeros(3, B, device=dev))
    traj = torch.zeros(N + 1, 3, B, device=dev)
    vlim = torch.zeros(N + 1, B, device=dev)
    s.node_input(nin, M, goal_map=G)  # (the stage's outputs for the first writer call below: the samples are fixed)
    torch.cuda.synchronize()
    hist, same_table = [], True
    host = lambda x: x.cpu().numpy().copy()  # noqa: E731
    for tick in range(max_ticks):
        xb, ub, cr = (v.to_tensor()[:, :B] for v in s.state())
        s.stage_limits_from_map(smap, pose=nin.pose, reset=fresh, vlim=vlim)
        torch.cuda.synchronize()
        rec = dict(xbar=host(xb), ubar=host(ub), carried=host(cr), vlim=host(vlim), reset=host(fresh), mode=host(M))
        table = s.stage_bounds().to_tensor()
        s.node_cycle(npar, nin, M, goal_map=G, segs=S, nseg=NS, path_u=U, reset=fresh, traj_out=traj, **out)
        torch.cuda.synchronize()
        # (the rows of a robot that left GOTO_POSE / FOLLOW_PATH in this cycle are not rewritten: none has, before a failure)
        same_table &= bool(torch.equal(table, s.stage_bounds().to_tensor()))
        rec.update(traj=host(traj), pose=host(nin.pose), vel=host(nin.vel), **{k: host(v) for k, v in out.items()})
        hist.append(rec)
        bad = np.flatnonzero(rec["status"] != 0)
        if len(bad):
            break
    else:
        print(json.dumps(dict(metric="first failed solve (diff N=%d, B=%d, seeded speed map)" % (N, B), failed=False,
                              ticks=max_ticks, table_equals_writer=same_table)), flush=True)
        return
    i = int(bad[0])
    col = lambda k: np.stack([h[k][..., i] for h in hist]).astype(np.float32)  # noqa: E731
    np.savez_compressed(
        a.dump_failed, robot=i, tick=tick, N=N, mode=np.array([h["mode"][i] for h in hist], np.uint8),
        reset=np.array([h["reset"][i] for h in hist], np.uint8), pose=col("pose"), vel=col("vel"),
        goal=goal[:, i].astype(np.float32), traj=col("traj"), vlim=col("vlim"), carried=col("carried"),
        xbar=col("xbar"), ubar=col("ubar"), u0=col("u0"), cmd=col("cmd"), qp_res=col("qp_res"),
        status=np.array([h["status"][i] for h in hist], np.int32),
        qp_iter=np.array([h["qp_iter"][i] for h in hist], np.int32))
    plan = s.plan_ex(B, "run")
    print(json.dumps(dict(metric="first failed solve (diff N=%d, B=%d, seeded speed map)" % (N, B), failed=True,
                          robot=i, tick=tick, status=int(hist[-1]["status"][i]), qp_iter=int(hist[-1]["qp_iter"][i]),
                          qp_res=[float(x) for x in hist[-1]["qp_res"][:, i]], mode=int(hist[-1]["mode"][i]),
                          failed_robots=[int(b) for b in bad], table_equals_writer=same_table,
                          kernel=plan["kernel"], segments=plan["segments"], out=a.dump_failed)), flush=True)


def mission_sets(segs, nseg):
    """(plain one-part paths, one-part sets, three-part sets) of a seeded fleet: every robot's first segment alone,
    and the same followed by its reversal (driven backwards) and itself again. Segment records [B][3][16]."""
    B = len(nseg)
    one = np.zeros((B, 3, SEG_DOUBLES))
    one[:, 0] = segs[:, 0]
    three = one.copy()
    back = segs[:, 0].copy()
    for o in (0, 4, 8):  # c(1 - u) of a cubic c(u), ascending coefficients
        c0, c1, c2, c3 = (segs[:, 0, o + k] for k in range(4))
        back[:, o], back[:, o + 1], back[:, o + 2], back[:, o + 3] = c0 + c1 + c2 + c3, -(c1 + 2 * c2 + 3 * c3), \
            c2 + 3 * c3, -c3
    back[:, 12] = -segs[:, 0, 12]
    three[:, 1], three[:, 2] = back, segs[:, 0]
    return one, three


def mission_bench(a):
    """the queue tick against the plain node tick (see the module docstring). Every handle runs warm-started ticks on
    fixed measurements with path_u fed back, as --node does; `dropped` counts robots that left FollowPath."""
    from nmpc_nav_control_amd._lib import NODE_FOLLOW_PATH
    from nmpc_nav_control_amd.batch import BatchSolver, NodeParams
    from nmpc_nav_control_amd.path import PathQueue
    dev = torch.device("cuda:0")
    N = a.num_poses - 1
    npar = NodeParams.default()
    stream = torch.cuda.current_stream()
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    for B in (4096, 1024):
        segs, nseg, nu = seeded_paths(B)
        nu = np.minimum(nu, 0.45)
        ones = np.ones(B, np.int32)
        pose = t(seeded_poses(segs, ones, nu))
        one, three = mission_sets(segs, nseg)
        vel = torch.zeros(3, B, device=dev)

        def handle():
            return dict(solver=BatchSolver("diff", N, B, device=dev), M=torch.full((B,), NODE_FOLLOW_PATH, dtype=torch.uint8, device=dev),
                        u0=torch.zeros(2, B, device=dev), st=torch.zeros(B, dtype=torch.int32, device=dev))

        plain, q1, q3 = handle(), handle(), handle()
        plain.update(S=t(one), NS=t(ones), U=torch.zeros(B, dtype=torch.float64, device=dev))
        for d, sets, n in ((q1, one, 1), (q3, three, 3)):
            d["Q"] = PathQueue(B, 3, device=dev)
            d["Q"].segs.copy_(t(sets))
            d["Q"].npart.fill_(n)

        def plain_step():
            d = plain
            d["solver"].node_tick(npar, d["M"], pose, vel, segs=d["S"], nseg=d["NS"], path_u=d["U"], u0=d["u0"],
                                  status=d["st"])

        def queue_step(d):
            d["solver"].node_tick_queue(npar, d["Q"], d["M"], pose, vel, u0=d["u0"], status=d["st"])

        steps = {"node_tick": plain_step, "queue_one_part": lambda: queue_step(q1),
                 "queue_three_part": lambda: queue_step(q3)}
        for fn in steps.values():  # warm-up: code objects, the handles' node buffers, the warm-started iterates
            timed(fn, 10, stream)
        ms = {k: [] for k in steps}
        for _ in range(5):
            for k, fn in steps.items():
                ms[k].append(timed(fn, a.iters, stream))
        med = {k: sorted(v)[2] for k, v in ms.items()}
        same = all(torch.equal(plain[k], q1[k]) for k in ("u0", "st", "M")) and torch.equal(plain["U"], q1["Q"].path_u)
        print(json.dumps(dict(
            metric="mission tick ms (diff N=%d)" % N, B=B, node_tick_ms=round(med["node_tick"], 4),
            queue_one_part_ms=round(med["queue_one_part"], 4), queue_three_part_ms=round(med["queue_three_part"], 4),
            queue_over_node=round(med["queue_one_part"] / med["node_tick"], 4),
            spread_ms={k: round(max(v) - min(v), 4) for k, v in ms.items()},
            windows={k: [round(x, 4) for x in v] for k, v in ms.items()},
            one_part_equals_node_tick=bool(same),
            dropped={k: int((d["M"] != NODE_FOLLOW_PATH).sum()) for k, d in (("node", plain), ("one", q1), ("three", q3))},
            failed={k: int((d["st"] != 0).sum()) for k, d in (("node", plain), ("one", q1), ("three", q3))},
            window_three=[int(q3["Q"].head.max()), int(q3["Q"].tail.max())])), flush=True)


if __name__ == "__main__":
    main()
