#!/usr/bin/env python3
"""What a per-robot device table costs: bench.py's closed loop (fleet.Fleet, the stationary renewing fleet) with the
table off and with the table on holding the handle's own values, i.e. the same QPs, and the cost of one launch of each
of the table's writers. One JSON line per measurement.

usage: python tools/bench_tables.py --table robot_params|stage_bounds|robot_model|frame|separation
                                    [--config metric|diff1024|omni4|tric] [--model diff] [--batch 4096] [--N 40]
                                    [--steps 100] [--warmup 240] [--repeats 3]
--config names a (model, batch, N) of bench.py (default metric: diff, 4096, 40); --model, --batch and --N replace its
members. Each repeat builds the table's fleets afresh and times them one after the other, so a group sees the same box
state; `rate` is robot ticks per second over the timed steps (solve + plant step, HIP events on the stream).
  robot_params  off, on (every field set to the handle's values);           writer: set_robot_limits
  stage_bounds  off, on (the first writer's fill: the handle's box at every stage);  writers: set_stage_limits, shift
  robot_model   off, uniform (the handle's p in every column), rule (the mixed fleet of tests/robot_model_cases.py,
                whose factors are imported from there; the harness plant steps each robot with its own column, so
                this closed loop is the mixed fleet's);                     writer: set_robot_model
  frame         the run-mode closed loop reads nothing of the frame table, so its variants are the launches that
                do: a follow_path tick and a queue node tick (every robot in FOLLOW_PATH) of robots standing beside
                seeded paths, with the table off and with it on (tests/frame_cases.py's four origins mixed robot by
                robot, the segments moved there in fp64, the same fp32 poses); `us_per_tick` is the mean over the
                timed ticks, launched back to back;   writers: set_robot_frame, recentre (a radius that moves every
                robot, then one that moves none), to_frame and from_frame of a pose and of a trajectory
  separation    fleet separation (nmpc_batch_export_tracks + nmpc_batch_stage_limits_from_tracks before every tick,
                the fleet's own export as the tracks, M = B): off, spread (every robot its own origin on a square grid
                of 10 m pitch: nobody is in range of anybody), dense (a pitch of 1.33 m: about 16 tracks within the
                3 m range of every robot). The three variants have the frame table on with the same origins as their
                `off`, so the tick is the same; `sep_us` is export + writer alone, timed back to back on the final
                state, and `cull` what the box test kept, counted by tests/separation_ref.py on 256 of the robots
                --guard: the writer's guard form (nmpc_batch_stage_limits_from_tracks_ex with seeded priorities
                0..3) and nmpc_batch_sep_hold behind it; `guard.held` counts the robots the hold took at the end
The writers are timed on 4096 robots with a mask on half of them: mean over 200 back-to-back launches."""
import argparse
import itertools
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nmpc_nav_control_amd.batch import BatchSolver, NodeParams  # noqa: E402
from nmpc_nav_control_amd.fleet import Fleet  # noqa: E402
from nmpc_nav_control_amd.scenario import DEFAULT_SEED, PARAMS  # noqa: E402
from nmpc_nav_control_amd.path import PathQueue  # noqa: E402
from nmpc_nav_control_amd.batch import SepGuard, Tracks  # noqa: E402
from tests import frame_cases  # noqa: E402  (the origins, stated once)
from tests import separation_ref  # noqa: E402
from tests.path_cases import random_paths  # noqa: E402
from tests.path_nearest_ref import near_err  # noqa: E402
from tests.robot_model_cases import P0, P1, P2  # noqa: E402  (the rule's factors, stated once)

CONFIGS = {"metric": ("diff", 4096, 40), "diff1024": ("diff", 1024, 40), "omni4": ("omni4", 4096, 40),
           "tric": ("tric", 8192, 60)}
WRITER_B = 4096


def own_values(solver, B, dev):
    """the handle's own bounds and weights as [n][B] device tensors (the fp32 values the kernels take)"""
    p = solver.params
    rows = dict(lbx=solver.nbx, ubx=solver.nbx, lbu=solver.nbu, ubu=solver.nbu, W=solver.ny, W_e=solver.nx)
    return {k: torch.tensor(list(getattr(p, k))[:n], dtype=torch.float32, device=dev)[:, None].repeat(1, B).contiguous()
            for k, n in rows.items()}


def model_table(solver, B, rule, dev):
    """float32 [np][B]: the handle's p in every column, or the mixed fleet's"""
    p = np.tile(np.array(PARAMS[solver.model][:solver.np], np.float64)[:, None], (1, B))
    if rule:
        i = np.arange(B)
        p[0] *= np.array(P0)[i % 3]
        p[1] *= np.array(P1)[i % 4]
        if solver.np > 2:
            p[2] *= np.array(P2)[(i // 2) % 3]
    return torch.from_numpy(p.astype(np.float32)).to(dev)


def half_mask(B, dev):
    return (torch.arange(B, device=dev) % 2 == 0).to(torch.uint8)


def rp_writers(s, B, dev):
    v, mask = torch.full((B,), 0.8, device=dev), half_mask(B, dev)
    return [("set_robot_limits launch", lambda: s.set_robot_limits(v_max=v, mask=mask), dict(model=s.model, B=B))]


def sb_writers(s, B, dev):
    v, mask = torch.full((s.N + 1, B), 0.8, device=dev), half_mask(B, dev)
    keys = dict(model=s.model, B=B, N=s.N)
    return [("set_stage_limits launch", lambda: s.set_stage_limits(v_max=v, mask=mask), keys),
            ("shift_stage_bounds launch", lambda: s.shift_stage_bounds(1, B=B), keys)]


def rm_writers(s, B, dev):
    p, mask = model_table(s, B, True, dev), half_mask(B, dev)
    return [("set_robot_model launch", lambda: s.set_robot_model(p, mask=mask),
             dict(model=s.model, B=B, N=s.N, table_bytes=4 * s.np * B))]


def fr_writers(s, B, dev):
    per = torch.from_numpy(frame_cases.per_robot(B).T.copy()).to(dev)
    mask, moved = half_mask(B, dev), torch.zeros(B, dtype=torch.uint8, device=dev)
    pose = per.clone()
    pose[0] += 0.25
    turns = itertools.cycle((per + 100.0, pose))  # every launch moves every masked robot: 100 m out, then back
    traj = torch.zeros(s.N + 1, 3, B, dtype=torch.float64, device=dev)
    traj[:, :2] = per[None]
    pose32, traj32 = torch.zeros(3, B, device=dev), torch.zeros(s.N + 1, 3, B, device=dev)
    pose3 = torch.cat([pose, torch.zeros(1, B, dtype=torch.float64, device=dev)]).contiguous()
    p64, t64 = torch.zeros_like(pose3), torch.zeros_like(traj)
    keys = dict(model=s.model, B=B, N=s.N, table_bytes=16 * B)
    return [("set_robot_frame launch", lambda: s.set_robot_frame(per, mask=mask), keys),
            ("recentre launch, every masked robot moves",
             lambda: s.recentre(next(turns), 2.0, mask=mask, moved=moved), keys),
            ("recentre launch, no robot moves", lambda: s.recentre(pose, 1e9, mask=mask, moved=moved), keys),
            ("to_frame launch, pose [3][B]", lambda: s.to_frame(pose3, out=pose32), keys),
            ("from_frame launch, pose [3][B]", lambda: s.from_frame(pose32, out=p64), keys),
            ("to_frame launch, traj [N+1][3][B]", lambda: s.to_frame(traj, out=traj32), keys),
            ("from_frame launch, traj [N+1][3][B]", lambda: s.from_frame(traj32, out=t64), keys)]


# per table: the closed loop's variants (label -> how the fleet's solver gets the table, None: off) and its writers
# (what, one launch, the line's own keys; the first one's first call allocates and fills the table)
TABLES = {
    "robot_params": (dict(off=None, on=lambda s, B, dev: s.set_robot_params(**own_values(s, B, dev))), rp_writers),
    "stage_bounds": (dict(off=None, on=lambda s, B, dev: s.shift_stage_bounds(0)), sb_writers),
    "robot_model": (dict(off=None, uniform=lambda s, B, dev: s.set_robot_model(model_table(s, B, False, dev)),
                         rule=lambda s, B, dev: s.set_robot_model(model_table(s, B, True, dev))), rm_writers),
    "frame": (dict(off=False, on=True), fr_writers),
    "separation": (dict(off=None, spread=None, dense=None), None),
}


def timed(model, B, N, steps, warmup, label, fill, dev):
    f = Fleet(model, B, N, DEFAULT_SEED, dev)
    if fill:
        fill(f.solver, B, dev)
    for _ in range(warmup):
        f.tick()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(steps):
        f.tick()
    b.record()
    torch.cuda.synchronize()
    ms = a.elapsed_time(b)
    fails = int((f.status != 0).sum().item())
    return dict(model=model, B=B, N=N, table=label, steps=steps, ms_per_step=round(ms / steps, 4),
                rate=round(B * steps / ms * 1e3, 1), failed_last_tick=fails, plan=f.solver.plan_ex(B, "run")["kernel"])


SEP_PITCH = dict(off=10.0, spread=10.0, dense=1.33)


def timed_separation(model, B, N, steps, warmup, label, dev, guard=False):
    """the closed loop with export + writer before every tick (label off: without them), every robot's origin on a grid.
    guard: the writer's guard form with seeded priorities, and the hold's launch behind it (the loop times the launches:
    held is counted, the plain ticks do not act on it)"""
    f = Fleet(model, B, N, DEFAULT_SEED, dev)
    s = f.solver
    side = int(np.ceil(np.sqrt(B)))
    i = np.arange(B)
    origin = SEP_PITCH[label] * np.stack([i % side, i // side]).astype(np.float64)
    s.set_robot_frame(torch.from_numpy(origin).to(dev))
    xy = torch.zeros(N + 1, 2, B, dtype=torch.float64, device=dev)
    tr = Tracks(xy, own_first=0)
    G = None
    if guard:
        pr = np.random.default_rng(DEFAULT_SEED).integers(0, 4, B).astype(np.int32)
        G = SepGuard(torch.from_numpy(pr).to(dev))

    def sep():
        s.export_tracks(xy, first=0, pose=f.pose, reset=f.reset)
        s.stage_limits_from_tracks(tr, pose=f.pose, reset=f.reset, guard=G)
        if G is not None:
            s.sep_hold(G, reset=f.reset, B=B)

    def tick():
        if label != "off":
            sep()
        f.tick()
    for _ in range(warmup):
        tick()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(steps):
        tick()
    b.record()
    torch.cuda.synchronize()
    ms = a.elapsed_time(b)
    r = dict(model=model, B=B, N=N, table=label, steps=steps, ms_per_step=round(ms / steps, 4),
             rate=round(B * steps / ms * 1e3, 1), failed_last_tick=int((f.status != 0).sum().item()))
    if label != "off":
        a.record()
        for _ in range(20):
            sep()
        b.record()
        torch.cuda.synchronize()
        r["sep_us"] = round(a.elapsed_time(b) / 20 * 1e3, 1)
        if G is not None:
            r["guard"] = dict(held=int(s.sep_state().to_tensor()[0, :B].sum().item()))
        T = xy.cpu().numpy()
        pick = np.arange(0, B, max(1, B // 256))[:256]
        c = separation_ref.cull_counts_map(T[:, :, pick], T, own=pick)
        r["cull"] = dict(box_tests=int(c["box_tests"]), kept_mean=round(float(c["kept"].mean()), 2),
                         kept_max=int(c["kept"].max()), pair_evals_mean=round(float(c["pair_evals"].mean()), 1))
    return r


def path_fleet(B, S=4, seed=DEFAULT_SEED):
    """robots beside the start of seeded forward paths (as tests/test_gpu_path_nearest.py:follow_case): segs [B][S][16],
    nseg [B], pose and vel [B][3] (fp32)"""
    rng = np.random.default_rng(seed)
    segs, nseg, nu = random_paths(B, seed=seed, max_segs=S, reverse_frac=0.0)
    pose = np.zeros((B, 3), np.float32)
    for i in range(B):
        en, _ = near_err(segs[i], int(nseg[i]), rng.uniform(0, 0.3), (0.0, 0.0, 0.0))
        pose[i] = (en[0] + rng.uniform(-0.1, 0.1), en[1] + rng.uniform(-0.1, 0.1), en[2] + rng.uniform(-0.2, 0.2))
    vel = np.zeros((B, 3), np.float32)
    vel[:, 0] = rng.uniform(0.0, 0.5, B)
    return segs, nseg, pose, vel


def timed_path_ticks(model, B, N, steps, warmup, label, on, dev):
    """the two launches that read the frame table, each timed over `steps` back-to-back ticks of a standing fleet"""
    segs, nseg, pose, vel = path_fleet(B)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    per = frame_cases.per_robot(B)
    S = segs.shape[1]
    z = lambda *sh, dt=torch.float32: torch.zeros(*sh, dtype=dt, device=dev)  # noqa: E731
    for what in ("follow_path", "node_tick_queue"):
        s = BatchSolver(model, N, B, device=dev)
        sg = d(frame_cases.move_segs(segs, per) if on else segs)
        if on:
            s.set_robot_frame(d(per.T.copy()))
            s.init_iterate()
        P, V, ns = d(pose.T), d(vel.T), d(nseg)
        out = dict(cmd=z(3, B), u0=z(s.nu, B), status=z(B, dt=torch.int32), qp_iter=z(B, dt=torch.int32))
        traj, err = z(N + 1, 3, B), z(2, B, dt=torch.float64)
        if what == "follow_path":
            u = z(B, dt=torch.float64)
            tick = lambda: s.follow_path(P, V, sg, ns, u, 1 / 40, err=err, traj_out=traj, **out)  # noqa: E731
        else:
            q = PathQueue(B, S, device=dev)
            q.segs.copy_(torch.nan_to_num(sg))
            q.npart.copy_(ns)
            mode, ev = torch.full((B,), 2, dtype=torch.uint8, device=dev), z(B, dt=torch.uint8)  # NODE_FOLLOW_PATH
            n, rs = z(1, dt=torch.int32), z(B, dt=torch.uint8)
            npar = NodeParams.default(max_pos_err=float("inf"), max_ori_err=float("inf"), final_pos_err=0.0)

            def tick():
                s.node_tick_queue(npar, q, mode, P, V, reset=rs, event=ev, err=err, traj_out=traj, n_solved=n, **out)
        for _ in range(warmup):
            tick()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(steps):
            tick()
        b.record()
        torch.cuda.synchronize()
        ms = a.elapsed_time(b)
        yield dict(model=model, B=B, N=N, table=label, what=what + " tick", steps=steps,
                   us_per_tick=round(ms / steps * 1e3, 2), rate=round(B * steps / ms * 1e3, 1),
                   failed_last_tick=int((out["status"] != 0).sum().item()))


def writer_launches(writers, model, N, dev, reps=200):
    s = BatchSolver(model, N, WRITER_B, device=dev)
    ws = writers(s, WRITER_B, dev)
    ws[0][1]()  # (allocates and fills the table)
    for what, call, keys in ws:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(reps):
            call()
        b.record()
        torch.cuda.synchronize()
        yield dict(what=what, **keys, reps=reps, us_per_launch=round(a.elapsed_time(b) / reps * 1e3, 2))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--table", required=True, choices=sorted(TABLES))
    ap.add_argument("--config", default="metric", choices=sorted(CONFIGS))
    ap.add_argument("--model")
    ap.add_argument("--batch", type=int)
    ap.add_argument("--N", type=int)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=240)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--guard", action="store_true", help="separation: the guard form of the writer and the hold's launch")
    args = ap.parse_args()
    model, B, N = (x if x is not None else c for x, c in zip((args.model, args.batch, args.N), CONFIGS[args.config]))
    variants, writers = TABLES[args.table]
    # (the model table's lines carry the config's name, as they always have)
    tag = dict(config=args.config) if args.table == "robot_model" else {}
    dev = torch.device("cuda:0")
    for rep in range(args.repeats):
        for label, fill in variants.items():
            if args.table == "frame":
                for r in timed_path_ticks(model, B, N, args.steps, args.warmup, label, fill, dev):
                    print(json.dumps(dict(r, repeat=rep)), flush=True)
                continue
            if args.table == "separation":
                print(json.dumps(dict(timed_separation(model, B, N, args.steps, args.warmup, label, dev,
                                                       guard=args.guard and label != "off"), repeat=rep)),
                      flush=True)
                continue
            r = timed(model, B, N, args.steps, args.warmup, label, fill, dev)
            print(json.dumps(dict(r, **tag, repeat=rep)), flush=True)
    for r in writer_launches(writers, model, N, dev) if writers else ():
        print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
