#!/usr/bin/env python3
"""What the per-robot table of bounds and weights costs: bench.py's closed loop (fleet.Fleet, the stationary renewing
fleet) with the table off and with the table on holding the handle's own values, i.e. the same QPs, and the cost of
one nmpc_batch_set_robot_limits launch. One JSON line per measurement.

usage: python tools/bench_robot_params.py [--model diff] [--batch 4096] [--N 40] [--steps 100] [--warmup 240]
                                          [--repeats 3]
Each repeat builds both fleets afresh and times them one after the other (off, on), so the pairs see the same box
state; `rate` is robot ticks per second over the timed steps (solve + plant step, HIP events on the stream)."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nmpc_nav_control_amd.fleet import Fleet  # noqa: E402
from nmpc_nav_control_amd.scenario import DEFAULT_SEED  # noqa: E402


def own_values(solver, B, dev):
    """the handle's own parameters as [n][B] device tensors (the fp32 values the kernels take)"""
    p = solver.params
    rows = dict(lbx=solver.nbx, ubx=solver.nbx, lbu=solver.nbu, ubu=solver.nbu, W=solver.ny, W_e=solver.nx)
    return {k: torch.tensor(list(getattr(p, k))[:n], dtype=torch.float32, device=dev)[:, None].repeat(1, B).contiguous()
            for k, n in rows.items()}


def timed(model, B, N, steps, warmup, table, dev):
    f = Fleet(model, B, N, DEFAULT_SEED, dev)
    if table:
        f.solver.set_robot_params(**own_values(f.solver, B, dev))
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
    return dict(model=model, B=B, N=N, table="on" if table else "off", steps=steps, ms_per_step=round(ms / steps, 4),
                rate=round(B * steps / ms * 1e3, 1), failed_last_tick=fails, plan=f.solver.plan_ex(B, "run")["kernel"])


def limits_launch(model, B, N, dev, reps=200):
    """one set_robot_limits launch with a mask on half of the robots: mean over `reps` back-to-back launches"""
    from nmpc_nav_control_amd.batch import BatchSolver
    s = BatchSolver(model, N, B, device=dev)
    v = torch.full((B,), 0.8, device=dev)
    mask = (torch.arange(B, device=dev) % 2 == 0).to(torch.uint8)
    s.set_robot_limits(v_max=v, mask=mask)  # (allocates and fills the table)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        s.set_robot_limits(v_max=v, mask=mask)
    b.record()
    torch.cuda.synchronize()
    return dict(what="set_robot_limits launch", model=model, B=B, reps=reps,
                us_per_launch=round(a.elapsed_time(b) / reps * 1e3, 2))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--model", default="diff")
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--N", type=int, default=40)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=240)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    for rep in range(args.repeats):
        for table in (False, True):
            r = timed(args.model, args.batch, args.N, args.steps, args.warmup, table, dev)
            print(json.dumps(dict(r, repeat=rep)), flush=True)
    print(json.dumps(limits_launch(args.model, 4096, args.N, dev)), flush=True)


if __name__ == "__main__":
    main()
