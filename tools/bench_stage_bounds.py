#!/usr/bin/env python3
"""What the stage table costs: bench.py's closed loop (fleet.Fleet, the stationary renewing fleet) with the table off
and with the table on holding the handle's own box at every stage, i.e. the same QPs, and the cost of one writer launch
and one shift launch. One JSON line per measurement.

usage: python tools/bench_stage_bounds.py [--model diff] [--batch 4096] [--N 40] [--steps 100] [--warmup 240]
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


def timed(model, B, N, steps, warmup, table, dev):
    f = Fleet(model, B, N, DEFAULT_SEED, dev)
    if table:
        f.solver.shift_stage_bounds(0)  # (the first writer fills every stage with the handle's own box)
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


def writer_launches(model, B, N, dev, reps=200):
    """one set_stage_limits launch (v_max at every stage, a mask on half of the robots) and one shift by a stage: mean
    over `reps` back-to-back launches each"""
    from nmpc_nav_control_amd.batch import BatchSolver
    s = BatchSolver(model, N, B, device=dev)
    v = torch.full((N + 1, B), 0.8, device=dev)
    mask = (torch.arange(B, device=dev) % 2 == 0).to(torch.uint8)
    s.set_stage_limits(v_max=v, mask=mask)  # (allocates and fills the table)
    out = []
    for what, call in (("set_stage_limits launch", lambda: s.set_stage_limits(v_max=v, mask=mask)),
                       ("shift_stage_bounds launch", lambda: s.shift_stage_bounds(1, B=B))):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(reps):
            call()
        b.record()
        torch.cuda.synchronize()
        out.append(dict(what=what, model=model, B=B, N=N, reps=reps,
                        us_per_launch=round(a.elapsed_time(b) / reps * 1e3, 2)))
    return out


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
    for r in writer_launches(args.model, 4096, args.N, dev):
        print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
