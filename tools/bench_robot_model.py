#!/usr/bin/env python3
"""What the model table costs: bench.py's closed loop (fleet.Fleet, the stationary renewing fleet) with the table off,
with the table on holding the handle's own p in every column (the same QPs), and with the table on holding a mixed
fleet (the rule of tests/robot_model_cases.py, whose factors are imported from there), and the cost of one writer
launch. One JSON line per measurement.

usage: python tools/bench_robot_model.py [--config metric|diff1024|omni4|tric] [--steps 100] [--warmup 240]
                                         [--repeats 3]
Each repeat builds the three fleets afresh and times them one after the other (off, uniform, rule), so a triple sees
the same box state; `rate` is robot ticks per second over the timed steps (solve + plant step, HIP events on the
stream). The harness plant steps each robot with its own column, so the rule's closed loop is the mixed fleet's."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nmpc_nav_control_amd.fleet import Fleet  # noqa: E402
from nmpc_nav_control_amd.scenario import DEFAULT_SEED, PARAMS  # noqa: E402
from tests.robot_model_cases import P0, P1, P2  # noqa: E402  (the rule's factors, stated once)

CONFIGS = {"metric": ("diff", 4096, 40), "diff1024": ("diff", 1024, 40), "omni4": ("omni4", 4096, 40),
           "tric": ("tric", 8192, 60)}


def table_of(model, B, rule, n_p):
    """float32 [np][B]: the handle's p in every column, or the mixed fleet's"""
    p = np.tile(np.array(PARAMS[model][:n_p], np.float64)[:, None], (1, B))
    if rule:
        i = np.arange(B)
        p[0] *= np.array(P0)[i % 3]
        p[1] *= np.array(P1)[i % 4]
        if n_p > 2:
            p[2] *= np.array(P2)[(i // 2) % 3]
    return p.astype(np.float32)


def timed(model, B, N, steps, warmup, table, dev):
    f = Fleet(model, B, N, DEFAULT_SEED, dev)
    if table != "off":
        f.solver.set_robot_model(torch.from_numpy(table_of(model, B, table == "rule", f.solver.np)).to(dev))
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
    return dict(model=model, B=B, N=N, table=table, steps=steps, ms_per_step=round(ms / steps, 4),
                rate=round(B * steps / ms * 1e3, 1), failed_last_tick=fails, plan=f.solver.plan_ex(B, "run")["kernel"])


def writer_launch(model, B, N, dev, reps=200):
    """one set_robot_model launch with a mask on half of the robots: mean over `reps` back-to-back launches"""
    from nmpc_nav_control_amd.batch import BatchSolver
    s = BatchSolver(model, N, B, device=dev)
    p = torch.from_numpy(table_of(model, B, True, s.np)).to(dev)
    mask = (torch.arange(B, device=dev) % 2 == 0).to(torch.uint8)
    s.set_robot_model(p, mask=mask)  # (allocates and fills the table)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        s.set_robot_model(p, mask=mask)
    b.record()
    torch.cuda.synchronize()
    return dict(what="set_robot_model launch", model=model, B=B, N=N, reps=reps, table_bytes=4 * s.np * B,
                us_per_launch=round(a.elapsed_time(b) / reps * 1e3, 2))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--config", default="metric", choices=sorted(CONFIGS))
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=240)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    model, B, N = CONFIGS[args.config]
    dev = torch.device("cuda:0")
    for rep in range(args.repeats):
        for table in ("off", "uniform", "rule"):
            r = timed(model, B, N, args.steps, args.warmup, table, dev)
            print(json.dumps(dict(r, config=args.config, repeat=rep)), flush=True)
    print(json.dumps(writer_launch(model, 4096, N, dev)), flush=True)


if __name__ == "__main__":
    main()
