#!/usr/bin/env python3
"""What a per-robot device table costs: bench.py's closed loop (fleet.Fleet, the stationary renewing fleet) with the
table off and with the table on holding the handle's own values, i.e. the same QPs, and the cost of one launch of each
of the table's writers. One JSON line per measurement.

usage: python tools/bench_tables.py --table robot_params|stage_bounds|robot_model
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
The writers are timed on 4096 robots with a mask on half of them: mean over 200 back-to-back launches."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nmpc_nav_control_amd.batch import BatchSolver  # noqa: E402
from nmpc_nav_control_amd.fleet import Fleet  # noqa: E402
from nmpc_nav_control_amd.scenario import DEFAULT_SEED, PARAMS  # noqa: E402
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


# per table: the closed loop's variants (label -> how the fleet's solver gets the table, None: off) and its writers
# (what, one launch, the line's own keys; the first one's first call allocates and fills the table)
TABLES = {
    "robot_params": (dict(off=None, on=lambda s, B, dev: s.set_robot_params(**own_values(s, B, dev))), rp_writers),
    "stage_bounds": (dict(off=None, on=lambda s, B, dev: s.shift_stage_bounds(0)), sb_writers),
    "robot_model": (dict(off=None, uniform=lambda s, B, dev: s.set_robot_model(model_table(s, B, False, dev)),
                         rule=lambda s, B, dev: s.set_robot_model(model_table(s, B, True, dev))), rm_writers),
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
    args = ap.parse_args()
    model, B, N = (x if x is not None else c for x, c in zip((args.model, args.batch, args.N), CONFIGS[args.config]))
    variants, writers = TABLES[args.table]
    # (the model table's lines carry the config's name, as they always have)
    tag = dict(config=args.config) if args.table == "robot_model" else {}
    dev = torch.device("cuda:0")
    for rep in range(args.repeats):
        for label, fill in variants.items():
            r = timed(model, B, N, args.steps, args.warmup, label, fill, dev)
            print(json.dumps(dict(r, **tag, repeat=rep)), flush=True)
    for r in writer_launches(writers, model, N, dev):
        print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
