"""Child process of tests/test_gpu_team_handoff.py: the team kernel with and without its in-block hand-off on the
same fleets, written to an npz. One process per call, so that the environment (NMPC_AMD_ROWPAR_MAX=0 and
NMPC_AMD_SPLIT_MAX=0: the unsplit team form at these small batches; NMPC_AMD_SCHED; NMPC_AMD_LIB) is fixed before the
library loads.
usage: handoff_probe.py loops  model N out B[,B...] C[,C...]   closed loops, one per batch and cap
       handoff_probe.py infeas out C                              one infeasible robot among 64
       handoff_probe.py node   out C                              a node tick whose active count ends inside a block
       handoff_probe.py w1     out                                the one-wave segmented row-parallel kernel, 300 robots"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from nmpc_nav_control_amd._lib import default_params  # noqa: E402
from nmpc_nav_control_amd.batch import BatchSolver, NodeParams  # noqa: E402
from nmpc_nav_control_amd.fleet import Fleet  # noqa: E402
from oracle.oracle import Oracle  # noqa: E402

DEV = torch.device("cuda:0")
SEED = 20250824
TICKS = 6


def team_env():
    os.environ["NMPC_AMD_ROWPAR_MAX"] = "0"
    os.environ["NMPC_AMD_SPLIT_MAX"] = "0"
    os.environ.pop("NMPC_AMD_HANDOFF", None)


def fleet(model, N, B, C):
    f = Fleet(model, B, N, SEED + 1, DEV)
    f.solver.set_handoff(C)
    plan = f.solver.plan_ex(B, "run")
    assert plan["kernel"] == "team", plan
    return f


def outputs(f):
    xv, uv, cv = f.solver.state()
    B = f.B
    return dict(status=f.status.cpu().numpy().copy(), qp_iter=f.qp_iter.cpu().numpy().copy(),
                u0=f.u0.cpu().numpy().copy(), cmd=f.cmd.cpu().numpy().copy(), X=xv.to_tensor()[:, :B].cpu().numpy(),
                U=uv.to_tensor()[:, :B].cpu().numpy(), C=cv.to_tensor()[:, :B].cpu().numpy())


def loops(model, N, out, Bs, Cs):
    """For every batch size and cap: a closed loop of TICKS ticks from the same start, every robot reset on tick 0;
    per tick the outputs, the launch's hand-off iteration and the errors of u0 and of the new iterate against the fp64
    oracle's replay of that tick from the GPU's own pre-tick state."""
    o = Oracle(model, N, rule="batched")
    res = {}
    for B in Bs:
        for C in Cs:
            f = fleet(model, N, B, C)
            f.reset.fill_(1)
            for tick in range(TICKS):
                torch.cuda.synchronize()
                sn = f.snapshot()
                f.solve()
                torch.cuda.synchronize()
                xb, ub, cr = sn["xbar"].copy(), sn["ubar"].copy(), sn["carried"].copy()
                _, _, u0_o, st_o, _ = o.batch_tick(sn["pose"], sn["vel"], sn["steer"], sn["traj"], sn["tlen"], sn["reset"],
                                                  cr, xb, ub)
                d = outputs(f)
                ok = (d["status"] == 0) & (st_o == 0)
                after = f.snapshot()["xbar"]
                d["eu"] = np.float64(np.abs(d["u0"].T[ok] - u0_o[ok]).max() if ok.any() else 0.0)
                d["ex"] = np.float64(np.abs(after[ok] - xb[ok]).max() if ok.any() else 0.0)
                d["st_o"] = st_o
                d["plan"] = np.int32(f.solver.plan_handoff(B, "run")["iteration"])
                for k, v in d.items():
                    res[f"B{B}_C{C}_t{tick}_{k}"] = v
                f.advance()
            f.solver.close()
    np.savez(out, **res)


def infeas(out, C):
    """test_gpu_fleet.py::test_failure_stays_on_its_robot's infeasible robot (a carried speed reference of 50 m/s
    against the 1 m/s bound) among 64: the same tick clean and with it, hand-off on, and with it, hand-off off."""
    N, B, bad = 40, 64, 21
    f = fleet("diff", N, B, C)
    for _ in range(4):
        f.tick()
    torch.cuda.synchronize()
    st0 = dict(handle=f.solver.save_state(), pose=f.pose.clone(), vel=f.vel.clone(), traj=f.traj.clone(),
               tlen=f.tlen.clone(), C=f.solver.state()[2].to_tensor())

    def restore(inject):
        f.solver.restore_state(st0["handle"])
        for k in ("pose", "vel", "traj", "tlen"):
            getattr(f, k).copy_(st0[k])
        if inject:
            Cm = st0["C"].clone()
            Cm[0, bad] = 50.0
            f.solver.state()[2].copy_from(Cm)

    res = {"bad": np.int32(bad), "X0": f.solver.state()[0].to_tensor()[:, :B].cpu().numpy()}
    for name, inject, cap in (("clean", False, C), ("dirty", True, C), ("plain", True, 0)):
        restore(inject)
        f.solver.set_handoff(cap)
        f.solve()
        torch.cuda.synchronize()
        for k, v in outputs(f).items():
            res[f"{name}_{k}"] = v
    np.savez(out, **res)


def node(out, C):
    """A node tick of 37 robots of which 21 solve (the active count ends inside the second block, and inside a wave of
    it), against a node tick of those 21 robots alone."""
    N, B = 8, 37
    rng = np.random.default_rng(5)
    pose = np.zeros((B, 3), np.float32)
    pose[:, :2] = rng.uniform(-1, 1, (B, 2))
    pose[:, 2] = rng.uniform(-1, 1, B)
    goal = pose.copy()
    goal[:, :2] += rng.uniform(0.3, 0.9, (B, 2)).astype(np.float32)
    goal[:, 2] += rng.uniform(-0.5, 0.5, B).astype(np.float32)
    act = np.ones(B, bool)
    act[rng.choice(B, 16, replace=False)] = False
    res = {"act": act}
    for name, idx in (("all", np.arange(B)), ("alone", np.flatnonzero(act))):
        n = len(idx)
        s = BatchSolver("diff", N, n, params=default_params("diff", N))
        s.set_handoff(C)
        t = lambda a, dt=torch.float32: torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dt)  # noqa: E731
        mode = t(np.where(act[idx], 1, 0), torch.uint8)  # NMPC_NODE_GOTO_POSE / IDLE
        vel = torch.zeros(3, n, device=DEV)
        vel[0] = 0.1
        d = dict(cmd=torch.zeros(3, n, device=DEV), u0=torch.zeros(2, n, device=DEV),
                 status=torch.full((n,), -7, dtype=torch.int32, device=DEV),
                 qp_iter=torch.full((n,), -7, dtype=torch.int32, device=DEV))
        nsol = torch.zeros(1, dtype=torch.int32, device=DEV)
        s.node_tick(NodeParams.default(), mode, t(pose[idx].T), vel, goal=t(goal[idx].T), n_solved=nsol, **d)
        torch.cuda.synchronize()
        res[f"{name}_n"] = nsol.cpu().numpy()
        res[f"{name}_plan"] = np.int32(s.plan_handoff(n, "run")["iteration"])
        res[f"{name}_X"] = s.state()[0].to_tensor()[:, :n].cpu().numpy()
        for k, v in d.items():
            res[f"{name}_{k}"] = v.cpu().numpy()
        s.close()
    np.savez(out, **res)


def w1(out):
    """diff N = 40, 300 robots on the one-wave segmented row-parallel kernel, three closed-loop ticks."""
    os.environ["NMPC_AMD_ROWPAR_W"] = "1"
    os.environ["NMPC_AMD_SEG"] = "4"
    N, B = 40, 300
    f = Fleet("diff", B, N, SEED + 1, DEV)
    assert f.solver.plan(B) == ("rowpar", 1, 4), f.solver.plan(B)
    f.reset.fill_(1)
    res = {}
    for tick in range(3):
        f.solve()
        torch.cuda.synchronize()
        for k, v in outputs(f).items():
            res[f"t{tick}_{k}"] = v
        f.advance()
    np.savez(out, **res)


def main():
    what = sys.argv[1]
    if what == "w1":
        return w1(sys.argv[2])
    team_env()
    if what == "loops":
        ints = lambda s: [int(v) for v in s.split(",")]  # noqa: E731
        return loops(sys.argv[2], int(sys.argv[3]), sys.argv[4], ints(sys.argv[5]), ints(sys.argv[6]))
    if what == "infeas":
        return infeas(sys.argv[2], int(sys.argv[3]))
    if what == "node":
        return node(sys.argv[2], int(sys.argv[3]))
    raise SystemExit(f"unknown probe {what}")


if __name__ == "__main__":
    main()
