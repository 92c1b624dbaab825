"""What the GPU tests of the per-robot device tables share (test_gpu_robot_params.py, test_gpu_stage_bounds.py,
test_gpu_robot_model.py, test_gpu_run_edges.py, test_gpu_table_writers.py): device tensors of host arrays, the closed
loop on the harness plant, one tick's comparison with the per-robot oracles, and the launch forms.

Tolerance of the oracle comparisons: test_gpu_parity.py's, |u0 - u0_oracle|_inf and |cmd - cmd_oracle|_inf <= 1e-3 with
every status 0."""
import numpy as np
import torch

from nmpc_nav_control_amd._lib import default_params
from nmpc_nav_control_amd.batch import BatchSolver
from nmpc_nav_control_amd.scenario import make_fleet
from tests import far_field_cases as ff
from tests import robot_param_cases as rc

TOL_U = 1e-3
DEV = torch.device("cuda:0")
MODELS = ["diff", "omni4", "tric"]


def t(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device=DEV, dtype=dtype)


def table_args(P):
    """device tensors [n][B] of a parameter dict [B][n]"""
    return {k: t(P[k].T) for k in rc.FIELDS}


def state_of(s):
    """iterate, carried refs and warm flags"""
    return [v.to_tensor() for v in s.state()] + [s.warm_state()[0].to_tensor()]


class Loop:
    """test_run_closed_loop_matches_oracle's loop on the harness plant: device inputs and outputs of B robots of the
    seeded fleet, one run() per tick, the host copies of the tick's inputs for the oracles. offset: the fleet moved
    from the map origin (tests/far_field_cases.py:shift_fleet; [2], or [B][2] for one offset per robot)."""

    def __init__(self, solver, model, B, seed=rc.SEED, offset=(0.0, 0.0)):
        self.s, self.model, self.B = solver, model, B
        N = solver.N
        fl = self.fl = ff.shift_fleet(make_fleet(model, B, seed=seed), offset)
        solver.state()[2].copy_from(_pad(t(fl["carried"]), solver.capacity))
        self.pose, self.vel, self.steer = t(fl["pose"]), t(fl["vel"]), t(fl["steer"])
        self.path, self.prog = t(fl["path"]), t(fl["s"])
        self.steer_arg = self.steer if model == "tric" else None
        self.traj = torch.zeros(N + 1, 3, B, device=DEV)
        self.tlen = torch.zeros(B, dtype=torch.int32, device=DEV)
        self.out = dict(cmd=torch.zeros(3, B, device=DEV), u0=torch.zeros(solver.nu, B, device=DEV),
                        status=torch.zeros(B, dtype=torch.int32, device=DEV),
                        qp_iter=torch.zeros(B, dtype=torch.int32, device=DEV), qp_res=torch.zeros(3, B, device=DEV))
        solver.fleet_sim_step(self.path, self.prog, self.pose, self.vel, self.steer_arg, None, None, self.traj,
                              self.tlen, advance=False)

    def host_inputs(self):
        torch.cuda.synchronize()
        f64 = lambda a: np.ascontiguousarray(a, np.float64)  # noqa: E731
        return (f64(self.pose.cpu().numpy().T), f64(self.vel.cpu().numpy().T),
                f64(self.steer.cpu().numpy()) if self.model == "tric" else None,
                f64(self.traj.cpu().numpy().transpose(2, 0, 1)), np.ascontiguousarray(self.tlen.cpu().numpy(), np.int32))

    def run(self, reset=None):
        self.s.run(self.pose, self.vel, self.traj, steer=self.steer_arg, traj_len=self.tlen, reset=reset, **self.out)
        torch.cuda.synchronize()

    def advance(self):
        self.s.fleet_sim_step(self.path, self.prog, self.pose, self.vel, self.steer_arg, self.out["u0"],
                              self.out["status"], self.traj, self.tlen, advance=True)

    def carried(self):
        return self.s.state()[2].to_tensor()[:, :self.B]


def _pad(a, cap):
    out = torch.zeros(a.shape[0], cap, device=DEV)
    out[:, :a.shape[1]] = a
    return out


def check_tick(loop, fleet, inp, tick, tol=TOL_U, **kw):
    """one tick's u0 / cmd / status against the per-robot oracles on the same inputs (kw: further arguments of the
    oracles' tick); returns the two errors"""
    cmd_o, u0_o, st_o, it_o = fleet.tick(*inp, **kw)
    st = loop.out["status"].cpu().numpy()
    eu = np.abs(loop.out["u0"].cpu().numpy().T - u0_o).max()
    ec = np.abs(loop.out["cmd"].cpu().numpy().T - cmd_o).max()
    print(f"tick {tick}: oracle status {st_o.tolist()} iters <= {it_o.max()}; device status {st.tolist()} iters "
          f"{loop.out['qp_iter'].cpu().numpy().tolist()}; |du0| {eu:.2e} |dcmd| {ec:.2e}")
    assert (st_o == 0).all(), (tick, st_o)
    assert (st == 0).all(), (tick, st)
    assert eu <= tol, (tick, eu)
    assert ec <= tol, (tick, ec)
    return eu, ec


# The launch forms: (environment, qp_ipm, what nmpc_batch_plan_ex must report). NMPC_AMD_REC_SPLIT selects the team
# kernel's record planes, so that form switches the row-parallel kernel off as well (B = 15 would take it otherwise and
# the variable would select nothing).
TEAM = {"NMPC_AMD_ROWPAR_MAX": "0"}
PLAIN = dict(TEAM, NMPC_AMD_SPLIT_MAX="0")
FORMS = {
    "seg": ({}, 1, lambda p: p["kernel"] == "rowpar" and p["segments"] > 0),
    "serial": ({"NMPC_AMD_SEG": "0"}, 1, lambda p: p["kernel"] == "rowpar" and p["segments"] == 0),
    "team_split_launch": (TEAM, 1, lambda p: p["kernel"] == "team" and p["waves_per_robot"] == 0),
    "team_plain": (PLAIN, 1, lambda p: p["kernel"] == "team" and p["waves_per_robot"] == 0),
    "rec_split": (dict(PLAIN, NMPC_AMD_REC_SPLIT="1"), 1,
                  lambda p: p["kernel"] == "team" and p["record_layout"] == "split"),
    "mehrotra": ({}, 0, lambda p: p["kernel"] == "team" and p["warm_tag"] == 3),
}
CASES = [(m, f) for m in MODELS for f in FORMS if f != "rec_split" or m == "diff"]


def make_solver(monkeypatch, model, N, cap, form):
    env, ipm, _ = FORMS[form]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    prm = default_params(model, N)
    prm.qp_ipm = ipm
    return BatchSolver(model, N, cap, params=prm, device=DEV)
