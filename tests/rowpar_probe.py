"""Solves of the row-parallel kernel's hand-off cases with one library, written to an npz (run as a child process of
tests/test_gpu_rowpar_handoff.py, so that each library -- the product's or the checker build named by NMPC_AMD_LIB --
is the only libnmpc_amd.so in its process). usage: rowpar_probe.py inputs.npz out.npz

The cases are the smallest shapes at which each hand-off between the waves of a block exists (k_sqp_rti_rowpar):
P0b on wave 0 taking P0a's rounds of 12 stages from waves 1-3 (four waves, segmented: 7, 4, 2 rounds and, as the
control, one), the sensitivity rows taking the factor columns stage by stage from the factorisation's wave (waves 2-3
behind waves 0-1 on four waves, wave 1 behind wave 0 on two), run mode's unwrap wave taking every round's poses.

Every case runs three ticks, the first cold and the next two warm. Immediately before each tick a second handle
solves another fleet of the same shape, so that the LDS a premature read would pick up holds another fleet's values:
after the same kernel on the same inputs it would hold exactly the expected ones and the read would go unnoticed."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(HERE), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

TICKS = 3
SEED, SEED_STALE = 20250824, 20250825  # (the compared fleet: helpers.oracle_closed_loop's default seed)


def cases():
    out = []
    for model in ("diff", "omni4", "tric"):
        # (N, B, segments of the default plan, creation-time overrides). N = 11 is prime, so its default plan is the
        # serial kernel, which has no P0 overlap at all; NMPC_AMD_SEG=1 runs the segmented kernel with one segment, the
        # overlap with one round
        # overlap with one round. (80, 1) is the reference node's own launch; its one robot is not one chk_lag holds
        # back (inst % 3 == 1), so (80, 2) runs the same plan with one that is
        for N, B, seg, env in ((80, 1, 8, {}), (80, 2, 8, {}), (40, 9, 5, {}), (12, 4, 3, {}),
                               (11, 4, 1, {"NMPC_AMD_SEG": "1"})):
            out.append(dict(name=f"solve_{model}_N{N}_B{B}", mode="solve", model=model, N=N, B=B, waves=4, seg=seg,
                            rounds=-(-(N + 1) // 12), env=env))
    out.append(dict(name="run_diff_N40_B9", mode="run", model="diff", N=40, B=9, waves=4, seg=5, rounds=4, env={}))
    # two waves per robot: no P0 overlap; the sensitivities on wave 1 behind wave 0's counter
    out.append(dict(name="solve_diff_N40_B257", mode="solve", model="diff", N=40, B=257, waves=2, seg=4, rounds=0,
                    env={"NMPC_AMD_ROWPAR_MAX": "1024"}))
    return out


def make_inputs(path):
    """The inputs of every case, once for all libraries: the compared fleet and the one solved before it, from
    helpers.oracle_closed_loop(model, N, B, 2), with the fp64 oracle's u0 of the compared fleet's first tick."""
    from helpers import oracle_closed_loop
    from oracle.oracle import path_discretize
    from path_cases import random_paths
    d = {}
    for c in cases():
        N, B = c["N"], c["B"]
        for tag, seed in (("", SEED), ("stale_", SEED_STALE)):
            k = f"{c['name']}__{tag}"
            if c["mode"] == "solve":
                o, rec = oracle_closed_loop(c["model"], N, B, 2, seed=seed)
                d[k + "x0"] = np.stack([r[0] for r in rec]).T
                d[k + "yref"] = np.stack([r[1] for r in rec]).transpose(1, 2, 0)
                d[k + "We"] = np.stack([r[2] for r in rec]).T
                d[k + "X"] = np.stack([r[3] for r in rec]).reshape(B, -1).T
                d[k + "U"] = np.stack([r[4] for r in rec]).reshape(B, -1).T
                if not tag:
                    d[k + "u0_oracle"] = np.stack([o.sqp_rti(r[3], r[4], r[0], r[1], r[2])[3][0] for r in rec])
            else:  # as tests/test_gpu_split.py::test_rowpar_run_matches_team
                rng = np.random.default_rng(seed)
                segs, nseg, nu = random_paths(B, seed=seed % 1000, max_segs=4, reverse_frac=0.2)
                nu[:] = rng.uniform(0, 0.3, B)
                traj, _ = path_discretize(segs, nseg, nu, 1 / 40, N + 1, False)
                pose = traj[:, 0, :].copy()
                pose[:, :2] += rng.uniform(-0.1, 0.1, (B, 2))
                vel = np.zeros((B, 3))
                vel[:, 0] = rng.uniform(0.0, 0.5, B)
                d[k + "pose"], d[k + "vel"] = pose.T, vel.T
                d[k + "traj"] = traj.transpose(1, 2, 0)
                i = np.arange(B)
                d[k + "traj_len"] = np.where(i % 3 == 0, 1, np.where(i % 3 == 1, N // 2, N + 1)).astype(np.int32)
    np.savez(path, **{k: np.ascontiguousarray(v) for k, v in d.items()})


def main():
    import torch

    from nmpc_nav_control_amd._lib import default_params
    from nmpc_nav_control_amd.batch import BatchSolver

    inp, out_path = np.load(sys.argv[1]), sys.argv[2]
    dev = torch.device("cuda:0")

    def t(a, dtype=torch.float32):
        return torch.from_numpy(np.ascontiguousarray(a)).to(device=dev, dtype=dtype)

    out = {"lib": os.environ.get("NMPC_AMD_LIB", "")}
    for c in cases():
        model, N, B, run = c["model"], c["N"], c["B"], c["mode"] == "run"
        os.environ.update(c["env"])
        hs = [BatchSolver(model, N, B, params=default_params(model, N)) for _ in range(2)]  # compared, stale
        for k in c["env"]:
            del os.environ[k]
        nx, nu = hs[0].nx, hs[0].nu
        p = hs[0].plan_ex(B, c["mode"])
        out[f"{c['name']}__plan"] = np.array([p["kernel"] == "rowpar", p["waves_per_robot"], p["segments"]], np.int32)
        ins = []
        for h, tag in zip(hs, ("", "stale_")):
            g = lambda f, dt=torch.float32: t(inp[f"{c['name']}__{tag}{f}"], dt)  # noqa: E731
            if run:
                ins.append(dict(pose=g("pose"), vel=g("vel"), traj=g("traj"), traj_len=g("traj_len", torch.int32)))
            else:
                xv, uv, _ = h.state()
                X, U = xv.to_tensor(), uv.to_tensor()
                X[:, :B], U[:, :B] = g("X"), g("U")
                xv.copy_from(X)
                uv.copy_from(U)
                ins.append(dict(x0=g("x0"), yref=g("yref"), We=g("We")))
        for tick in range(TICKS):
            res = []
            for h, a in zip(reversed(hs), reversed(ins)):  # the other fleet first, the compared one right behind it
                o = dict(u0=torch.zeros(nu, B, device=dev), status=torch.full((B,), -7, dtype=torch.int32, device=dev),
                         qp_iter=torch.zeros(B, dtype=torch.int32, device=dev), qp_res=torch.zeros(3, B, device=dev))
                if run:
                    o["cmd"] = torch.zeros(3, B, device=dev)
                    h.run(a["pose"], a["vel"], a["traj"], traj_len=a["traj_len"], **o)
                else:
                    o["xtraj"] = torch.zeros((N + 1) * nx, B, device=dev)
                    o["utraj"] = torch.zeros(N * nu, B, device=dev)
                    h.solve(a["x0"], a["yref"], We=a["We"], **o)
                res.append(o)
            torch.cuda.synchronize()
            o = res[1]
            if run:
                o["carried"] = hs[0].state()[2].to_tensor()[:, :B]
            for k, v in o.items():
                out[f"{c['name']}__t{tick}__{k}"] = v.cpu().numpy()
        for h in hs:
            h.close()
    np.savez(out_path, **out)


if __name__ == "__main__":
    main()
