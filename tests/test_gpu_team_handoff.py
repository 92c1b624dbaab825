"""The team kernel's in-block hand-off (k_sqp_rti_team_ho, csrc/sqp_rti_team_ho.hip): a robot
whose IPM has not stopped at the top of iteration C leaves the four-robots-per-wave loop, and one wave of its block
finishes it in the segmented one-wave form of the row-parallel tick.

tests/handoff_probe.py runs the fleets in child processes (NMPC_AMD_ROWPAR_MAX=0, NMPC_AMD_SPLIT_MAX=0: the unsplit
team form at these batch sizes). Bars:
 - a handed-over robot ends with the segmented kernel's arithmetic, so hand-off on against hand-off off is held per
   tick to what tests/test_gpu_seg.py holds the segmented kernel to against the serial one: equal status, IPM counts
   within 3; and u0 and the new iterate against the fp64 oracle's replay of the tick within 1e-3
   (tests/test_gpu_golden.py TOL_U / TOL_X, tests/test_gpu_seg.py TOL);
 - where nobody is handed over (C >= qp_iter_max), where a robot only changes its slot (placement), its neighbours
   (a failing robot, an active count that ends inside a block) or the barrier form of the one-wave kernel: bit for bit.
"""
import functools
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from handoff_probe import TICKS

from nmpc_nav_control_amd._lib import default_params
from nmpc_nav_control_amd.batch import BatchSolver

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL_U = TOL_X = 1e-3  # against the oracle's replay (test_gpu_golden.py, test_gpu_seg.py TOL)
ITER_BAND = 3         # IPM counts, hand-off on against off (test_gpu_seg.py; VERDICT r06's figure for a hand-off)
C_NEVER = 99          # >= qp_iter_max of every model: the hand-off kernel with nobody handed over
BATCHES = (16, 17, 37, 64)  # 17: a block with one team and three waves without any
OUT = ("status", "qp_iter", "u0", "cmd", "X", "U", "C")
_TMP = tempfile.TemporaryDirectory(prefix="handoff_")


CHK_W1BAR = os.path.join(ROOT, "nmpc_nav_control_amd", "lib", "chk_w1bar", "libnmpc_amd.so")
LOOPS = (("diff", 8), ("diff", 40), ("tric", 60))


@functools.lru_cache(maxsize=None)
def default_cap():
    """the measured default hand-off iteration: what set_handoff(-1), NMPC_HANDOFF_AUTO, asks for (the fleet driver's
    setting for the metric fleet; a new handle starts with the hand-off off)"""
    s = BatchSolver("diff", 40, 4096, params=default_params("diff", 40))
    assert s.plan_handoff(4096, "run")["iteration"] == 0
    s.set_handoff(-1)
    c = s.plan_handoff(4096, "run")["iteration"]
    s.close()
    return c


def caps():
    return sorted({0, 1, 3, default_cap(), C_NEVER})


def jobs():
    """name -> (handoff_probe.py arguments with {out} for the npz, environment): every child of this module"""
    bs, cs = ",".join(str(b) for b in BATCHES), ",".join(str(c) for c in caps())
    j = {f"loops_{m}_{N}": (["loops", m, str(N), "{out}", bs, cs], {}) for m, N in LOOPS}
    for s in ("off", "sorted"):
        j[f"sched_{s}"] = (["loops", "diff", "40", "{out}", "37,64", "3"], {"NMPC_AMD_SCHED": s})
    j["infeas"] = (["infeas", "{out}", "3"], {})
    j["node"] = (["node", "{out}", "1"], {})
    j["w1_product"] = (["w1", "{out}"], {})
    j["w1_chk"] = (["w1", "{out}"], {"NMPC_AMD_LIB": CHK_W1BAR})
    return j


_procs = {}


def probe(name):
    """The npz of child `name` as a dict. The first call starts every child of the module side by side (nine
    processes, each its own library load and environment); each call then waits for its own."""
    if not _procs:
        assert os.path.exists(CHK_W1BAR), f"{CHK_W1BAR} is built by the csrc Makefile (all)"
        for n, (args, env) in jobs().items():
            e = dict(os.environ)
            for k in ("NMPC_AMD_LIB", "NMPC_AMD_SCHED", "NMPC_AMD_HANDOFF"):
                e.pop(k, None)
            e.update(env, OMP_NUM_THREADS="2")
            out = os.path.join(_TMP.name, n + ".npz")
            p = subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "handoff_probe.py"),
                                  *[a.format(out=out) for a in args]], env=e, stdout=subprocess.PIPE,
                                 stderr=subprocess.PIPE, text=True)
            _procs[n] = [p, out, None]
    p, out, res = _procs[name]
    if res is None:
        try:
            _, err = p.communicate(timeout=300)
        finally:
            if p.poll() is None:
                p.kill()
        assert p.returncode == 0, (name, err[-3000:])
        res = _procs[name][2] = dict(np.load(out))
    return res


@pytest.fixture(scope="module", autouse=True)
def _reap():
    yield
    for p, _, _ in _procs.values():
        if p.poll() is None:
            p.kill()


def loops(model, N):
    return probe(f"loops_{model}_{N}")


def same_bits(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("model,N", LOOPS)
def test_handoff_closed_loops(built, model, N, B):
    """Closed loops of 6 ticks (every robot reset on tick 0) with C = 1 (every robot is handed over, 16 per block, four
    in turn on each wave), C = 3 and the default C against the loop with the hand-off off: per tick equal status, IPM
    counts within 3, u0 and the new iterate within 1e-3 of the oracle's replay. diff N = 8 has two stages per
    segment, the shortest the segment code takes."""
    d = loops(model, N)
    for C in caps():
        if C in (0, C_NEVER):
            continue
        worst = [0.0, 0.0, 0]
        for tick in range(TICKS):
            g = lambda k, c=C: d[f"B{B}_C{c}_t{tick}_{k}"]  # noqa: E731
            assert g("plan") == C and g("plan", 0) == 0, (C, tick, g("plan"))
            assert np.array_equal(g("status"), g("status", 0)), (C, tick, g("status"), g("status", 0))
            dit = int(np.abs(g("qp_iter").astype(int) - g("qp_iter", 0).astype(int)).max())
            worst = [max(worst[0], float(g("eu"))), max(worst[1], float(g("ex"))), max(worst[2], dit)]
        print(f"\n{model} N={N} B={B} C={C}: u0 err {worst[0]:.2e}, x err {worst[1]:.2e}, IPM count diff {worst[2]}; "
              f"off: u0 err {max(float(d[f'B{B}_C0_t{t}_eu']) for t in range(TICKS)):.2e}")
        assert worst[2] <= ITER_BAND, (C, worst)
        assert worst[0] <= TOL_U and worst[1] <= TOL_X, (C, worst)


@pytest.mark.parametrize("model,N", LOOPS)
def test_cap_at_iter_max_is_the_plain_launch(built, model, N):
    """C >= qp_iter_max: the hand-off kernel runs, phase 1 is the team tick unchanged and nobody is handed over, so
    every output and the resident state equal the plain launch's bit for bit, tick after tick."""
    d = loops(model, N)
    for B in BATCHES:
        for tick in range(TICKS):
            assert d[f"B{B}_C{C_NEVER}_t{tick}_plan"] == C_NEVER
            for k in OUT:
                assert same_bits(d[f"B{B}_C{C_NEVER}_t{tick}_{k}"], d[f"B{B}_C0_t{tick}_{k}"]), (B, tick, k)


def test_placement_invariance(built):
    """The same fleet with NMPC_AMD_SCHED off and sorted, hand-off on at C = 3: the sorted order moves robots to other
    slots, waves and blocks from the second tick on, and every robot's result is the same bit for bit. The rule looks
    at the robot's own count, and which wave finishes a robot changes no arithmetic."""
    a, b = probe("sched_off"), probe("sched_sorted")
    for B in (37, 64):
        for tick in range(TICKS):
            assert a[f"B{B}_C3_t{tick}_plan"] == 3
            for k in OUT:
                assert same_bits(a[f"B{B}_C3_t{tick}_{k}"], b[f"B{B}_C3_t{tick}_{k}"]), (B, tick, k)
        its = a[f"B{B}_C3_t{TICKS - 1}_qp_iter"]
        assert its.max() > its.min() and its.max() > 3  # (the sorted order is not the index order, and robots hand over)


def test_failing_robot_in_phase_two(built):
    """One infeasible robot (test_gpu_fleet.py::test_failure_stays_on_its_robot's construction) with C = 3, below its
    exit iteration: it fails in phase 2, on a wave that also finishes healthy robots, with the plain launch's status
    and a zero command, and keeps its iterate; every other robot equals the tick without it bit for bit."""
    C = 3
    d = probe("infeas")
    bad = int(d["bad"])
    assert d["plain_status"][bad] == 4 and d["plain_qp_iter"][bad] > C, (d["plain_status"][bad], d["plain_qp_iter"][bad])
    assert d["dirty_status"][bad] == d["plain_status"][bad]
    assert (d["dirty_cmd"][:, bad] == 0).all()
    assert same_bits(d["dirty_X"][:, bad], d["X0"][:, bad])
    good = np.ones(d["clean_status"].shape[0], bool)
    good[bad] = False
    assert (d["clean_status"] == 0).all() and (d["clean_qp_iter"] > C).any()
    for k in OUT:
        assert same_bits(d[f"dirty_{k}"][..., good], d[f"clean_{k}"][..., good]), k


def test_node_tick_active_count_inside_a_block(built):
    """A node tick of 37 robots of which 21 solve: the active count ends inside the second block and inside one of its
    waves, whose idle teams and the block's two empty waves still reach the barrier. C = 1: every solving robot is
    handed over. The 21 robots equal the same robots in a node tick of their own, bit for bit."""
    d = probe("node")
    act = d["act"]
    assert d["all_plan"] == 1 and d["alone_plan"] == 1
    assert int(d["all_n"][0]) == int(act.sum()) == 21 and int(d["alone_n"][0]) == 21
    assert (d["all_status"][act] == 0).all() and (d["all_qp_iter"][act] >= 1).all()
    for k in ("status", "qp_iter", "u0", "cmd", "X"):
        assert same_bits(np.ascontiguousarray(d[f"all_{k}"][..., act]), d[f"alone_{k}"]), k


def test_one_wave_kernel_keeps_its_results(built):
    """The one-wave row-parallel kernels take a wave-local fence where they took the block barrier. lib/chk_w1bar is
    the product with the barrier back (csrc/Makefile): diff N = 40, 300 robots under NMPC_AMD_ROWPAR_W=1
    NMPC_AMD_SEG=4, three ticks, every output and the resident state bit for bit."""
    a, b = probe("w1_product"), probe("w1_chk")
    assert set(a) == set(b) and len(a) == 3 * len(OUT)
    for k in a:
        assert same_bits(a[k], b[k]), k
    assert (a["t2_status"] == 0).all() and a["t2_qp_iter"].max() > a["t2_qp_iter"].min()


def test_plan(built):
    """nmpc_batch_plan_handoff: on for the metric launch (diff N = 40, 4096 robots; 16 blocks of LDS per 16 CUs), off
    for a dense launch (tric N = 60, 8192), omni4, a horizon that four segments do not divide, run_path, C = 0, a
    split or row-parallel launch, split records and a per-robot table (the forms the hand-off kernel leaves out fall
    back to the plain kernel)."""
    h = BatchSolver("diff", 40, 4096, params=default_params("diff", 40))
    # a new handle: off; the measured default on request; the metric fleet's driver asks for it (fleet.py)
    assert h.plan_handoff(4096, "run")["iteration"] == 0 and default_cap() in (10, 12, 14, 16)
    from nmpc_nav_control_amd.fleet import FleetNode
    node = FleetNode([("diff", 4096)], 40, 20250825, "cuda:0")
    assert node.fleets[0].solver.plan_handoff(4096, "run")["iteration"] == default_cap()
    del node
    ht = BatchSolver("tric", 60, 2048, params=default_params("tric", 60))
    assert ht.plan_handoff(2048, "run")["iteration"] == 0
    ht.set_handoff(12)
    assert ht.plan_handoff(2048, "run")["iteration"] == 12 and ht.plan_ex(2048, "run")["record_layout"] == "wide"
    ht.close()
    h.set_handoff(12)
    p = h.plan_handoff(4096, "run")
    assert p["iteration"] == 12 and p["segments"] == 4 and 80_000 < p["lds_bytes"] <= 163_840, p
    assert h.plan_handoff(4096, "solve")["iteration"] == 12
    assert h.plan_ex(4096, "run")["kernel"] == "team" and h.plan_ex(4096, "run")["record_layout"] == "wide"
    assert h.plan_handoff(4096, "run_path") == dict(iteration=0, segments=0, lds_bytes=0)
    assert h.plan_handoff(1024, "run")["iteration"] == 0  # the row-parallel kernel
    h.set_handoff(0)
    assert h.plan_handoff(4096, "run")["iteration"] == 0
    h.set_handoff(12)
    h.set_record_layout("split")
    assert h.plan_handoff(4096, "run")["iteration"] == 0 and h.plan_ex(4096, "run")["record_layout"] == "split"
    h.set_record_layout("wide")
    import torch
    h.set_robot_limits(v_max=torch.full((4096,), 0.8, device="cuda:0"))
    assert h.plan_handoff(4096, "run")["iteration"] == 0  # the per-robot table: the plain kernel's RP form
    h.clear_robot_params()
    assert h.plan_handoff(4096, "run")["iteration"] == 12
    for model, N, B in (("tric", 60, 8192), ("omni4", 40, 4096), ("diff", 42, 4096)):
        s = BatchSolver(model, N, B, params=default_params(model, N))
        s.set_handoff(12)
        assert s.plan_handoff(B, "run")["iteration"] == 0, (model, N, B)
        s.close()
    h.close()
