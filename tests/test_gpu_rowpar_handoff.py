"""The row-parallel kernel's hand-offs between the waves of a block (k_sqp_rti_rowpar: P0b taking P0a's rounds, the
sensitivity rows taking the factorisation's stages, run mode's unwrap wave; each through an LDS counter one wave
spins on) and the forms they replaced, which the kernel keeps behind compile flags.

The csrc Makefile builds a checker library per form (lib/chk_noov, lib/chk_sensfused, lib/chk_dsep) and lib/chk_lag,
the product's arithmetic with one wave of every third robot held back (NMPC_LAG_WAVE, sqp_rti_rowpar.hip) so that
the waves behind a counter really have to wait. tests/rowpar_probe.py solves the same cases with each library, one
child process per library; every other comparison of the suite runs both sides with the waves in near lockstep.

 - every library: status 0, and the first tick's u0 within the parity bound of the fp64 oracle's sqp_rti;
 - chk_lag against the product: every output bit for bit. Both execute the same arithmetic and the kernel is
   deterministic (test_solve_iterate_equals_resident_solve asserts bit equality of two row-parallel launches), so any
   difference is an ordering dependence. With one count of wave-rounds for the three P0a waves (the kernel before
   the per-wave counts) this fails at every N >= 12 and holds at N = 11, one round;
 - chk_noov, chk_sensfused against the product: the same operations placed on other rows, the bound of that class
   (tests/test_gpu_split.py TOL);
 - chk_dsep against the product: phase D's sums over the stages in another order, the bound of that class
   (tests/test_gpu_seg.py TOL_SEG).
"""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import rowpar_probe
from rowpar_probe import TICKS, cases

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-3       # against the oracle (tests/test_gpu_parity.py)
TOL_SAME = 1e-5  # the same operations in another place (tests/test_gpu_split.py TOL), qp_iter within 1
TOL_SEG = 3e-4   # sums in another order (tests/test_gpu_seg.py TOL_SEG), qp_iter within 3
CHECKERS = ("chk_noov", "chk_sensfused", "chk_dsep", "chk_lag")
SOLVE_OUT = ("status", "qp_iter", "qp_res", "u0", "xtraj", "utraj")
RUN_OUT = ("status", "qp_iter", "qp_res", "u0", "cmd", "carried")
CLOSE_OUT = ("u0", "xtraj", "cmd", "carried")  # the outputs compared to a tolerance (the rest: bit comparisons only)


def lib_path(name):
    return os.path.join(ROOT, "nmpc_nav_control_amd", "lib", name, "libnmpc_amd.so")


def run_children(libs, tmp):
    """One rowpar_probe.py child per library of `libs` (name -> path, None: the product's), all on the same inputs;
    the children run side by side. Returns name -> npz."""
    inputs = os.path.join(tmp, "inputs.npz")
    rowpar_probe.make_inputs(inputs)
    procs = {}
    for name, lib in libs.items():
        env = dict(os.environ)
        env.pop("NMPC_AMD_LIB", None)
        if lib:
            assert os.path.exists(lib), f"{lib} is built by the csrc Makefile (all)"
            env["NMPC_AMD_LIB"] = lib
        procs[name] = subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "rowpar_probe.py"), inputs,
                                        os.path.join(tmp, f"{name}.npz")], env=env, stdout=subprocess.PIPE,
                                       stderr=subprocess.PIPE, text=True)
    outs = {}
    try:
        for name, p in procs.items():
            _, err = p.communicate(timeout=300)
            assert p.returncode == 0, (name, err[-3000:])
            outs[name] = dict(np.load(os.path.join(tmp, f"{name}.npz")))
    finally:
        for p in procs.values():
            if p.poll() is None:
                p.kill()
    return outs, dict(np.load(inputs))


def outputs(c):
    return RUN_OUT if c["mode"] == "run" else SOLVE_OUT


def bit_differences(a, b):
    """The (case, tick, output) whose arrays differ in any bit between the probe results a and b."""
    diff = []
    for c in cases():
        for tick in range(TICKS):
            for k in outputs(c):
                u, v = a[f"{c['name']}__t{tick}__{k}"], b[f"{c['name']}__t{tick}__{k}"]
                if u.shape != v.shape or u.tobytes() != v.tobytes():
                    diff.append((c["name"], tick, k))
    return diff


@pytest.fixture(scope="module")
def runs(built, tmp_path_factory):
    t0 = time.time()
    libs = {"product": None}
    libs.update({n: lib_path(n) for n in CHECKERS})
    outs, inputs = run_children(libs, str(tmp_path_factory.mktemp("rowpar_handoff")))
    print(f"rowpar hand-off probes: {len(libs)} children, {time.time() - t0:.1f} s")
    for n in CHECKERS:
        assert str(outs[n]["lib"]).endswith(f"{n}/libnmpc_amd.so")
    assert str(outs["product"]["lib"]) == ""
    return outs, inputs


@pytest.mark.parametrize("name", ("product",) + CHECKERS)
def test_every_library_solves(runs, name):
    outs, inputs = runs
    r = outs[name]
    for c in cases():
        # the launch is the one the case is about: the row-parallel kernel, four (two) waves, the segment count
        assert tuple(r[f"{c['name']}__plan"]) == (1, c["waves"], c["seg"]), (c["name"], r[f"{c['name']}__plan"])
        for tick in range(TICKS):
            st = r[f"{c['name']}__t{tick}__status"]
            assert (st == 0).all(), (c["name"], tick, st)
        if c["mode"] == "solve":
            err = float(np.abs(r[f"{c['name']}__t0__u0"].T - inputs[f"{c['name']}__u0_oracle"]).max())
            assert err <= TOL, (c["name"], err)


def test_lagging_wave_changes_no_bit(runs):
    outs, _ = runs
    diff = bit_differences(outs["product"], outs["chk_lag"])
    assert not diff, diff


def max_differences(a, b):
    worst = {"u": 0.0, "x": 0.0, "it": 0}
    for c in cases():
        for tick in range(TICKS):
            g = lambda r, k: r[f"{c['name']}__t{tick}__{k}"]  # noqa: E731
            for k in outputs(c):
                if k not in CLOSE_OUT:
                    continue
                d = float(np.abs(g(a, k) - g(b, k)).max())
                key = "u" if k in ("u0", "cmd") else "x"
                worst[key] = max(worst[key], d)
            worst["it"] = max(worst["it"], int(np.abs(g(a, "qp_iter") - g(b, "qp_iter")).max()))
    return worst


@pytest.mark.parametrize("name,tol,dit", [("chk_noov", TOL_SAME, 1), ("chk_sensfused", TOL_SAME, 1),
                                          ("chk_dsep", TOL_SEG, 3)])
def test_replaced_form_matches_product(runs, name, tol, dit):
    """Measured on the MI355X, maxima over every case and tick against the product: chk_noov and chk_sensfused
    exactly 0, no array differing in a bit (the bound stays the class's); chk_dsep u0 / cmd 3.6e-5, states 2.4e-6,
    qp_iter 1."""
    outs, _ = runs
    w = max_differences(outs["product"], outs[name])
    nbits = len(bit_differences(outs["product"], outs[name]))
    print(f"{name} vs product: inputs (u0, cmd) {w['u']:.3e} states (xtraj, carried) {w['x']:.3e} "
          f"qp_iter {w['it']} arrays differing in a bit {nbits}")
    for c in cases():
        for tick in range(TICKS):
            g = lambda r, k: r[f"{c['name']}__t{tick}__{k}"]  # noqa: E731
            for k in outputs(c):
                if k not in CLOSE_OUT:
                    continue
                d = float(np.abs(g(outs["product"], k) - g(outs[name], k)).max())
                assert d <= tol, (c["name"], tick, k, d)
            di = int(np.abs(g(outs["product"], "qp_iter") - g(outs[name], "qp_iter")).max())
            assert di <= dit, (c["name"], tick, di)
