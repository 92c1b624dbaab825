"""The far-field instrument (tests/far_field_cases.py) is valid: the shift is a shift, the fp64 oracle alone solves
every tick of the closed loop that tests/test_gpu_far_field.py runs at every offset (the cold tick 0 and the reset
tick included), the shifted edge table decides as the unshifted one, and the oracle is translation-covariant up to
what the fp32 quantisation of its inputs explains. CPU only.

The closed loop is tests/helpers.py:oracle_closed_loop at the GPU tests' shape (N = 20, 21 robots, 6 ticks, every
fifth robot reset before tick 3). The solver is given each tick's pose and references rounded to fp32, which is what a
device caller has; the iterate chain stays fp64."""
import functools

import numpy as np
import pytest

import far_field_cases as ff
import run_edge_cases as rc
from helpers import oracle_closed_loop
from nmpc_nav_control_amd.scenario import make_fleet
from oracle.oracle import Oracle
from tests import robot_param_cases as rp

MODELS = ["diff", "omni4", "tric"]
N, B, T, RESET_TICK = 20, 21, 6, 3
RESETS = {RESET_TICK: range(0, B, 5)}
PROBES = 3  # sign patterns of the one-ulp probe


def ulp32(a):
    return np.spacing(np.abs(np.asarray(a, np.float64)).astype(np.float32)).astype(np.float64)


def round_quant(tick, pose, traj):
    return rc.f32(pose), rc.f32(traj)


@functools.lru_cache(maxsize=None)
def loop(model, off, probe=None):
    """The closed loop at offset `off`. probe = (seed, at): at the origin, every x and y the solver is given moved by
    one fp32 ulp of a coordinate at offset `at`, with random signs: the oracle's response to the quantisation that
    offset brings."""
    fl = ff.shift_fleet(make_fleet(model, B, seed=rp.SEED), off)
    quant = round_quant
    if probe is not None:
        rng = np.random.default_rng(probe[0])
        step = ulp32(probe[1])

        def quant(tick, pose, traj):
            pose, traj = rc.f32(pose), rc.f32(traj)
            pose[:2] += step * rng.choice([-1.0, 1.0], 2)
            traj[:, :2] += step * rng.choice([-1.0, 1.0], traj[:, :2].shape)
            return pose, traj
    log = []
    oracle_closed_loop(model, N, B, T, fl=fl, quant=quant, reset_at=RESETS, log=log)
    return log


@pytest.mark.parametrize("off", ff.OFFSETS, ids=ff.off_id)
@pytest.mark.parametrize("model", MODELS)
def test_shifted_fleet_is_the_fleet_shifted(model, off):
    fl = make_fleet(model, B, seed=rp.SEED)
    sh = ff.shift_fleet(fl, off)
    assert set(sh) == set(fl)
    for k in fl:
        assert sh[k].dtype == fl[k].dtype and sh[k].shape == fl[k].shape, k
        if k not in ("pose", "path"):
            assert np.array_equal(sh[k], fl[k]), k
    for k in ("pose", "path"):
        assert np.array_equal(sh[k][2:], fl[k][2:]), k
        back = sh[k][:2].astype(np.float64) - np.asarray(off)[:, None]
        assert (np.abs(back - fl[k][:2].astype(np.float64)) <= 0.5 * ulp32(sh[k][:2])).all(), k
    if off == (0.0, 0.0):
        assert all(np.array_equal(sh[k], fl[k]) for k in fl)
    # one offset per robot: each robot is the robot of the fleet shifted by its own offset
    per = np.array([ff.OFFSETS[i % 4] for i in range(B)])
    mixed = ff.shift_fleet(fl, per)
    for j, o in enumerate(ff.OFFSETS):
        one = ff.shift_fleet(fl, o)
        for k in fl:
            assert np.array_equal(mixed[k][..., j::4], one[k][..., j::4]), (k, o)


@pytest.mark.parametrize("off", ff.OFFSETS, ids=ff.off_id)
@pytest.mark.parametrize("model", MODELS)
def test_shifted_table_is_the_table_shifted(model, off):
    """every pose and trajectory row (garbage included) moves by the offset to within half an ulp, nothing else moves,
    and the pre-solve decides alike on it: the same terminal weights (diff's hack) and the same unwrapped headings"""
    n = 21
    cs = rc.cases(model, n)
    sh = ff.shift_cases(cs, off)
    o = Oracle(model, n, rule="batched")
    assert [c.name for c in sh] == [c.name for c in cs]
    for c, d in zip(cs, sh):
        assert (d.hack, d.exact, d.marks) == (c.hack, c.exact, c.marks)
        for tk, sk in zip(c.ticks, d.ticks):
            assert set(sk) == set(tk)
            for k in ("vel", "steer", "traj_len", "reset"):
                assert np.array_equal(sk[k], tk[k]) if k == "vel" else sk[k] == tk[k], (c.name, k)
            for k in ("pose", "traj"):
                assert np.array_equal(sk[k], rc.f32(sk[k])), (c.name, k)
                assert np.array_equal(sk[k][..., 2], tk[k][..., 2]), (c.name, k)
                assert (np.abs(sk[k][..., :2] - off - tk[k][..., :2]) <= 0.5 * ulp32(sk[k][..., :2])).all(), (c.name, k)
            m = min(tk["traj_len"], n + 1)
            assert np.array_equal(sk["traj"][m:, :2], np.tile(rc.f32(np.array(rc.GARBAGE[:2]) + off), (n + 1 - m, 1)))
            args = (tk["vel"], 0.0 if tk["steer"] is None else tk["steer"])
            _, yref, We = o.prepare(tk["pose"], *args, tk["traj"][:m], np.zeros(o.nbx))
            _, yref_s, We_s = o.prepare(sk["pose"], *args, sk["traj"][:m], np.zeros(o.nbx))
            assert np.array_equal(We_s, We), (c.name, We_s, We)
            assert np.array_equal(yref_s[:, 2:], yref[:, 2:]), c.name
    if off == (0.0, 0.0):
        for c, d in zip(cs, sh):
            for tk, sk in zip(c.ticks, d.ticks):
                assert all(np.array_equal(sk[k], tk[k]) for k in ("pose", "traj"))


@pytest.mark.parametrize("off", ff.OFFSETS, ids=ff.off_id)
@pytest.mark.parametrize("model", MODELS)
def test_oracle_alone_solves_every_tick(model, off):
    """status 0 and fewer than 50 IPM iterations on every tick, the cold tick 0 and the reset tick on their own lines"""
    log = loop(model, off)
    assert len(log) == T
    cold, reset = log[0], log[RESET_TICK]
    assert (cold["status"] == 0).all() and cold["qp_iter"].max() < 50, (cold["status"], cold["qp_iter"])
    assert (reset["status"] == 0).all() and reset["qp_iter"].max() < 50, (reset["status"], reset["qp_iter"])
    for t, rec in enumerate(log):
        assert (rec["status"] == 0).all() and rec["qp_iter"].max() < 50, (t, rec["status"], rec["qp_iter"])
        assert np.isfinite(rec["u0"]).all(), t
    print(f"{model} {off}: qp_iter max {max(int(r['qp_iter'].max()) for r in log)}")


@pytest.mark.parametrize("off", ff.OFFSETS[1:], ids=ff.off_id)
@pytest.mark.parametrize("model", MODELS)
def test_oracle_is_translation_covariant(model, off):
    """|u0(offset) - u0(origin)| over the closed loop is no more than the input quantisation explains. The bound is the
    oracle's own response, at the origin, to moving every x and y it is given by one ulp of a coordinate at the
    offset (the largest over PROBES sign patterns, robots and ticks up to the one compared): rounding moves each input
    by half an ulp at most."""
    base, far = loop(model, (0.0, 0.0)), loop(model, off)
    probes = [loop(model, (0.0, 0.0), (seed, off)) for seed in range(PROBES)]
    bound = 0.0
    for t in range(T):
        bound = max([bound] + [float(np.abs(p[t]["u0"] - base[t]["u0"]).max()) for p in probes])
        dev = float(np.abs(far[t]["u0"] - base[t]["u0"]).max())
        print(f"{model} {off} tick {t}: |u0(off) - u0(0)| {dev:.2e}  one-ulp response {bound:.2e}")
        assert dev <= bound, (t, dev, bound)
    assert bound > 0.0  # (tric's cold u0 sits on its bounds for the whole fleet: tick 0 alone sees nothing)
