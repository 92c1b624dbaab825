"""The edge-case table of run mode's pre-solve (tests/run_edge_cases.py) is a valid instrument: no case sits on an
fp32 decision boundary, the fp64 oracle alone stays inside its limits on every case, the numpy restatement of the
pre-solve (tests/prepare_ref.py) is the oracle's bit for bit, and every mistake it can switch on would be seen by
tests/test_gpu_run_edges.py. CPU only."""
import functools

import numpy as np
import pytest

import prepare_ref as pr
import run_edge_cases as rc
from oracle.oracle import Oracle

MODELS = ["diff", "omni4", "tric"]
GPU_NS = [1, 2, 20, 21, 22]  # the horizons of tests/test_gpu_run_edges.py
MARGIN = 1e-3                # distance of every fp32 decision from its boundary
TOL = 1e-3                   # test_gpu_run_edges.py's tolerance on u0 and on the state trajectory
FACTOR = 10.0                # a mistake must move the oracle's result by FACTOR * TOL: fp32 noise, up to 1 x TOL, cannot
                             # mask it. A condition, not a measurement


@functools.lru_cache(maxsize=None)
def chain(model, N):
    """The table through Oracle.batch_tick (rule="batched", the device API's), T ticks from the created iterate and
    zero carried refs. Per tick: the state before it (carried, xbar, ubar, the reset not yet applied), and status /
    qp_iter / u0 / the state after it."""
    o = Oracle(model, N, rule="batched")
    cs = rc.cases(model, N)
    B = len(cs)
    xbar, ubar = np.zeros((B, N + 1, o.nx)), np.zeros((B, N, o.nu))
    for i in range(B):
        xbar[i], ubar[i] = o.iterate_create()
    carried = np.zeros((B, o.nbx))
    ticks = []
    for t in range(rc.T):
        pose, vel, steer, traj, tlen, reset = rc.batch_inputs(cs, t)
        pre = (carried.copy(), xbar.copy(), ubar.copy())
        _, cmd, u0, st, it = o.batch_tick(pose, vel, steer if model == "tric" else None, traj, tlen, reset, carried,
                                          xbar, ubar)
        ticks.append(dict(pre=pre, status=st, qp_iter=it, u0=u0, xbar=xbar.copy()))
    return o, cs, ticks


def pre_state(ticks, t, i, reset):
    carried, xbar, ubar = (a[i].copy() for a in ticks[t]["pre"])
    if reset:
        xbar[:], ubar[:] = 0.0, 0.0
    return carried, xbar, ubar


@pytest.mark.parametrize("model", MODELS)
def test_prepare_ref_is_the_oracles_bit_for_bit(model):
    for N in GPU_NS:
        o, cs, ticks = chain(model, N)
        for i, c in enumerate(cs):
            for t, tk in enumerate(c.ticks):
                carried, _, _ = pre_state(ticks, t, i, tk["reset"])
                n = min(tk["traj_len"], N + 1)
                want = o.prepare(tk["pose"], tk["vel"], 0.0 if tk["steer"] is None else tk["steer"], tk["traj"][:n],
                                 carried)
                got = pr.prepare(model, o.prm, tk["pose"], tk["vel"], tk["steer"], tk["traj"], carried,
                                 traj_len=tk["traj_len"])
                for a, b, what in zip(got, want, ("x0", "yref", "We")):
                    np.testing.assert_array_equal(a, b, err_msg=f"{model} N={N} {c.name} tick {t} {what}")


@pytest.mark.parametrize("model", MODELS)
def test_table_values_are_fp32_and_garbage_is_where_it_should_be(model):
    for N in GPU_NS:
        cs = rc.cases(model, N)
        names = [c.name for c in cs]
        assert len(set(names)) == len(names)
        assert sum("len_N" in c.marks for c in cs) == 1 and sum("multi" in c.marks for c in cs) == 3
        lens = {c.ticks[0]["traj_len"] for c in cs}
        assert {n for n in (1, 2, 3, N // 2, N - 1, N, N + 1, N + 5) if n >= 1} <= lens and min(lens) >= 1
        for c in cs:
            assert len(c.ticks) == rc.T
            for tk in c.ticks:
                for k in ("pose", "vel", "traj"):
                    assert np.array_equal(tk[k], tk[k].astype(np.float32).astype(np.float64)), (c.name, k)
                assert tk["traj"].shape == (N + 1, 3)
                n = min(tk["traj_len"], N + 1)
                assert np.array_equal(tk["traj"][n:], np.tile(rc.f32(rc.GARBAGE), (N + 1 - n, 1))), c.name
                assert np.abs(tk["traj"][:n, :2]).max() < 5.0, c.name
        assert [sum(tk["reset"] for tk in c.ticks) for c in cs if c.name == "reset"] == [1]
        assert next(c for c in cs if c.name == "reset").ticks[rc.RESET_TICK]["reset"] == 1
        if model == "tric":
            assert {c.ticks[0]["steer"] for c in cs} >= {float(rc.f32(s)) for s in (0.3, 0.785, 1.2)} | {None}
        for pl in (rc.placements(cs), rc.placements(cs, 257)):
            marked = [i for i, c in enumerate(cs) if c.marks]
            assert len(pl) == len(marked)
            for o_, m in zip(pl, marked):
                B = len(o_)
                assert B % 4 and B % 16 and B <= 300 and set(o_) == set(range(len(cs)))
                assert o_[0] == m and o_[-1] == m
                for q in marked:
                    assert any(o_[s - 1] == q and o_[s] == q for s in range(16, B, 16)), (m, q)


@pytest.mark.parametrize("model", MODELS)
def test_margins(model):
    """The device decides in fp32: every unwrap decision is at least 1e-3 from +-pi (the two exact rows decide on
    fp32-exact numbers instead), and last two references that are meant to be distinct differ by at least 1e-3 in some
    component after the unwrap; those meant to be equal are equal."""
    for N in GPU_NS:
        o, cs, ticks = chain(model, N)
        for i, c in enumerate(cs):
            for t, tk in enumerate(c.ticks):
                d = pr.unwrap_deltas(tk["pose"], tk["traj"], tk["traj_len"])
                gap = np.abs(np.abs(d) - np.pi).min()
                if c.exact:
                    # delta 3.125 (keep) or 3.25 (unwrap): exact in fp32 and in fp64, 0.0166 and 0.108 from pi
                    assert d[0] in (3.125, 3.25) and np.float32(tk["traj"][0, 2]) - np.float32(tk["pose"][2]) == d[0]
                assert gap >= MARGIN, (model, N, c.name, t, gap)
                carried, _, _ = pre_state(ticks, t, i, tk["reset"])
                _, yref, We = pr.prepare(model, o.prm, tk["pose"], tk["vel"], tk["steer"], tk["traj"], carried,
                                         traj_len=tk["traj_len"])
                diff = np.abs(yref[N, :3] - yref[N - 1, :3]).max()
                assert c.hack in ("on", "off")
                if c.hack == "on":
                    assert diff == 0.0, (model, N, c.name, t)
                else:
                    assert diff >= MARGIN, (model, N, c.name, t, diff)
                if model == "diff":
                    assert We[0] == (100.0 if c.hack == "on" else 1.0) * o.prm.W[0], (N, c.name, t)
        # the hack's boundary rows are what they say (N >= 2: at N = 1 the list has two poses only)
        by = {c.name: c for c in cs}
        tr = by["hack_x"].ticks[0]["traj"]
        assert tr[N, 0] == tr[N - 1, 0] and abs(tr[N, 1] - tr[N - 1, 1]) >= MARGIN
        tr = by["hack_xy"].ticks[0]["traj"]
        assert (tr[N, :2] == tr[N - 1, :2]).all() and abs(tr[N, 2] - tr[N - 1, 2]) >= MARGIN
        tr = by["hack_xy_cut"].ticks[0]["traj"]
        assert (tr[N, :2] == tr[N - 1, :2]).all() and abs(tr[N, 2] - tr[N - 1, 2]) > 2 * np.pi - 0.1  # across the cut


@pytest.mark.parametrize("model", MODELS)
def test_reference_alone_stays_inside_the_limits(model):
    """status 0 and fewer than 50 IPM iterations on every tick of every case, for every horizon of the GPU matrix"""
    for N in GPU_NS:
        _, cs, ticks = chain(model, N)
        for t, rec in enumerate(ticks):
            bad = [(c.name, int(s), int(q)) for c, s, q in zip(cs, rec["status"], rec["qp_iter"]) if s != 0 or q >= 50]
            assert not bad, (model, N, t, bad)
        print(f"{model} N={N}: qp_iter max {max(int(r['qp_iter'].max()) for r in ticks)}")


def moved(o, x0, yref, We, xbar, ubar, base):
    st, _, xb, ub = o.sqp_rti(xbar, ubar, x0, yref, We)
    if st != 0 or not (np.isfinite(xb).all() and np.isfinite(ub).all()):
        return np.inf, np.inf  # (the GPU test asserts status 0 on both sides)
    return float(np.abs(ub[0] - base[1][0]).max()), float(np.abs(xb - base[0]).max())


def sensitivity(model, N):
    """{mistake: (case, |du0|, |dx|)}: the case that moves most, the oracle's u0 and new state trajectory from the
    mistaken pre-solve against the correct one, both from the same state before the tick (the replay form of the
    GPU test). The tick is the warm tick 3; carry_stale is taken at the reset tick 2 instead, the only tick where the
    resident iterate's stage 1 and the carried refs disagree (elsewhere x1's reference states are the carried values:
    both are x0 + u0 dt), and it is the state trajectory that shows it: its stage 0 is x0."""
    o, cs, ticks = chain(model, N)
    out = {}
    for mk in pr.MISTAKES:
        if not pr.applies(model, mk):
            continue
        t = rc.RESET_TICK if mk == "carry_stale" else rc.WARM_TICK
        best = ("-", 0.0, 0.0)
        for i, c in enumerate(cs):
            tk = c.ticks[t]
            carried, xbar, ubar = pre_state(ticks, t, i, tk["reset"])
            args = (model, o.prm, tk["pose"], tk["vel"], tk["steer"], tk["traj"], carried)
            st, _, xb, ub = o.sqp_rti(xbar, ubar, *pr.prepare(*args, traj_len=tk["traj_len"]))
            assert st == 0
            du, dx = moved(o, *pr.prepare(*args, mistake=mk, traj_len=tk["traj_len"], x1_prev=xbar[1]), xbar, ubar,
                           (xb, ub))
            if max(du, dx) > max(best[1], best[2]):
                best = (c.name, du, dx)
        out[mk] = best
    return out


def test_every_mistake_is_visible_at_ten_times_the_tolerance():
    """At N = 21, for every (model, mistake) whose step the model has (the hack's: diff only), some case moves the
    oracle's u0 or its new state trajectory by at least 10 x 1e-3.

    Measured: the weakest model's most sensitive case per mistake, max(|du0|, |dx|): pad_prev 3.2e-2 (tric; omni4
    0.11, diff 1.46), pad_raw 2.0, hack_xy 1.21, hack_never 1.42, hack_always 1.32 (diff), no_unwrap 2.0,
    unwrap_vs_pose 2.0 (u0 goes from one bound to the other on all three), unwrap_pad 0.93 (tric), kin_swap 0.26
    (diff, u0; tric's u0 sits on its bound either way, its x0 moves by 1.0), carry_stale 1.5e-2 (tric, the state
    trajectory alone: a reset tick is blind in tric's u0; omni4 7.1e-2, diff 0.26). The smallest is 15 x the
    tolerance."""
    rows = []
    for model in MODELS:
        s = sensitivity(model, 21)
        for mk, (name, du, dx) in s.items():
            rows.append((model, mk, name, du, dx))
            print(f"{model:6s} {mk:15s} {name:18s} |du0| {du:9.3e}  |dx| {dx:9.3e}  "
                  f"({max(du, dx) / TOL:.0f} x tol)")
    assert {(m, k) for m, k, *_ in rows} == {(m, k) for m in MODELS for k in pr.MISTAKES if pr.applies(m, k)}
    weak = [r for r in rows if max(r[3], r[4]) < FACTOR * TOL]
    assert not weak, weak
