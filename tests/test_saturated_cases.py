"""The saturated case table (tests/saturated_cases.py) does what it claims, on the CPU: the fp64 reference solves every
kept case inside its iteration limit, the iterates are saturated, families B and C have the zero or one-ulp gaps they
name, the reference's solutions satisfy the KKT certificate of the independently condensed QP (tests/dense_qp.py),
and a library that ignored the table or read the neighbouring stage would be seen by tests/test_gpu_saturated.py."""
import numpy as np
import pytest

from oracle.oracle import Oracle
from tests import saturated_cases as sat
from tests import speed_map_ref as sm
from tests import stage_bound_cases as sc
from tests.dense_qp import condense, kkt_certificate, oracle_multipliers

F32 = np.float32
TOL = 1e-3      # test_gpu_saturated.py's tolerance on u0
FACTOR = 15.0   # a mistake must move the reference's u0 by FACTOR * TOL (test_run_edge_cases.py's bar for its table)
# family A, measured with the reference alone: (largest IPM iteration count, limited robots that end with more than N / 4
# stages within 1e-6 of the limit), of 640 solves and 16 robots; the test asserts at least half of the second
STATIC = {("diff", 20): (25, 11), ("omni4", 20): (15, 12), ("tric", 20): (14, 7), ("diff", 40): (18, 12),
          # the rotation remainders of the GPU test
          ("diff", 21): (25, 11), ("diff", 22): (24, 12)}
SOLVE = [("diff", 20), ("omni4", 20), ("tric", 20), ("diff", 40)]


def certificate(o, xbar, ubar, x0, yref, We, box):
    """the reference's step on one spliced QP against the KKT conditions of the condensed QP, at test_oracle.py's bars"""
    ix, iu = sc.idx(o)
    st, it, _, ub, sol = sc.solve_spliced(o, xbar, ubar, x0, yref, We, box, return_sol=True)
    assert st == 0 and it < sat.QP_ITER_MAX, (st, it)
    H, g, C, d, _, _ = condense(sc.spliced_qp(o, xbar, ubar, x0, yref, We, box), o.nbx, ix, o.nbu, iu)
    stat, prim, dual, comp = kkt_certificate(H, g, C, d, (ub - ubar).reshape(-1), oracle_multipliers(sol, o.N, o.nbu,
                                                                                                     o.nbx))
    assert stat <= 1e-9 * max(1.0, np.abs(g).max()), stat
    assert prim <= 1e-10 and dual <= 0.0 and comp <= 1e-8, (prim, dual, comp)
    return it


def test_zone_limits_are_the_speed_maps_rule_on_one_cell():
    """lim_k against speed_map_ref.limits on a one-cell map of ZONE, bit for bit"""
    for model in ("diff", "omni4", "tric"):
        N = 20
        o = Oracle(model, N, rule="batched")
        carried = sat.static_loop(model, N)["fleet"].carried
        ns = sc.speed_rows(model, o.nbx)
        m = sm.Map(-100.0, -100.0, 200.0, np.full((1, 1), sat.ZONE, F32))
        want = sm.limits(m, np.zeros((N + 1, 2, sat.B), F32), F32(o.prm.ubx[0]), F32(o.prm.ubu[0]), o.prm.dt,
                         carried.T.astype(F32), ns, slope=sat.SLOPE)
        got = sat.zone_limits(model, N, carried)
        assert got.dtype == F32 and np.array_equal(got, want.T), model


@pytest.mark.parametrize("model,N", list(STATIC))
def test_static_loop_reference(model, N):
    """family A: no robot left out, every solve status 0 below the iteration limit, and the limited robots end on it"""
    L = sat.static_loop(model, N)
    st, it = np.array(L["status"]), np.array(L["iters"])
    F = L["fleet"]
    cnt = sat.on_limit(model, F.xbar, L["P"][-1])
    held = sum(1 for i in range(sat.B) if sat.limited(i) and cnt[i] > N / 4)
    print(f"{model} N={N}: failed {int((st != 0).sum())} of {st.size}, qp_iter max {it.max()}, limited robots with "
          f"more than N/4 stages on the limit {held} of {sat.B}; stages on the limit {cnt.tolist()}")
    assert st.shape == (sat.T, sat.B) and (st == 0).all()
    assert it.max() < sat.QP_ITER_MAX and it.max() <= STATIC[(model, N)][0]
    assert 2 * held >= STATIC[(model, N)][1]
    # every table value is an fp32 value, the unlimited robots and rows hold the default box
    D = sc.default_profile(model, N, sat.B)
    for P in (L["P"][0], L["P"][-1]):
        for k in sc.FIELDS:
            assert np.array_equal(P[k], sat.f32(P[k]))
            assert np.array_equal(P[k][3::4], D[k][3::4]) and np.array_equal(P[k][:, 0], D[k][:, 0])
        assert np.array_equal(P["lbu"], D["lbu"]) and np.array_equal(P["ubu"], D["ubu"])
        assert (P["ubx"][0::4, 1:, 0] < D["ubx"][0::4, 1:, 0]).all()
    # the certificate on the last tick's QPs
    xb, ub, carried = L["pre"][-1]
    pose, vel, steer, traj, tlen = L["inp"]
    for i, o in enumerate(F.os):
        args = o.prepare(pose[i], vel[i], 0.0 if steer is None else steer[i], traj[i][:int(tlen[i])], carried[i])
        certificate(o, xb[i], ub[i], *args, {k: L["P"][-1][k][i] for k in sc.FIELDS})


@pytest.mark.parametrize("model,N", SOLVE)
def test_solve_cases_reference_and_gaps(model, N):
    """families B and C: the reference solves every kept robot below the iteration limit with a KKT certificate, at
    most MAX_DROPPED robots are removed per case, and the gaps are the ones the case names, in fp32 and in fp64"""
    o = Oracle(model, N, rule="batched")
    ix, iu = sc.idx(o)
    ns = sc.speed_rows(model, o.nbx)
    cases = sat.solve_cases(model, N)
    assert [c.name for c in cases] == [f"B-K{K}-{v}" for K in sat.ks(N) for v in sat.VARIANTS] + \
        [f"C-K{N // 2 - 3}-exact"]
    for c in cases:
        assert len(c.keep) >= sat.B - sat.MAX_DROPPED
        its = [certificate(o, c.xbar[i], c.ubar[i], c.x0[i], c.yref[i], c.We[i], c.box(i)) for i in range(len(c.keep))]
        for a in (c.xbar, c.ubar, c.x0, c.yref, c.We) + tuple(c.P.values()):
            assert np.array_equal(a, sat.f32(a))
        v = sat.speed_states(o, c.xbar)[:, 1:c.K + 1]            # [n][K][ns]
        lim = c.P["ubx"][:, 1:c.K + 1, :ns]
        assert np.array_equal(c.P["lbx"][:, 1:c.K + 1, :ns], -lim)
        top = v.max(axis=2)
        free = top < sat.FLOOR                                     # (the floor holds: no gap is named there)
        gap64 = (lim - v).min(axis=2)
        gap32 = (lim.astype(F32) - v.astype(F32)).min(axis=2)
        ulp = np.spacing(top.astype(F32)).astype(np.float64)
        want = {"exact": 0.0 * ulp, "above": ulp, "below": -np.spacing(np.nextafter(top.astype(F32), F32(0)))}
        assert np.array_equal(gap64[~free], want[c.variant][~free]), c.name
        assert np.array_equal(gap32[~free].astype(np.float64), gap64[~free]), c.name
        assert (~free).mean() > 0.9
        D = sc.default_profile(model, N, len(c.keep))
        assert np.array_equal(c.P["ubx"][:, c.K + 1:], D["ubx"][:, c.K + 1:])
        if c.family == "C":  # every input on a bound at every stage, and dx0 = START_GAP towards zero
            on = (c.P["ubu"] - c.ubar[:, :, iu] == 0) | (c.P["lbu"] - c.ubar[:, :, iu] == 0)
            assert on.all()
            assert np.abs(np.abs(c.xbar[:, 0, ix[:ns]] - c.x0[:, ix[:ns]]) - sat.START_GAP).max() < 1e-7
        print(f"{model} N={N} {c.name}: {len(c.keep)} robots, qp_iter max {max(its)}, pinned entries "
              f"{int((~free).sum())}")


def moved(o, args, box, base):
    st, _, _, ub = sc.solve_spliced(o, *args, box)
    return np.inf if st != 0 else float(np.abs(ub[0] - base[0]).max())


@pytest.mark.parametrize("model,N", SOLVE)
def test_a_mistake_in_the_table_is_visible(model, N):
    """per family: ignoring the table, or reading stage k + 1 in place of stage k, moves the reference's u0 on some robot
    by at least 15 x the 1e-3 tolerance (from the same state, the replay form of the GPU test)"""
    o = Oracle(model, N, rule="batched")
    L = sat.static_loop(model, N)
    pose, vel, steer, traj, tlen = L["inp"]
    worst = {}
    for mk in ("ignore", "next"):
        best = 0.0
        for tick in (1, sat.T // 2, sat.T - 1):
            xb, ub, carried = L["pre"][tick]
            Pm = sat.zone_profile(model, N, carried, mistake=mk)
            for i in range(sat.B):
                args = (xb[i], ub[i]) + o.prepare(pose[i], vel[i], 0.0 if steer is None else steer[i],
                                                  traj[i][:int(tlen[i])], carried[i])
                _, _, _, un = sc.solve_spliced(o, *args, {k: L["P"][tick][k][i] for k in sc.FIELDS})
                best = max(best, moved(o, args, {k: Pm[k][i] for k in sc.FIELDS}, un))
        worst[("A", mk)] = best
        for fam in ("B", "C"):
            best = 0.0
            for c in sat.solve_cases(model, N):
                if c.family != fam:
                    continue
                Pm = c.profile(mk)
                for i in range(len(c.keep)):
                    args = (c.xbar[i], c.ubar[i], c.x0[i], c.yref[i], c.We[i])
                    _, _, _, un = sc.solve_spliced(o, *args, c.box(i))
                    best = max(best, moved(o, args, c.box(i, Pm), un))
            worst[(fam, mk)] = best
    print(model, N, {f"{f}/{m}": round(v, 3) for (f, m), v in worst.items()})
    weak = {k: v for k, v in worst.items() if v < FACTOR * TOL}
    assert not weak, weak


def test_recorded_case_reference():
    """The recorded failure (robot 459 of the B = 1024 fleet under the seeded speed map, diff, N = 40, GOTO_POSE): the
    fp64 reference solves the failing tick's QP -- Oracle.prepare on the stored pose, velocity, references and carried
    refs, the stored iterate and the stored limits -- and the stored pattern is the recorded one. The robot has reached
    a fixed point of the static-plant loop: lim_1 = c (the map's cell limit is the carried speed itself), that speed
    reference state lies on the limit with a gap of exactly 0 on stages 1..17, and the inputs ride their bounds over
    the horizon: the second on +a_max on 33 stages, the first on -a_max on the 22 stages after the limit lets go (on
    stages 0..16, where its state is pinned to the limit, it is 0 to 1e-6). 78 of the QP's 240 bounds have
    ub - zbar = 0 or lb - zbar = 0 exactly."""
    d = sat.recorded()
    N, tk = d["N"], d["tick"]
    o = Oracle("diff", N, rule="batched")
    ix, iu = sc.idx(o)
    assert d["robot"] == 459 and tk == 32 and N == 40
    assert (d["status"][:tk] == 0).all() and d["status"][tk] == 1 and (d["mode"] == 1).all()  # (1: GOTO_POSE)
    assert d["reset"][0] == 1 and (d["reset"][1:] == 0).all()
    for k in ("pose", "vel", "traj"):
        assert (d[k] == d[k][0]).all(), k  # the plant stands still
    xbar, ubar, vlim = d["xbar"][tk], d["ubar"][tk], d["vlim"][tk]
    x0, yref, We = o.prepare(d["pose"][tk], d["vel"][tk], 0.0, d["traj"][tk][:1], d["carried"][tk])
    P = sat.limits_profile("diff", N, vlim[None])
    box = {k: P[k][0] for k in sc.FIELDS}
    st, it, _, ub = sc.solve_spliced(o, xbar, ubar, x0, yref, We, box)
    c = np.abs(d["carried"][tk]).max()
    gap = vlim[:, None] - sat.speed_states(o, xbar)                        # [N+1][2]
    on_u = np.abs(np.abs(ubar[:, iu]) - np.array(o.prm.ubu[:o.nbu])) == 0   # [N][2]
    zero = int((gap[1:] == 0).sum() + on_u.sum())
    print(f"recorded tick {tk}: reference status {st} in {it} iterations, |u0| {np.abs(ub[0]).max():.2e}; device status "
          f"{d['status'][tk]} at qp_iter {d['qp_iter'][tk]}, qp_res {d['qp_res'][tk].tolist()}; c {c!r} lim_1 "
          f"{vlim[1]!r}; state stages with gap 0: {np.flatnonzero((gap[1:] == 0).any(axis=1)) + 1}; inputs on a bound "
          f"at {on_u.sum(axis=0).tolist()} of {N} stages; bounds with gap exactly 0: {zero} of {4 * N + 2 * N}")
    assert st == 0 and it == 14
    assert vlim[1] == c
    assert (gap[1:18, 0] == 0).all() and (gap[1:] >= 0).all()
    assert on_u.sum(axis=0).tolist() == [22, 33] and (np.abs(ubar[:17, 0]) <= 1e-6).all()
    assert (d["qp_iter"][tk], np.isnan(d["qp_res"][tk][2])) == (21, True)
