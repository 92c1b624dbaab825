"""The numpy model of the device tables' writers (tests/table_writer_ref.py) against its own invariants; no GPU. The
device tables are compared with the model in tests/test_gpu_table_writers.py."""
import numpy as np
import pytest

from tests import table_writer_ref as tw

N, B, CAP = 3, 9, 12
DIMS = {"diff": (2, 2, 7, 2), "omni4": (4, 4, 11, 4), "tric": (2, 2, 7, 2)}  # nbx, nbu, nx, nu
MASK = (np.arange(B) % 2 == 0).astype(np.uint8)


def rnd(rng, *shape):
    return rng.uniform(0.1, 2.0, shape).astype(np.float32)


def rp_fields(model):
    nbx, nbu, nx, nu = DIMS[model]
    return (("lbx", nbx), ("ubx", nbx), ("lbu", nbu), ("ubu", nbu), ("W", nx + nu), ("W_e", nx))


def tables(model, rng):
    nbx, nbu, _, _ = DIMS[model]
    fields = rp_fields(model)
    rp = tw.RowTable(fields, CAP, rnd(rng, sum(n for _, n in fields)))
    sb = tw.StageTable(N, nbx, nbu, CAP, rnd(rng, 2 * nbx + 2 * nbu))
    return rp, sb


def limits(rng, per_stage=False):
    """the five limit arrays: [B] each, or per stage [N + 1][B] (states) and [N][B] (inputs)"""
    st, inp = ((N + 1, B), (N, B)) if per_stage else ((B,), (B,))
    return dict(v_max=rnd(rng, *st), a_max=rnd(rng, *inp), alpha_min=rnd(rng, *st), alpha_max=rnd(rng, *st),
                dalpha_max=rnd(rng, *inp))


@pytest.mark.parametrize("model", sorted(DIMS))
def test_masked_out_columns_are_unchanged_by_every_writer(model):
    rng = np.random.default_rng(1)
    nbx, nbu, _, _ = DIMS[model]
    rp, sb = tables(model, rng)
    rp0, sb0 = rp.a.copy(), sb.a.copy()
    tric = model == "tric"
    rp.set(B, MASK, **{k: rnd(rng, n, B) for k, n in rp_fields(model)})
    rp.set_limits(B, tric, MASK, **limits(rng))
    sb.set(B, MASK, lbx=rnd(rng, N + 1, nbx, B), ubx=rnd(rng, N + 1, nbx, B), lbu=rnd(rng, N, nbu, B),
           ubu=rnd(rng, N, nbu, B))
    sb.set_limits(B, tric, MASK, **limits(rng, True))
    sb.shift(B, 1, MASK)
    out = np.r_[np.flatnonzero(MASK == 0), np.arange(B, CAP)]  # masked out, and past B
    assert np.array_equal(rp.a[:, out], rp0[:, out]) and np.array_equal(sb.a[:, out], sb0[:, out])
    on = np.flatnonzero(MASK)
    assert (rp.a[:, on] != rp0[:, on]).all()  # (and the writers did write: every row of the others)
    assert (sb.a[:N, on] != sb0[:N, on]).all() and (sb.a[N, on][:, :2 * nbx] != sb0[N, on][:, :2 * nbx]).all()
    assert np.array_equal(sb.a[N, :, 2 * nbx:], sb0[N, :, 2 * nbx:])  # stage N has no inputs: those rows hold the fill


@pytest.mark.parametrize("n", [N, N + 5])
def test_shift_by_the_horizon_or_more_copies_the_last_stage(n):
    rng = np.random.default_rng(2)
    nbx, nbu, _, _ = DIMS["omni4"]
    _, sb = tables("omni4", rng)
    sb.set(CAP, None, lbx=rnd(rng, N + 1, nbx, CAP), ubx=rnd(rng, N + 1, nbx, CAP), lbu=rnd(rng, N, nbu, CAP),
           ubu=rnd(rng, N, nbu, CAP))
    before = sb.a.copy()
    sb.shift(CAP, n)
    for k in range(N + 1):
        assert np.array_equal(sb.a[k, :, :2 * nbx], before[N, :, :2 * nbx])  # state rows: stage N
    for k in range(N):
        assert np.array_equal(sb.a[k, :, 2 * nbx:], before[N - 1, :, 2 * nbx:])  # input rows: stage N - 1
    assert np.array_equal(sb.a[N, :, 2 * nbx:], before[N, :, 2 * nbx:])


def test_shift_by_less_than_the_horizon():
    rng = np.random.default_rng(3)
    nbx, nbu, _, _ = DIMS["diff"]
    _, sb = tables("diff", rng)
    sb.set(CAP, None, lbx=rnd(rng, N + 1, nbx, CAP), lbu=rnd(rng, N, nbu, CAP))
    before = sb.a.copy()
    sb.shift(CAP, 0)
    assert np.array_equal(sb.a, before)
    sb.shift(CAP, 1)
    for k in range(N + 1):
        assert np.array_equal(sb.a[k, :, :2 * nbx], before[min(k + 1, N), :, :2 * nbx])
    for k in range(N):
        assert np.array_equal(sb.a[k, :, 2 * nbx:], before[min(k + 1, N - 1), :, 2 * nbx:])


def test_tric_limits_touch_slot_1_with_the_steering_arrays_only():
    rng = np.random.default_rng(4)
    rp, sb = tables("tric", rng)
    rp0, sb0 = rp.a.copy(), sb.a.copy()
    steer = {k: v for k, v in limits(rng).items() if k not in ("v_max", "a_max")}
    rp.set_limits(B, True, None, **steer)
    slot1 = [rp.off[f] + 1 for f in ("lbx", "ubx", "lbu", "ubu")]
    rest = np.setdiff1d(np.arange(rp.a.shape[0]), slot1)
    assert np.array_equal(rp.a[rest], rp0[rest])
    assert np.array_equal(rp.a[slot1, :B], np.stack([steer["alpha_min"], steer["alpha_max"], -steer["dalpha_max"],
                                                    steer["dalpha_max"]]))
    # the speed arrays alone: slot 0 alone
    rp.a[:] = rp0
    rp.set_limits(B, True, None, v_max=steer["alpha_max"], a_max=steer["dalpha_max"])
    assert np.array_equal(rp.a[slot1], rp0[slot1])
    slot0 = [r - 1 for r in slot1]
    assert (rp.a[slot0, :B] != rp0[slot0, :B]).all()
    # the same per stage
    st = {k: v for k, v in limits(rng, True).items() if k not in ("v_max", "a_max")}
    sb.set_limits(B, True, None, **st)
    assert np.array_equal(sb.a[:, :, [0, 2, 4, 6]], sb0[:, :, [0, 2, 4, 6]])
    assert np.array_equal(sb.a[:, :B, 1], st["alpha_min"]) and np.array_equal(sb.a[:, :B, 3], st["alpha_max"])
    assert np.array_equal(sb.a[:N, :B, 5], -st["dalpha_max"]) and np.array_equal(sb.a[:N, :B, 7], st["dalpha_max"])
    # and no other model reads the steering arrays
    rpd, sbd = tables("diff", rng)
    rpd0, sbd0 = rpd.a.copy(), sbd.a.copy()
    rpd.set_limits(B, False, None, **steer)
    sbd.set_limits(B, False, None, **st)
    assert np.array_equal(rpd.a, rpd0) and np.array_equal(sbd.a, sbd0)


def test_stage_fill_takes_the_per_robot_columns():
    rng = np.random.default_rng(5)
    nbx, nbu, _, _ = DIMS["omni4"]
    rp, _ = tables("omni4", rng)
    rp.set(B, MASK, ubx=rnd(rng, nbx, B))
    rows = 2 * nbx + 2 * nbu
    sb = tw.StageTable(N, nbx, nbu, CAP, rp.a[:rows])
    for k in range(N + 1):
        assert np.array_equal(sb.a[k], rp.a[:rows].T)
    assert np.array_equal(tw.decode_stage(sb.bytes(), N, CAP, rows), sb.a)
