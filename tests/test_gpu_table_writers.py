"""The writers of the three per-robot device tables (csrc/robot_tables.hip) against the numpy model of their content
(tests/table_writer_ref.py): after every call the whole table, read through the solver's view, equals the model's bit
for bit. The writers copy and negate float32 values, so nothing here has a tolerance. The columns past B and the
masked-out ones are part of the comparison: they hold the fill, the handle's own float32 values.

Shapes: N = 3 (state rows have 4 stages, input rows 3); (B, capacity) = (9, 12) with every other robot masked, so that
B, the capacity and the block of 256 are three numbers, and (300, 321), where x crosses the block edge with a ragged
tail. Every source array is random, so a value stored to another row, stage or robot shows."""
import numpy as np
import pytest
import torch

from nmpc_nav_control_amd.batch import BatchSolver
from tests import robot_model_cases as mc
from tests import robot_param_cases as rc
from tests import table_writer_ref as tw
from tests.table_harness import DEV, MODELS, t

pytestmark = pytest.mark.gpu
N = 3
SHAPES = [(9, 12), (300, 321)]
CASES = [(m, B, cap) for m in MODELS for B, cap in SHAPES]


def rnd(rng, *shape):
    return rng.uniform(0.1, 2.0, shape).astype(np.float32)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def dev(src):
    """device tensors of a dict of float32 arrays"""
    return {k: t(v) for k, v in src.items()}


class Case:
    """a solver of `cap` robots, the mask of every other one of the first B, and the fills its tables get"""

    def __init__(self, model, B, cap, seed):
        self.model, self.B, self.cap, self.tric = model, B, cap, model == "tric"
        self.s = s = BatchSolver(model, N, cap, device=DEV)
        self.rng = np.random.default_rng(seed)
        self.mask = (np.arange(B) % 2 == 0).astype(np.uint8)
        self.dmask = torch.from_numpy(self.mask).to(DEV)
        self.fields = (("lbx", s.nbx), ("ubx", s.nbx), ("lbu", s.nbu), ("ubu", s.nbu), ("W", s.ny), ("W_e", s.nx))
        hp = rc.handle_params(model, N, 1)
        self.column = np.concatenate([hp[k][0] for k in rc.FIELDS]).astype(np.float32)
        self.p = mc.handle_model(model, N, 1)[0].astype(np.float32)
        self.rows = 2 * s.nbx + 2 * s.nbu

    def rp_ref(self):
        return tw.RowTable(self.fields, self.cap, self.column)

    def sb_ref(self, rp=None):
        """the stage table as its first writer fills it: from the per-robot table rp when that is on"""
        box = self.column if rp is None else rp.a
        return tw.StageTable(N, self.s.nbx, self.s.nbu, self.cap, box[:self.rows])

    def limits(self, per_stage=False):
        st, inp = ((N + 1, self.B), (N, self.B)) if per_stage else ((self.B,), (self.B,))
        r = self.rng
        return dict(v_max=rnd(r, *st), a_max=rnd(r, *inp), alpha_min=rnd(r, *st), alpha_max=rnd(r, *st),
                    dalpha_max=rnd(r, *inp))

    def stage_src(self, names):
        n = dict(lbx=(N + 1, self.s.nbx), ubx=(N + 1, self.s.nbx), lbu=(N, self.s.nbu), ubu=(N, self.s.nbu))
        return {k: rnd(self.rng, *n[k], self.B) for k in names}

    def same_rows(self, view, ref, what):
        torch.cuda.synchronize()
        got = view().to_tensor().cpu().numpy()
        assert got.shape == ref.a.shape, what
        assert np.array_equal(bits(got), bits(ref.a)), what

    def same_stage(self, ref, what):
        torch.cuda.synchronize()
        raw = self.s.stage_bounds().to_tensor().cpu().numpy()
        assert raw.shape == ref.bytes().shape and np.array_equal(raw, ref.bytes()), what
        assert np.array_equal(bits(tw.decode_stage(raw, N, self.cap, self.rows)), bits(ref.a)), what


@pytest.mark.parametrize("model,B,cap", CASES)
def test_robot_params_writers(built, model, B, cap):
    c = Case(model, B, cap, 11)
    s, ref = c.s, c.rp_ref()
    assert s.robot_params() is None
    # the first writer fills: every column but the masked robots' limit rows is the handle's
    lim = c.limits()
    s.set_robot_limits(**dev(lim), mask=c.dmask)
    ref.set_limits(B, c.tric, c.mask, **lim)
    c.same_rows(s.robot_params, ref, "limits, masked")
    # some fields, masked; then every field, all robots
    part = {k: rnd(c.rng, n, B) for k, n in c.fields if k in ("ubx", "W")}
    s.set_robot_params(**dev(part), mask=c.dmask)
    ref.set(B, c.mask, **part)
    c.same_rows(s.robot_params, ref, "two fields, masked")
    full = {k: rnd(c.rng, n, B) for k, n in c.fields}
    s.set_robot_params(**dev(full))
    ref.set(B, None, **full)
    c.same_rows(s.robot_params, ref, "every field")
    lim = c.limits()
    s.set_robot_limits(**dev(lim))
    ref.set_limits(B, c.tric, None, **lim)
    c.same_rows(s.robot_params, ref, "limits")
    # clear, then a writer: the table is filled again before it is written
    s.clear_robot_params()
    assert s.robot_params() is None
    ref = c.rp_ref()
    part = {"lbu": rnd(c.rng, s.nbu, B)}
    s.set_robot_params(**dev(part), mask=c.dmask)
    ref.set(B, c.mask, **part)
    c.same_rows(s.robot_params, ref, "refill")


@pytest.mark.parametrize("model,B,cap", CASES)
def test_robot_model_writer(built, model, B, cap):
    c = Case(model, B, cap, 12)
    s = c.s

    def fresh():
        return tw.RowTable((("p", s.np),), cap, c.p)

    ref = fresh()
    assert s.robot_model() is None
    for mask, dmask, what in ((c.mask, c.dmask, "masked"), (None, None, "all")):
        p = rnd(c.rng, s.np, B)
        s.set_robot_model(t(p), mask=dmask)
        ref.set(B, mask, p=p)
        c.same_rows(s.robot_model, ref, what)
    s.clear_robot_model()
    assert s.robot_model() is None
    ref, p = fresh(), rnd(c.rng, s.np, B)
    s.set_robot_model(t(p), mask=c.dmask)
    ref.set(B, c.mask, p=p)
    c.same_rows(s.robot_model, ref, "refill")


@pytest.mark.parametrize("model,B,cap", CASES)
def test_stage_bounds_writers(built, model, B, cap):
    c = Case(model, B, cap, 13)
    s, ref = c.s, c.sb_ref()
    assert s.stage_bounds() is None
    # the first writer fills every stage with the handle's box (the per-robot table is off)
    lim = c.limits(per_stage=True)
    s.set_stage_limits(**dev(lim), mask=c.dmask)
    ref.set_limits(B, c.tric, c.mask, **lim)
    c.same_stage(ref, "limits, masked")
    part = c.stage_src(("lbx", "ubu"))
    s.set_stage_bounds(**dev(part), mask=c.dmask)
    ref.set(B, c.mask, **part)
    c.same_stage(ref, "two fields, masked")
    full = c.stage_src(("lbx", "ubx", "lbu", "ubu"))
    s.set_stage_bounds(**dev(full))
    ref.set(B, None, **full)
    c.same_stage(ref, "every field")
    for n, mask, dmask in ((0, None, None), (1, c.mask, c.dmask), (N + 5, c.mask, c.dmask)):
        s.shift_stage_bounds(n, mask=dmask, B=B)
        ref.shift(B, n, mask)
        c.same_stage(ref, f"shift by {n}")
    lim = c.limits(per_stage=True)
    s.set_stage_limits(**dev(lim))
    ref.set_limits(B, c.tric, None, **lim)
    c.same_stage(ref, "limits")
    # clear, then a writer with the per-robot table on: the refill takes each robot's own column of that table
    s.clear_stage_bounds()
    assert s.stage_bounds() is None
    rp = c.rp_ref()
    box = {k: rnd(c.rng, n, B) for k, n in c.fields[:4]}
    s.set_robot_params(**dev(box), mask=c.dmask)
    rp.set(B, c.mask, **box)
    ref = c.sb_ref(rp)
    s.shift_stage_bounds(1, mask=c.dmask, B=B)
    ref.shift(B, 1, c.mask)  # (every stage is the same: the fill itself)
    c.same_stage(ref, "refill from the per-robot table")
    part = c.stage_src(("ubx", "lbu"))
    s.set_stage_bounds(**dev(part), mask=c.dmask)
    ref.set(B, c.mask, **part)
    c.same_stage(ref, "refill, then two fields")
    c.same_rows(s.robot_params, rp, "the per-robot table is not the stage writers'")
