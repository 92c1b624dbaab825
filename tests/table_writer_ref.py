"""A plain numpy model of the three per-robot device tables (csrc/robot_tables.hip): what each holds after a sequence of
fill / set / limits / shift calls. Every value is a float32 copy or negation of an input, so the device tables must
match these bit for bit (tests/test_gpu_table_writers.py); the model's own invariants: tests/test_table_writer_ref.py.

A writer touches robot i only for i < B and mask[i] != 0 (mask None: every i < B); every other column keeps what it
held, at first the fill."""
import numpy as np

BOX = (("lbx", -1), ("ubx", 1)), (("lbu", -1), ("ubu", 1))  # the box fields of the states and of the inputs, with signs


def _sel(B, mask):
    i = np.arange(B)
    return i if mask is None else i[np.asarray(mask)[:B] != 0]


def _f32(a):
    a = np.asarray(a)
    assert a.dtype == np.float32, a.dtype
    return a


def _limit_stores(tric, nbx, nbu, v_max=None, a_max=None, alpha_min=None, alpha_max=None, dalpha_max=None):
    """nmpc_model_params_set_limits as stores (field, slot, source, negated): ref states in [-v_max, v_max], inputs in
    [-a_max, a_max]; tric: slot 1 of each box is the steering's, [alpha_min, alpha_max] and [-dalpha_max, dalpha_max],
    and the steering arrays are read for no other model"""
    nv, na = (1, 1) if tric else (nbx, nbu)
    st = []
    if v_max is not None:
        st += [(f, j, v_max, s < 0) for j in range(nv) for f, s in BOX[0]]
    if a_max is not None:
        st += [(f, j, a_max, s < 0) for j in range(na) for f, s in BOX[1]]
    if tric:
        if alpha_min is not None:
            st.append(("lbx", 1, alpha_min, False))
        if alpha_max is not None:
            st.append(("ubx", 1, alpha_max, False))
        if dalpha_max is not None:
            st += [("lbu", 1, dalpha_max, True), ("ubu", 1, dalpha_max, False)]
    return [(f, j, np.negative(_f32(src)) if neg else _f32(src)) for f, j, src, neg in st]


class RowTable:
    """A row-major table [rows][cap]: the per-robot table (fields lbx ubx lbu ubu W W_e) or the model table (the one
    field p). fields: ((name, rows), ...); column: float32 [rows], the fill."""

    def __init__(self, fields, cap, column):
        self.n = dict(fields)
        self.off, r = {}, 0
        for k, n in fields:
            self.off[k] = r
            r += n
        column = _f32(column)
        assert column.shape == (r,)
        self.a = np.repeat(column[:, None], cap, axis=1)

    def set(self, B, mask=None, **src):
        """src[field]: float32 [n][B], or None / absent (those rows stay)"""
        sel = _sel(B, mask)
        for k, v in src.items():
            if v is not None:
                assert _f32(v).shape == (self.n[k], B)
                self.a[self.off[k]:self.off[k] + self.n[k], sel] = v[:, sel]

    def set_limits(self, B, tric, mask=None, **lim):
        """lim: v_max, a_max, alpha_min, alpha_max, dalpha_max float32 [B], each optional"""
        sel = _sel(B, mask)
        for f, j, v in _limit_stores(tric, self.n["lbx"], self.n["lbu"], **lim):
            assert v.shape == (B,)
            self.a[self.off[f] + j, sel] = v[sel]


class StageTable:
    """The stage table, [stage][robot][row] with rows lbx ubx lbu ubu, N + 1 stages. box: the fill, float32 [rows] (the
    handle's box) or [rows][cap] (the first rows of the per-robot table when that is on). The input rows of stage N are
    never written: they hold the fill."""

    def __init__(self, N, nbx, nbu, cap, box):
        self.N, self.n = N, dict(lbx=nbx, ubx=nbx, lbu=nbu, ubu=nbu)
        self.off = dict(lbx=0, ubx=nbx, lbu=2 * nbx, ubu=2 * nbx + nbu)
        rows = 2 * nbx + 2 * nbu
        box = _f32(box)
        assert box.shape in ((rows,), (rows, cap))
        self.a = np.empty((N + 1, cap, rows), np.float32)
        self.a[:] = box if box.ndim == 1 else box.T

    def stages(self, field):
        return self.N + (field in ("lbx", "ubx"))

    def set(self, B, mask=None, **src):
        """src[field]: float32 [N + 1][nbx][B] (lbx, ubx) or [N][nbu][B] (lbu, ubu), or None / absent"""
        sel = _sel(B, mask)
        for k, v in src.items():
            if v is not None:
                assert _f32(v).shape == (self.stages(k), self.n[k], B)
                self.a[:self.stages(k), sel, self.off[k]:self.off[k] + self.n[k]] = v[:, :, sel].transpose(0, 2, 1)

    def set_limits(self, B, tric, mask=None, **lim):
        """lim: v_max, alpha_min, alpha_max float32 [N + 1][B], a_max, dalpha_max [N][B], each optional"""
        sel = _sel(B, mask)
        for f, j, v in _limit_stores(tric, self.n["lbx"], self.n["lbu"], **lim):
            assert v.shape == (self.stages(f), B)
            self.a[:self.stages(f), sel, self.off[f] + j] = v[:, sel]

    def shift(self, B, n, mask=None):
        """stage k of every row = stage min(k + n, last), last = N (state rows) or N - 1 (input rows)"""
        sel = _sel(B, mask)
        for f in self.n:
            last = self.stages(f) - 1
            src = np.minimum(np.arange(last + 1) + n, last)
            cols = slice(self.off[f], self.off[f] + self.n[f])
            self.a[:last + 1, sel, cols] = self.a[src][:, sel, cols]

    def bytes(self):
        """the table as nmpc_batch_stage_bounds shows it: uint8 [1][bytes]"""
        return self.a.reshape(1, -1).view(np.uint8)


def decode_stage(raw, N, cap, rows):
    """the stage table's bytes (uint8, any shape) as float32 [stage][robot][row]"""
    return np.ascontiguousarray(raw).reshape(-1).view(np.float32).reshape(N + 1, cap, rows)
