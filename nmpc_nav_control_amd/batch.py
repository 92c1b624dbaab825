"""Batched solve path on the device: a thin Python owner of an ``nmpc_batch`` handle (libnmpc_amd.so).

Device memory and streams come from PyTorch (plumbing only); every array is an fp32 torch CUDA tensor in
the instance-minor ``[field][B]`` layout of include/nmpc_amd/nmpc_batch.h. All compute runs in the HIP
kernels of the library; there is no Python or CPU fallback.
"""
import ctypes

import torch

from ._lib import (KERNELS, MODEL_IDS, PLAN_MODES, REC_LAYOUTS, SCHEDULES, FleetRenew, FleetStats, LaunchPlan,
                   ModelParams, NodeInputStruct, NodeParamsStruct, RobotParamsStruct, SepGuardStruct, SepRuleStruct,
                   SpeedMapStruct, SpeedRuleStruct, StageBoundsStruct, TracksStruct, check, default_params, lib,
                   model_dims)


def _ptr(t, dtype=None, shape=None, name="argument"):
    """Device pointer of a contiguous CUDA tensor, checked against the dtype and shape the kernel reads (a
    wrong dtype would be reinterpreted silently by the C ABI)."""
    if t is None:
        return None
    if not t.is_cuda:
        raise ValueError(f"{name}: expected a device tensor")
    if not t.is_contiguous():
        raise ValueError(f"{name}: expected a contiguous tensor")
    if dtype is not None and t.dtype not in (dtype if isinstance(dtype, tuple) else (dtype,)):
        raise TypeError(f"{name}: expected dtype {dtype}, got {t.dtype}")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name}: expected shape {tuple(shape)}, got {tuple(t.shape)}")
    return ctypes.c_void_p(t.data_ptr())


F32, F64, I32, I64, U8 = torch.float32, torch.float64, torch.int32, torch.int64, (torch.uint8, torch.bool)


def _stream(stream):
    s = stream if stream is not None else torch.cuda.current_stream()
    return ctypes.c_void_p(s.cuda_stream)


def _segs_stride(segs, B):
    """Records per robot of segs, float64 [B][S][16] (the nmpc_path_segment layout)."""
    if segs.dim() != 3 or segs.shape[0] != B or segs.shape[2] != 16:
        raise ValueError(f"segs: expected shape ({B}, S, 16), got {tuple(segs.shape)}")
    return segs.shape[1]


class NodeParams:
    """nmpc_node_params (include/nmpc_amd/nmpc_batch.h): the node's thresholds, angles in radians. ``default()``
    is the shipped nmpc_nav_control.yaml; keyword arguments override fields (``NodeParams.default(max_pos_err=1.0)``)."""

    def __init__(self, **fields):
        self.c = NodeParamsStruct()
        check(lib().nmpc_node_params_default(ctypes.byref(self.c)), "nmpc_node_params_default")
        for k, v in fields.items():
            if k not in dict(NodeParamsStruct._fields_):
                raise AttributeError(f"nmpc_node_params has no field {k}")
            setattr(self.c, k, v)

    @classmethod
    def default(cls, **fields):
        return cls(**fields)

    def __getattr__(self, k):
        if k != "c" and k in dict(NodeParamsStruct._fields_):
            return getattr(self.c, k)
        raise AttributeError(k)


class NodeInput:
    """nmpc_node_input (include/nmpc_amd/nmpc_batch.h): the arguments of the node's input stage. ``default()`` is the
    shipped configuration (40 Hz, transform_timeout 0.1 s, the pose check lost as in getInputData, lenient, no
    recentre); keyword arguments override fields. The scalar fields are numbers; steer (float32 [B]), steer_ok, valid,
    moved (uint8 [B]), pose, vel (float32 [3][B]) and steer_out (float32 [B]) are device tensors or None, which this
    object keeps alive."""

    _SHAPES = dict(steer=(F32, 1), steer_ok=(U8, 1), valid=(torch.uint8, 1), pose=(F32, 3), vel=(F32, 3),
                   steer_out=(F32, 1), moved=(torch.uint8, 1))

    def __init__(self, **fields):
        self.c = NodeInputStruct()
        check(lib().nmpc_node_input_default(ctypes.byref(self.c)), "nmpc_node_input_default")
        self.tensors = {}
        for k, v in fields.items():
            setattr(self, k, v)

    @classmethod
    def default(cls, **fields):
        return cls(**fields)

    def __setattr__(self, k, v):
        if k in ("c", "tensors"):
            object.__setattr__(self, k, v)
        elif k in self._SHAPES:
            self.tensors[k] = v
        elif k in dict(NodeInputStruct._fields_):
            setattr(self.c, k, v)
        else:
            raise AttributeError(f"nmpc_node_input has no field {k}")

    def __getattr__(self, k):
        if k in NodeInput._SHAPES:
            return self.tensors.get(k)
        if k != "c" and k in dict(NodeInputStruct._fields_):
            return getattr(self.c, k)
        raise AttributeError(k)

    def struct(self, B):
        """the C struct with the tensors' device pointers, each checked against the shape a call of B robots reads"""
        for k, (dtype, rows) in self._SHAPES.items():
            setattr(self.c, k, _ptr(self.tensors.get(k), dtype, (B,) if rows == 1 else (rows, B), k))
        return self.c


class SpeedMap:
    """nmpc_speed_map (include/nmpc_amd/nmpc_batch.h): a grid of speed limits in map coordinates. (x0, y0) is the low
    corner of cell (0, 0), res the cell edge in metres, vmax a float32 device tensor [h][w] (row cy, column cx; +inf: no
    limit), which this object keeps alive; outside is the limit off the grid."""

    def __init__(self, x0, y0, res, vmax, outside=float("inf")):
        if vmax is None or vmax.dim() != 2:
            raise ValueError("vmax: expected a device tensor [h][w]")
        self.vmax = vmax
        h, w = vmax.shape
        self.c = SpeedMapStruct(x0=float(x0), y0=float(y0), res=float(res), w=int(w), h=int(h),
                                vmax=_ptr(vmax, F32, (h, w), "vmax"), outside=float(outside))


class Tracks:
    """nmpc_tracks (include/nmpc_amd/nmpc_batch.h): predicted paths in map coordinates, a float64 device tensor
    xy [K+1][2][M] (track j at stage k, k * dt from now), which this object keeps alive; None: no tracks (M = 0).
    own_first: robot i of a call is track own_first + i and skips it (-1: no track is the handle's)."""

    def __init__(self, xy=None, own_first=-1):
        if xy is not None and (xy.dim() != 3 or xy.shape[1] != 2):
            raise ValueError("xy: expected a device tensor [K+1][2][M]")
        self.xy = xy
        K1, M = (1, 0) if xy is None else (xy.shape[0], xy.shape[2])
        self.M, self.K = int(M), int(K1) - 1
        self.c = TracksStruct(xy=_ptr(xy, F64, (K1, 2, M), "xy") if xy is not None else None, M=self.M, K=self.K,
                              own_first=int(own_first))


class SepGuard:
    """nmpc_sep_guard (include/nmpc_amd/nmpc_batch.h): right of way and the protective hold on top of the separation
    rule. priority int32 [M] device or None (larger wins, equal: both count; INT_MAX for what must always count),
    own_priority int32 [B] device or None (then priority[own_first + i]); this object keeps both alive. A robot is held
    when the smallest unfiltered gap over the stages 0..min(hold_stages, N) is below stop_gap and released at or above
    release_gap; hold=0: right of way only."""

    def __init__(self, priority=None, own_priority=None, stop_gap=0.45, release_gap=0.55, hold_stages=4, hold=1):
        self.priority, self.own_priority = priority, own_priority
        I32 = torch.int32
        for name, a in (("priority", priority), ("own_priority", own_priority)):
            if a is not None and a.dim() != 1:
                raise ValueError(f"{name}: expected a device tensor int32 [M] (priority) or [B] (own_priority)")
        self.c = SepGuardStruct(
            priority=_ptr(priority, I32, tuple(priority.shape), "priority") if priority is not None else None,
            own_priority=_ptr(own_priority, I32, tuple(own_priority.shape), "own_priority")
            if own_priority is not None else None,
            stop_gap=float(stop_gap), release_gap=float(release_gap), hold_stages=int(hold_stages), hold=int(hold))


def _sep_rule(clearance, gain, range, ahead_only):
    return SepRuleStruct(clearance=float(clearance), gain=float(gain), range=float(range), ahead_only=int(ahead_only))


def _speed_rule(slope, v_floor):
    return SpeedRuleStruct(slope=float(slope), v_floor=float(v_floor))


class BatchSolver:
    """B independent OCP instances of one model, solved in lockstep on one GPU.

    ``solve`` is the batched ``{name}_acados_solve`` on caller-packed x0 / yref; ``run`` is the batched
    ``NMPCNavControl{Diff,Omni4,Tric}::run`` (pre-solve, SQP-RTI, post-solve) with the warm-start
    iterate and carried vel-ref states resident on the device between ticks.
    """

    fused_stats = True  # fleet_sim_step_renew accumulates the solve statistics in its own launch (nmpc_fleet_stats)

    def __init__(self, model, N, capacity, params=None, device="cuda", kernel=None, record_layout=None):
        self.model = model
        self.N = int(N)
        self.capacity = int(capacity)
        self.device = torch.device(device)
        self.params = params if params is not None else default_params(model, N)
        self.params.model = MODEL_IDS[model]
        self.params.N = self.N
        d = model_dims(model)
        self.nx, self.nu, self.ny, self.nbx, self.nbu = d["nx"], d["nu"], d["ny"], d["nbx"], d["nbu"]
        self.np = d["np"]
        self._h = ctypes.c_void_p()
        self._speed_map = None  # the attached SpeedMap (set_speed_map): its grid is the library's to read
        self._tracks = None     # the attached Tracks (set_tracks): likewise its buffer
        self._sep_guard = None  # the attached SepGuard (set_sep_guard): likewise its priorities
        with torch.cuda.device(self.device):
            check(lib().nmpc_batch_create(ctypes.byref(self.params), self.capacity, ctypes.byref(self._h)),
                  "nmpc_batch_create")
        self.kernel = "team"
        if kernel is not None:
            self.set_kernel(kernel)
        if record_layout is not None:
            self.set_record_layout(record_layout)

    def set_record_layout(self, layout):
        """The team kernel's scratch record layout of this handle: 'auto' (the model's choice from this handle
        alone, fixed at create), 'wide' or 'split' (nmpc_batch_set_record_layout; diff has both, tric only split,
        omni4 only wide). Robots whose multipliers sit in the other layout start their next IPM cold."""
        check(lib().nmpc_batch_set_record_layout(self._h, REC_LAYOUTS[layout]), "nmpc_batch_set_record_layout")

    def plan_ex(self, B, mode="solve"):
        """The launch a call of B robots makes (nmpc_batch_plan_ex): dict with kernel ('team' / 'rowpar'),
        waves_per_robot, segments, record_layout ('wide' / 'split'), warm_tag and record_bytes. mode: 'solve',
        'run' or 'run_path'."""
        p = LaunchPlan()
        check(lib().nmpc_batch_plan_ex(self._h, int(B), PLAN_MODES[mode], ctypes.byref(p)), "nmpc_batch_plan_ex")
        return dict(kernel="rowpar" if p.kernel else "team", waves_per_robot=p.waves_per_robot, segments=p.segments,
                    record_layout="split" if p.record_layout else "wide", warm_tag=p.warm_tag,
                    record_bytes=p.record_bytes)

    def set_handoff(self, iteration):
        """The team kernel's hand-off iteration C of this handle (nmpc_batch_set_handoff; 0: off, the create-time setting;
        -1: the measured default, NMPC_HANDOFF_AUTO): in the launches
        that qualify, a robot whose IPM has not stopped at the top of iteration C is finished alone by one wave of its
        block, in the segmented form."""
        check(lib().nmpc_batch_set_handoff(self._h, int(iteration)), "nmpc_batch_set_handoff")

    def plan_handoff(self, B, mode="solve"):
        """Whether a launch of B robots takes the hand-off (nmpc_batch_plan_handoff): dict with iteration (C, or 0:
        the plain kernel), segments and lds_bytes of the hand-off form. mode: 'solve', 'run' or 'run_path'."""
        it, sg, lds = ctypes.c_int(), ctypes.c_int(), ctypes.c_size_t()
        check(lib().nmpc_batch_plan_handoff(self._h, int(B), PLAN_MODES[mode], ctypes.byref(it), ctypes.byref(sg),
                                            ctypes.byref(lds)), "nmpc_batch_plan_handoff")
        return dict(iteration=it.value, segments=sg.value, lds_bytes=lds.value)

    def set_kernel(self, kernel):
        """'team' (16-lane team per robot): the only kernel."""
        check(lib().nmpc_batch_set_kernel(self._h, KERNELS[kernel]), "nmpc_batch_set_kernel")
        self.kernel = kernel

    def plan(self, B):
        """The kernel a solve / run launch of B robots takes (nmpc_batch_plan): (name, waves per robot, segments),
        name 'team' (k_sqp_rti_team) or 'rowpar' (k_sqp_rti_rowpar; segments 0 = its serial phases)."""
        k, w, sg = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        check(lib().nmpc_batch_plan(self._h, int(B), ctypes.byref(k), ctypes.byref(w), ctypes.byref(sg)),
              "nmpc_batch_plan")
        return ("rowpar" if k.value else "team"), w.value, sg.value

    def set_schedule(self, mode):
        """Team placement of the team kernel: 'auto' (default), 'off', 'sorted' or 'interleaved'
        (include/nmpc_amd/nmpc_batch.h; no effect on any result)."""
        check(lib().nmpc_batch_set_schedule(self._h, SCHEDULES[mode]), "nmpc_batch_set_schedule")

    def close(self):
        if self._h:
            lib().nmpc_batch_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_params(self, params):
        check(lib().nmpc_batch_set_params(self._h, ctypes.byref(params)), "nmpc_batch_set_params")
        self.params = params

    def init_iterate(self, B=None, mode=0, stream=None):
        """mode 0: {name}_acados_create semantics (carried refs zeroed); mode 1: {name}_acados_reset (iterate
        zeroed, carried refs kept, as the per-robot reset mask)."""
        B = self.capacity if B is None else int(B)
        check(lib().nmpc_batch_init_iterate(self._h, B, int(mode), _stream(stream)), "nmpc_batch_init_iterate")

    def state(self):
        """Views of the resident device state: xbar [(N+1)*NX][cap], ubar [N*NU][cap], carried [NBX][cap]."""
        xb, ub, cr = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
        stride = ctypes.c_int()
        check(lib().nmpc_batch_state(self._h, ctypes.byref(xb), ctypes.byref(ub), ctypes.byref(cr),
                                     ctypes.byref(stride)), "nmpc_batch_state")
        S = stride.value
        return (_DeviceView(xb.value, ((self.N + 1) * self.nx, S), self.device),
                _DeviceView(ub.value, (self.N * self.nu, S), self.device),
                _DeviceView(cr.value, (self.nbx, S), self.device))

    def warm_state(self):
        """Views of the IPM warm-start state (nmpc_batch_warm_state): per-robot flags [cap] (uint8) and the
        scratch records (bytes); with state() everything a solve reads from the handle."""
        w, sc, nb = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_size_t()
        check(lib().nmpc_batch_warm_state(self._h, ctypes.byref(w), ctypes.byref(sc), ctypes.byref(nb)),
              "nmpc_batch_warm_state")
        return (_DeviceView(w.value, (1, self.capacity), self.device, torch.uint8),
                _DeviceView(sc.value, (1, nb.value // 4), self.device))

    def forget_warm(self, mask=None, B=None, stream=None):
        """Cold IPM start at the next solve for the robots where mask != 0 (None: all of them); the iterate stays
        (nmpc_batch_forget_warm)."""
        B = self.capacity if B is None else int(B)
        check(lib().nmpc_batch_forget_warm(self._h, B, _ptr(mask, U8, (B,), "mask"), _stream(stream)),
              "nmpc_batch_forget_warm")

    def set_robot_params(self, lbx=None, ubx=None, lbu=None, ubu=None, W=None, W_e=None, mask=None, stream=None):
        """Per-robot bounds and weights (nmpc_batch_set_robot_params): each argument a float32 device tensor [n][B]
        (n = nbx, nbx, nbu, nbu, ny, nx) or None (those rows stay); mask uint8 [B] selects the robots (None: all).
        One launch on the stream; from then on every launch of this solver takes each robot's values from the table
        (until clear_robot_params)."""
        given = dict(lbx=lbx, ubx=ubx, lbu=lbu, ubu=ubu, W=W, W_e=W_e)
        B = self._batch_given(given, 1, "set_robot_params: no field given")
        rp = RobotParamsStruct(**{k: _ptr(given[k], F32, (n, B), k) for k, n in self._rp_fields()})
        check(lib().nmpc_batch_set_robot_params(self._h, B, ctypes.byref(rp), _ptr(mask, U8, (B,), "mask"),
                                                _stream(stream)), "nmpc_batch_set_robot_params")

    def set_robot_limits(self, v_max=None, a_max=None, alpha_min=None, alpha_max=None, dalpha_max=None, mask=None,
                         stream=None):
        """The batched nmpc_model_params_set_limits (nmpc_batch_set_robot_limits): float32 device tensors [B], each
        optional; the steering ones are read for tric only. mask as set_robot_params."""
        arrs = dict(v_max=v_max, a_max=a_max, alpha_min=alpha_min, alpha_max=alpha_max, dalpha_max=dalpha_max)
        B = self._batch_given(arrs, 0, "set_robot_limits: no limit given")
        check(lib().nmpc_batch_set_robot_limits(self._h, B, *[_ptr(t, F32, (B,), k) for k, t in arrs.items()],
                                                _ptr(mask, U8, (B,), "mask"), _stream(stream)),
              "nmpc_batch_set_robot_limits")

    def robot_params(self):
        """View of the per-robot table [rows][cap] (rows lbx ubx lbu ubu W W_e), or None while it is off
        (nmpc_batch_robot_params)."""
        return self._table_view("nmpc_batch_robot_params")

    def clear_robot_params(self):
        """Turn the per-robot table off: launches use the handle's parameters again."""
        check(lib().nmpc_batch_clear_robot_params(self._h), "nmpc_batch_clear_robot_params")

    def set_stage_bounds(self, lbx=None, ubx=None, lbu=None, ubu=None, mask=None, stream=None):
        """Stage-varying bounds (nmpc_batch_set_stage_bounds): lbx / ubx float32 device tensors [N+1][nbx][B], lbu /
        ubu [N][nbu][B], each optional (those rows stay); mask uint8 [B] selects the robots (None: all). One launch on
        the stream; from then on every launch of this solver takes each robot's box at stage k from the stage table
        (until clear_stage_bounds)."""
        N = self.N
        rows = dict(lbx=(lbx, N + 1, self.nbx), ubx=(ubx, N + 1, self.nbx), lbu=(lbu, N, self.nbu),
                    ubu=(ubu, N, self.nbu))
        B = self._batch_given({k: r[0] for k, r in rows.items()}, -1, "set_stage_bounds: no field given")
        sb =StageBoundsStruct(**{k: _ptr(t, F32, (ns, n, B), k) for k, (t, ns, n) in rows.items()})
        check(lib().nmpc_batch_set_stage_bounds(self._h, B, ctypes.byref(sb), _ptr(mask, U8, (B,), "mask"),
                                                _stream(stream)), "nmpc_batch_set_stage_bounds")

    def set_stage_limits(self, v_max=None, a_max=None, alpha_min=None, alpha_max=None, dalpha_max=None, mask=None,
                         stream=None):
        """The batched, per-stage nmpc_model_params_set_limits (nmpc_batch_set_stage_limits): v_max, alpha_min,
        alpha_max float32 device tensors [N+1][B], a_max and dalpha_max [N][B], each optional; the steering ones are
        read for tric only. mask as set_stage_bounds."""
        N = self.N
        arrs = dict(v_max=(v_max, N + 1), a_max=(a_max, N), alpha_min=(alpha_min, N + 1), alpha_max=(alpha_max, N + 1),
                    dalpha_max=(dalpha_max, N))
        B = self._batch_given({k: r[0] for k, r in arrs.items()}, -1, "set_stage_limits: no limit given")
        check(lib().nmpc_batch_set_stage_limits(self._h, B, *[_ptr(t, F32, (ns, B), k) for k, (t, ns) in arrs.items()],
                                                _ptr(mask, U8, (B,), "mask"), _stream(stream)),
              "nmpc_batch_set_stage_limits")

    def shift_stage_bounds(self, n=1, mask=None, B=None, stream=None):
        """Receding horizon (nmpc_batch_shift_stage_bounds): stage k of every row takes stage min(k + n, last), for the
        robots where mask != 0 (None: all of the first B, default the capacity)."""
        if int(n) < 0:
            raise ValueError("shift_stage_bounds: n must be >= 0")
        B = self.capacity if B is None else int(B)
        check(lib().nmpc_batch_shift_stage_bounds(self._h, B, int(n), _ptr(mask, U8, (B,), "mask"), _stream(stream)),
              "nmpc_batch_shift_stage_bounds")

    def stage_limits_from_map(self, map, pose=None, reset=None, mask=None, vlim=None, slope=0.8, v_floor=0.05, B=None,
                              stream=None):
        """The speed rows of the stage table from a SpeedMap (nmpc_batch_stage_limits_from_map): every stage of every
        processed robot's resident horizon is looked up in the map and the limit comes down along the horizon by at
        most slope * a_max * dt per stage, never below v_floor. pose float32 [3][B] and reset uint8 [B]: a robot with
        reset != 0 is looked up at its pose (its iterate is about to be zeroed); mask uint8 [B] selects the robots
        (None: all); vlim float32 [N+1][B] receives the limits. B: from pose, reset, mask or vlim, else the argument,
        else the capacity. One launch on the stream."""
        if reset is not None and pose is None:
            raise ValueError("stage_limits_from_map: reset needs pose")
        if B is None:
            given = [(pose, 1), (reset, 0), (mask, 0), (vlim, 1)]
            B = next((self._batch_of(t, ax) for t, ax in given if t is not None), self.capacity)
        B = int(B)
        rule = _speed_rule(slope, v_floor)
        check(lib().nmpc_batch_stage_limits_from_map(
            self._h, B, ctypes.byref(map.c), ctypes.byref(rule), _ptr(pose, F32, (3, B), "pose"),
            _ptr(reset, U8, (B,), "reset"), _ptr(mask, U8, (B,), "mask"), _ptr(vlim, F32, (self.N + 1, B), "vlim"),
            _stream(stream)), "nmpc_batch_stage_limits_from_map")

    def set_speed_map(self, map, slope=0.8, v_floor=0.05):
        """Attach a SpeedMap to the solver, or detach it (None) (nmpc_batch_set_speed_map): while one is attached,
        node_cycle runs stage_limits_from_map between its input stage and its tick, for the robots in GOTO_POSE or
        FOLLOW_PATH. The solver keeps the map object, and with it the grid, alive."""
        if map is None:
            check(lib().nmpc_batch_set_speed_map(self._h, None, None), "nmpc_batch_set_speed_map")
        else:
            rule = _speed_rule(slope, v_floor)
            check(lib().nmpc_batch_set_speed_map(self._h, ctypes.byref(map.c), ctypes.byref(rule)),
                  "nmpc_batch_set_speed_map")
        self._speed_map = map

    def export_tracks(self, xy, first=0, pose=None, reset=None, mode=None, B=None, stream=None):
        """The resident horizons of the robots [0, B) as tracks (nmpc_batch_export_tracks): the columns first ..
        first + B - 1 of xy, float64 [K+1][2][M] in map coordinates, stage min(k, N) at k. pose float32 [3][B]; a robot
        with reset != 0 (uint8 [B]) or, when mode (uint8 [B]) is given, one that is neither in GOTO_POSE nor in
        FOLLOW_PATH is written at its pose at every stage. B: from pose, reset or mode, else the argument, else the
        capacity. One launch on the stream."""
        if (reset is not None or mode is not None) and pose is None:
            raise ValueError("export_tracks: reset and mode need pose")
        if xy is None or xy.dim() != 3 or xy.shape[1] != 2:
            raise ValueError("xy: expected a device tensor [K+1][2][M]")
        if B is None:
            given = [(pose, 1), (reset, 0), (mode, 0)]
            B = next((self._batch_of(t, ax) for t, ax in given if t is not None), self.capacity)
        B = int(B)
        K1, M = xy.shape[0], xy.shape[2]
        check(lib().nmpc_batch_export_tracks(
            self._h, B, _ptr(pose, F32, (3, B), "pose"), _ptr(reset, U8, (B,), "reset"), _ptr(mode, U8, (B,), "mode"),
            _ptr(xy, F64, (K1, 2, M), "xy"), int(M), int(K1) - 1, int(first), _stream(stream)),
            "nmpc_batch_export_tracks")

    def stage_limits_from_tracks(self, tracks, map=None, pose=None, reset=None, mask=None, vlim=None, gap=None,
                                 clearance=0.6, gain=1.0, range=3.0, ahead_only=1, slope=0.8, v_floor=0.05, B=None,
                                 stream=None, guard=None, gap_all=None):
        """The speed rows of the stage table from Tracks and, optionally, a SpeedMap
        (nmpc_batch_stage_limits_from_tracks): every stage of every processed robot's horizon gets the cap
        gain * (gap - clearance) from the gap to the nearest track within range at the same time (ahead_only: in the
        half plane of its direction of travel), and the speed map's rule makes a limit profile of the caps. pose, reset,
        mask, vlim, slope, v_floor as stage_limits_from_map; gap float32 [N+1][B] receives the gaps (+inf: no track
        counts). guard: a SepGuard (nmpc_batch_stage_limits_from_tracks_ex): gap is then the gap to the nearest track
        the robot gives way to, gap_all float32 [N+1][B] receives the unfiltered one, a robot that is held (sep_state)
        stands at its pose, and sep_hold may follow."""
        if reset is not None and pose is None:
            raise ValueError("stage_limits_from_tracks: reset needs pose")
        if gap_all is not None and guard is None:
            raise ValueError("stage_limits_from_tracks: gap_all needs a guard")
        if guard is not None and guard.priority is not None and guard.priority.numel() != tracks.M:
            raise ValueError(f"guard: priority has {guard.priority.numel()} entries, the tracks are {tracks.M}")
        if B is None:
            given = [(pose, 1), (reset, 0), (mask, 0), (vlim, 1), (gap, 1)]
            B = next((self._batch_of(t, ax) for t, ax in given if t is not None), self.capacity)
        B = int(B)
        sep, rule = _sep_rule(clearance, gain, range, ahead_only), _speed_rule(slope, v_floor)
        if guard is not None and guard.own_priority is not None and guard.own_priority.numel() < B:
            raise ValueError(f"guard: own_priority has {guard.own_priority.numel()} entries, the call has {B} robots")
        if guard is not None:
            check(lib().nmpc_batch_stage_limits_from_tracks_ex(
                self._h, B, ctypes.byref(tracks.c), ctypes.byref(sep), ctypes.byref(guard.c),
                ctypes.byref(map.c) if map is not None else None, ctypes.byref(rule), _ptr(pose, F32, (3, B), "pose"),
                _ptr(reset, U8, (B,), "reset"), _ptr(mask, U8, (B,), "mask"), _ptr(vlim, F32, (self.N + 1, B), "vlim"),
                _ptr(gap, F32, (self.N + 1, B), "gap"), _ptr(gap_all, F32, (self.N + 1, B), "gap_all"),
                _stream(stream)), "nmpc_batch_stage_limits_from_tracks_ex")
            return
        check(lib().nmpc_batch_stage_limits_from_tracks(
            self._h, B, ctypes.byref(tracks.c), ctypes.byref(sep), ctypes.byref(map.c) if map is not None else None,
            ctypes.byref(rule), _ptr(pose, F32, (3, B), "pose"), _ptr(reset, U8, (B,), "reset"),
            _ptr(mask, U8, (B,), "mask"), _ptr(vlim, F32, (self.N + 1, B), "vlim"),
            _ptr(gap, F32, (self.N + 1, B), "gap"), _stream(stream)), "nmpc_batch_stage_limits_from_tracks")

    def set_tracks(self, tracks, export_own=False, clearance=0.6, gain=1.0, range=3.0, ahead_only=1):
        """Attach Tracks to the solver, or detach them (None) (nmpc_batch_set_tracks): while they are attached,
        node_cycle runs, between its input stage and its tick, export_tracks of its own robots at tracks.own_first (with
        export_own) and stage_limits_from_tracks, with the attached speed map if there is one, for the robots in
        GOTO_POSE or FOLLOW_PATH. The solver keeps the object, and with it the buffer, alive."""
        if tracks is None:
            check(lib().nmpc_batch_set_tracks(self._h, None, None, 0), "nmpc_batch_set_tracks")
        else:
            sep = _sep_rule(clearance, gain, range, ahead_only)
            check(lib().nmpc_batch_set_tracks(self._h, ctypes.byref(tracks.c), ctypes.byref(sep), int(bool(export_own))),
                  "nmpc_batch_set_tracks")
        self._tracks = tracks

    def sep_hold(self, guard, mode=None, reset=None, held_out=None, B=None, stream=None):
        """The protective hold (nmpc_batch_sep_hold): one launch on what the preceding stage_limits_from_tracks call
        with a guard left on the handle; updates the handle's held (sep_state) and writes held_out uint8 [B] when
        given. mode uint8 [B] or None (every robot is judged), reset uint8 [B] or None."""
        if B is None:
            given = [(mode, 0), (reset, 0), (held_out, 0)]
            B = next((self._batch_of(t, ax) for t, ax in given if t is not None), self.capacity)
        B = int(B)
        check(lib().nmpc_batch_sep_hold(self._h, B, ctypes.byref(guard.c), _ptr(mode, U8, (B,), "mode"),
                                        _ptr(reset, U8, (B,), "reset"), _ptr(held_out, U8, (B,), "held_out"),
                                        _stream(stream)), "nmpc_batch_sep_hold")

    def set_sep_guard(self, guard):
        """Attach a SepGuard to the solver, or detach it (None) (nmpc_batch_set_sep_guard); either way held is cleared.
        While a guard and tracks are attached, node_cycle runs the export, the guarded writer and the hold, and a held
        robot does not tick: stop command, its mode stays, event NMPC_NODE_EV_HELD."""
        if guard is not None and guard.priority is not None and self._tracks is not None \
                and guard.priority.numel() != self._tracks.M:
            raise ValueError(f"guard: priority has {guard.priority.numel()} entries, the tracks are {self._tracks.M}")
        check(lib().nmpc_batch_set_sep_guard(self._h, ctypes.byref(guard.c) if guard is not None else None),
              "nmpc_batch_set_sep_guard")
        self._sep_guard = guard

    def sep_state(self):
        """View of the hold's state (nmpc_batch_sep_state): held [1][cap] (uint8). State, for checkpoints."""
        h = ctypes.c_void_p()
        check(lib().nmpc_batch_sep_state(self._h, ctypes.byref(h)), "nmpc_batch_sep_state")
        return _DeviceView(h.value, (1, self.capacity), self.device, torch.uint8)

    def stage_bounds(self):
        """View of the stage table as opaque bytes [1][bytes] (uint8), or None while it is off
        (nmpc_batch_stage_bounds)."""
        return self._table_view("nmpc_batch_stage_bounds", opaque=True)

    def clear_stage_bounds(self):
        """Turn the stage table off: launches use one box per robot again."""
        check(lib().nmpc_batch_clear_stage_bounds(self._h), "nmpc_batch_clear_stage_bounds")

    def set_robot_model(self, p, mask=None, stream=None):
        """Per-robot model parameters (nmpc_batch_set_robot_model): p a float32 device tensor [np][B] (diff {b, tau_v},
        omni4 {l1 + l2, tau_v}, tric {d, tau_v, tau_a}); mask uint8 [B] selects the robots (None: all). One launch on
        the stream; from then on every launch of this solver, and the harness plant, takes each robot's p from the
        model table (until clear_robot_model)."""
        B = self._batch_of(p)
        check(lib().nmpc_batch_set_robot_model(self._h, B, _ptr(p, F32, (self.np, B), "p"),
                                               _ptr(mask, U8, (B,), "mask"), _stream(stream)),
              "nmpc_batch_set_robot_model")

    def robot_model(self):
        """View of the model table [np][cap], or None while it is off (nmpc_batch_robot_model)."""
        return self._table_view("nmpc_batch_robot_model")

    def clear_robot_model(self):
        """Turn the model table off: launches use the handle's p again."""
        check(lib().nmpc_batch_clear_robot_model(self._h), "nmpc_batch_clear_robot_model")

    def set_robot_frame(self, origin, mask=None, stream=None):
        """Per-robot map frames (nmpc_batch_set_robot_frame): origin a float64 device tensor [2][B], every robot's
        origin x and y in map coordinates; mask uint8 [B] selects the robots (None: all). One launch on the stream,
        which also moves those robots' resident iterate so that its map position stays. From then on every fp32
        position of this solver's launches is relative to the robot's origin, and the float64 path segments stay in
        map coordinates (until clear_robot_frame)."""
        B = self._batch_of(origin)
        check(lib().nmpc_batch_set_robot_frame(self._h, B, _ptr(origin, F64, (2, B), "origin"),
                                               _ptr(mask, U8, (B,), "mask"), _stream(stream)),
              "nmpc_batch_set_robot_frame")

    def recentre(self, pose_map, radius, mask=None, moved=None, stream=None):
        """set_robot_frame with a computed origin (nmpc_batch_recentre): pose_map float64 [2 or 3][B], the robots' map
        positions. A masked robot farther than radius (in x or y) from its origin gets the origin rint(position) and
        moved[i] = 1 (moved uint8 [B], optional); the others stay, moved[i] = 0."""
        B = self._batch_of(pose_map)
        if pose_map.shape[0] not in (2, 3):
            raise ValueError(f"pose_map: expected 2 or 3 rows, got {pose_map.shape[0]}")
        check(lib().nmpc_batch_recentre(self._h, B, _ptr(pose_map, F64, None, "pose_map"), float(radius),
                                        _ptr(mask, U8, (B,), "mask"), _ptr(moved, torch.uint8, (B,), "moved"),
                                        _stream(stream)), "nmpc_batch_recentre")

    def to_frame(self, map_values, out=None, stream=None):
        """Map coordinates into the robots' frames (nmpc_batch_to_frame): map_values float64 [n][c][B] or [c][B]
        (pose, traj, goal, x0, yref ...); components 0 and 1 of each group become float32 (v - origin), the others
        are converted. Returns the float32 tensor (out, when given)."""
        v = map_values if map_values.dim() == 3 else map_values.unsqueeze(0)
        n, c, B = v.shape
        self._batch_of(v, 2)
        res = out if out is not None else torch.empty(map_values.shape, dtype=F32, device=self.device)
        check(lib().nmpc_batch_to_frame(self._h, B, _ptr(v, F64, None, "map_values"), n, c,
                                        _ptr(res, F32, tuple(map_values.shape), "out"), _stream(stream)),
              "nmpc_batch_to_frame")
        return res

    def from_frame(self, frame_values, out=None, stream=None):
        """Frame values back into map coordinates (nmpc_batch_from_frame): frame_values float32 [n][c][B] or [c][B]
        (x1, xtraj, traj_out ...); returns the float64 tensor (out, when given)."""
        v = frame_values if frame_values.dim() == 3 else frame_values.unsqueeze(0)
        n, c, B = v.shape
        self._batch_of(v, 2)
        res = out if out is not None else torch.empty(frame_values.shape, dtype=F64, device=self.device)
        check(lib().nmpc_batch_from_frame(self._h, B, _ptr(v, F32, None, "frame_values"), n, c,
                                          _ptr(res, F64, tuple(frame_values.shape), "out"), _stream(stream)),
              "nmpc_batch_from_frame")
        return res

    def robot_frame(self):
        """View of the frame table [2][cap] (float64), or None while it is off (nmpc_batch_robot_frame)."""
        tb, stride = ctypes.c_void_p(), ctypes.c_int()
        check(lib().nmpc_batch_robot_frame(self._h, ctypes.byref(tb), ctypes.byref(stride)), "nmpc_batch_robot_frame")
        return _DeviceView(tb.value, (2, stride.value), self.device, F64) if tb.value else None

    def clear_robot_frame(self, stream=None):
        """Move every robot's iterate back to map coordinates and turn the frame table off (one launch)."""
        check(lib().nmpc_batch_clear_robot_frame(self._h, _stream(stream)), "nmpc_batch_clear_robot_frame")

    def save_state(self):
        """Device copies of everything a solve reads from the handle: iterate, carried refs, warm start (five
        tensors), then the per-robot table as a tensor when it is on, then the stage table as
        {"stage_bounds": bytes}, the model table as {"robot_model": tensor} and the frame table as {"robot_frame":
        tensor} when they are on, then the node's input state as {"node_input": {...}} when it is enabled."""
        saved = [v.to_tensor() for v in self.state() + self.warm_state()]
        for name, view, _, _ in self._tables():
            v = view()
            if v is not None:
                saved.append(v.to_tensor() if name is None else {name: v.to_tensor()})
        ist = self.input_state()
        if ist is not None:  # the node's input state: {"node_input": {"depth": int, "stamp": tensor, ...}}
            saved.append({"node_input": {k: (v if k == "depth" else v.to_tensor()) for k, v in ist.items()}})
        return saved

    def restore_state(self, saved):
        # every table as the checkpoint has it: loaded when it is there, else switched off. The frame table first, before
        # the iterate that is relative to it (its writer and its clear move the iterate that is resident then), then the
        # model table, the per-robot table last (the stage table's bytes replace its first fill, whatever that took
        # from the latter)
        have = {}
        for e in saved[5:]:
            have.update(e if isinstance(e, dict) else {None: e})
        # the input state as the checkpoint has it; a checkpoint without one leaves a state that is on as enable_input
        # does, all 0
        inp, ist = have.pop("node_input", None), self.input_state()
        if inp is not None:
            self.enable_input(inp["depth"])
            ist = self.input_state()
        if ist is not None:
            for k, v in ist.items():
                if k != "depth":
                    v.copy_from(inp[k] if inp is not None else torch.zeros(v.shape, dtype=v.dtype))
        for name, _, load, clear in reversed(self._tables()):
            if name in have:
                load(have[name].to(self.device))
                torch.cuda.synchronize()
            else:
                clear()
        for v, t in zip(self.state() + self.warm_state(), saved):
            v.copy_from(t)

    def _tables(self):
        """The per-robot device tables in save_state's order: the key of the table's entry in a checkpoint (None: a
        bare tensor), its view, how a saved copy is loaded (through a writer, which allocates the table and switches
        it on) and how it is switched off."""
        def load_params(t):
            cuts, off = {}, 0
            for k, n in self._rp_fields():
                cuts[k] = t[off:off + n].contiguous()
                off += n
            self.set_robot_params(**cuts)

        def load_stage(t):
            self.shift_stage_bounds(0)  # (a shift by no stage is the writer that writes nothing)
            self.stage_bounds().copy_from(t)

        return [(None, self.robot_params, load_params, self.clear_robot_params),
                ("stage_bounds", self.stage_bounds, load_stage, self.clear_stage_bounds),
                ("robot_model", self.robot_model, lambda t: self.set_robot_model(t.contiguous()),
                 self.clear_robot_model),
                ("robot_frame", self.robot_frame, lambda t: self.set_robot_frame(t.contiguous()),
                 self.clear_robot_frame)]

    def _rp_fields(self):
        """the per-robot table's fields and their rows, in the table's order"""
        return (("lbx", self.nbx), ("ubx", self.nbx), ("lbu", self.nbu), ("ubu", self.nbu), ("W", self.ny),
                ("W_e", self.nx))

    def _table_view(self, fn, opaque=False):
        """View of a device table through its C view function, or None while the table is off: [rows][cap] float32, or
        (opaque) the table's bytes [1][bytes] uint8."""
        tb = ctypes.c_void_p()
        if opaque:
            nb = ctypes.c_size_t()
            check(getattr(lib(), fn)(self._h, ctypes.byref(tb), ctypes.byref(nb)), fn)
            shape, dtype = (1, nb.value), torch.uint8
        else:
            rows, stride = ctypes.c_int(), ctypes.c_int()
            check(getattr(lib(), fn)(self._h, ctypes.byref(tb), ctypes.byref(rows), ctypes.byref(stride)), fn)
            shape, dtype = (rows.value, stride.value), torch.float32
        return _DeviceView(tb.value, shape, self.device, dtype) if tb.value else None

    def empty(self, *shape, dtype=torch.float32):
        return torch.empty(*shape, dtype=dtype, device=self.device)

    def _batch_of(self, t, axis=1):
        """B of a call, from its first input: axis 1 of a [field][B] tensor, or the axis given."""
        B = t.shape[axis]
        if not 0 <= B <= self.capacity:
            raise ValueError(f"batch {B} exceeds the capacity {self.capacity}")
        return B

    def _batch_given(self, fields, axis, none_msg):
        """B of a table writer whose fields (name -> tensor or None) are each optional, from the first one given."""
        given = [t for t in fields.values() if t is not None]
        if not given:
            raise ValueError(none_msg)
        return self._batch_of(given[0], axis)

    def _outputs(self, B, cmd, u0, status, qp_iter, qp_res, stream):
        """The trailing arguments of every run-mode entry point: the per-robot outputs and the stream."""
        return (_ptr(cmd, F32, (3, B), "cmd"), _ptr(u0, F32, (self.nu, B), "u0"), _ptr(status, I32, (B,), "status"),
                _ptr(qp_iter, I32, (B,), "qp_iter"), _ptr(qp_res, F32, (3, B), "qp_res"), _stream(stream))

    def solve(self, x0, yref, We=None, reset=None, u0=None, x1=None, xtraj=None, utraj=None, status=None,
              qp_iter=None, qp_res=None, stream=None):
        B = self._batch_of(x0)
        ny_in = yref.shape[1]
        N, nx, nu = self.N, self.nx, self.nu
        check(lib().nmpc_batch_solve(
            self._h, B, _ptr(x0, F32, (nx, B), "x0"), _ptr(yref, F32, (N + 1, ny_in, B), "yref"), ny_in,
            _ptr(We, F32, (nx, B), "We"), _ptr(reset, U8, (B,), "reset"), _ptr(u0, F32, (nu, B), "u0"),
            _ptr(x1, F32, (nx, B), "x1"), _ptr(xtraj, F32, ((N + 1) * nx, B), "xtraj"),
            _ptr(utraj, F32, (N * nu, B), "utraj"), _ptr(status, I32, (B,), "status"),
            _ptr(qp_iter, I32, (B,), "qp_iter"), _ptr(qp_res, F32, (3, B), "qp_res"), _stream(stream)),
            "nmpc_batch_solve")

    def solve_iterate(self, x0, yref, xbar, ubar, We=None, reset=None, status=None, qp_iter=None, qp_res=None,
                      stream=None):
        """nmpc_batch_solve with a caller-held iterate: xbar [(N+1)*NX][ld], ubar [N*NU][ld] are read and overwritten
        with the new iterate in place (nmpc_batch_solve_iterate). The IPM warm start still comes from the handle's
        slot i: keep instance i in slot i across calls, or call forget_warm after reordering."""
        B = self._batch_of(x0)
        ld = xbar.shape[1]
        if ubar.shape[1] != ld:
            raise ValueError("xbar and ubar need the same leading dimension")
        ny_in = yref.shape[1]
        N, nx, nu = self.N, self.nx, self.nu
        check(lib().nmpc_batch_solve_iterate(
            self._h, B, _ptr(x0, F32, (nx, B), "x0"), _ptr(yref, F32, (N + 1, ny_in, B), "yref"), ny_in,
            _ptr(We, F32, (nx, B), "We"), _ptr(reset, U8, (B,), "reset"), _ptr(xbar, F32, ((N + 1) * nx, ld), "xbar"),
            _ptr(ubar, F32, (N * nu, ld), "ubar"), ld, _ptr(status, I32, (B,), "status"),
            _ptr(qp_iter, I32, (B,), "qp_iter"), _ptr(qp_res, F32, (3, B), "qp_res"), _stream(stream)),
            "nmpc_batch_solve_iterate")

    def run(self, pose, vel, traj, steer=None, traj_len=None, reset=None, cmd=None, u0=None, status=None,
            qp_iter=None, qp_res=None, stream=None):
        B = self._batch_of(pose)
        check(lib().nmpc_batch_run(
            self._h, B, _ptr(pose, F32, (3, B), "pose"), _ptr(vel, F32, (3, B), "vel"),
            _ptr(steer, F32, (B,), "steer"), _ptr(traj, F32, (self.N + 1, 3, B), "traj"),
            _ptr(traj_len, I32, (B,), "traj_len"), _ptr(reset, U8, (B,), "reset"),
            *self._outputs(B, cmd, u0, status, qp_iter, qp_res, stream)), "nmpc_batch_run")

    def run_path(self, pose, vel, segs, nseg, nearest_u, sample_period, is_holonomic=False, steer=None, reset=None,
                 traj_out=None, cmd=None, u0=None, status=None, qp_iter=None, qp_res=None, stream=None):
        """processFollowPath's getNextNPoses + run for B robots in one launch (nmpc_batch_run_path): segs
        float64 [B][S][16] (the nmpc_path_segment layout, nmpc_nav_control_amd.path.pack_paths), nseg int32
        [B], nearest_u float64 [B]; traj_out [N+1][3][B] receives the poses."""
        B = self._batch_of(pose)
        stride = _segs_stride(segs, B)
        check(lib().nmpc_batch_run_path(
            self._h, B, _ptr(pose, F32, (3, B), "pose"), _ptr(vel, F32, (3, B), "vel"),
            _ptr(steer, F32, (B,), "steer"), _ptr(segs, torch.float64, None, "segs"), stride,
            _ptr(nseg, I32, (B,), "nseg"), _ptr(nearest_u, torch.float64, (B,), "nearest_u"), float(sample_period),
            1 if is_holonomic else 0, _ptr(reset, U8, (B,), "reset"),
            _ptr(traj_out, F32, (self.N + 1, 3, B), "traj_out"),
            *self._outputs(B, cmd, u0, status, qp_iter, qp_res, stream)), "nmpc_batch_run_path")

    def follow_path(self, pose, vel, segs, nseg, path_u, sample_period, is_holonomic=False, max_pos_err=float("inf"),
                    max_ori_err=float("inf"), steer=None, reset=None, err=None, off_path=None, traj_out=None, cmd=None,
                    u0=None, status=None, qp_iter=None, qp_res=None, stream=None):
        """The whole FollowPath tick on the device (nmpc_batch_follow_path): nearest path point, getNextNPoses +
        run from it, path-error check. path_u float64 [B] is read as the lower bound of the search (the robot's
        progress so far; 0 on a new path) and overwritten with nearest_u; err float64 [2][B] receives
        {pos_error_to_path, ori_error_to_path}, off_path uint8 [B] the robots whose error reached max_pos_err /
        max_ori_err (their cmd is zeroed; inf or NaN: no check). Everything else as run_path."""
        B = self._batch_of(pose)
        stride = _segs_stride(segs, B)
        check(lib().nmpc_batch_follow_path(
            self._h, B, _ptr(pose, F32, (3, B), "pose"), _ptr(vel, F32, (3, B), "vel"),
            _ptr(steer, F32, (B,), "steer"), _ptr(segs, torch.float64, None, "segs"), stride,
            _ptr(nseg, I32, (B,), "nseg"), _ptr(path_u, torch.float64, (B,), "path_u"), float(sample_period),
            1 if is_holonomic else 0, float(max_pos_err), float(max_ori_err), _ptr(reset, U8, (B,), "reset"),
            _ptr(err, torch.float64, (2, B), "err"), _ptr(off_path, U8, (B,), "off_path"),
            _ptr(traj_out, F32, (self.N + 1, 3, B), "traj_out"),
            *self._outputs(B, cmd, u0, status, qp_iter, qp_res, stream)), "nmpc_batch_follow_path")

    def node_tick(self, node_params, mode, pose, vel, goal=None, segs=None, nseg=None, path_u=None, steer=None,
                  reset=None, event=None, err=None, traj_out=None, n_solved=None, cmd=None, u0=None, status=None,
                  qp_iter=None, qp_res=None, stream=None):
        """One tick of the node's state machine for B robots, each in its own state (nmpc_batch_node_tick): mode
        uint8 [B] in/out (NODE_*), goal float32 [3][B] for the GOTO_POSE robots, segs / nseg / path_u as follow_path
        for the FOLLOW_PATH ones (each group may be None when no robot is in that mode), reset uint8 [B] in/out the
        pending controller resets (consumed by the robots that solve). event uint8 [B] receives NODE_EV_*, err
        float64 [2][B] the path errors (NaN for the others), traj_out the references of the solving robots (NaN for
        the others), n_solved int32 [1] their count. Robots that do not solve keep their resident state bit for bit
        and get zero outputs. node_params: a NodeParams."""
        B = self._batch_of(pose)
        stride = _segs_stride(segs, B) if segs is not None else 1
        check(lib().nmpc_batch_node_tick(
            self._h, B, ctypes.byref(node_params.c), _ptr(mode, torch.uint8, (B,), "mode"),
            _ptr(pose, F32, (3, B), "pose"), _ptr(vel, F32, (3, B), "vel"), _ptr(steer, F32, (B,), "steer"),
            _ptr(goal, F32, (3, B), "goal"), _ptr(segs, torch.float64, None, "segs"), stride,
            _ptr(nseg, I32, (B,), "nseg"), _ptr(path_u, torch.float64, (B,), "path_u"),
            _ptr(reset, torch.uint8, (B,), "reset"), _ptr(event, torch.uint8, (B,), "event"),
            _ptr(err, torch.float64, (2, B), "err"), _ptr(traj_out, F32, (self.N + 1, 3, B), "traj_out"),
            _ptr(n_solved, I32, (1,), "n_solved"), *self._outputs(B, cmd, u0, status, qp_iter, qp_res, stream)),
            "nmpc_batch_node_tick")

    def node_tick_queue(self, node_params, queue, mode, pose, vel, goal=None, steer=None, reset=None, event=None,
                        err=None, traj_out=None, n_solved=None, cmd=None, u0=None, status=None, qp_iter=None,
                        qp_res=None, stream=None):
        """node_tick with each robot's path-set queue on the device (nmpc_batch_node_tick_queue). queue: a
        nmpc_nav_control_amd.path.PathQueue, which owns segs, npart, head, tail and path_u (and frame, length and
        remains when it was built with them); the tick pops the parts behind each FOLLOW_PATH robot, extends its
        active window, and at the end of a part hops to the next queued one (event NODE_EV_NEXT_PART). Everything
        else as node_tick."""
        B = self._batch_of(pose)
        if queue.B != B:
            raise ValueError(f"queue: built for {queue.B} robots, the tick has {B}")
        check(lib().nmpc_batch_node_tick_queue(
            self._h, B, ctypes.byref(node_params.c), ctypes.byref(queue.struct()),
            _ptr(mode, torch.uint8, (B,), "mode"), _ptr(pose, F32, (3, B), "pose"), _ptr(vel, F32, (3, B), "vel"),
            _ptr(steer, F32, (B,), "steer"), _ptr(goal, F32, (3, B), "goal"),
            _ptr(queue.segs, torch.float64, (B, queue.S, 16), "segs"), queue.S,
            _ptr(queue.path_u, torch.float64, (B,), "path_u"), _ptr(reset, torch.uint8, (B,), "reset"),
            _ptr(event, torch.uint8, (B,), "event"), _ptr(err, torch.float64, (2, B), "err"),
            _ptr(traj_out, F32, (self.N + 1, 3, B), "traj_out"), _ptr(n_solved, I32, (1,), "n_solved"),
            *self._outputs(B, cmd, u0, status, qp_iter, qp_res, stream)), "nmpc_batch_node_tick_queue")

    def enable_input(self, depth):
        """Allocate the node's input state (nmpc_batch_enable_input): a ring of `depth` localisation samples per robot
        (2 <= depth <= 64) and the held pose, velocity and steering angle, all 0. The same depth again is a no-op."""
        check(lib().nmpc_batch_enable_input(self._h, int(depth)), "nmpc_batch_enable_input")

    def input_state(self):
        """Views of the input state (nmpc_batch_input_state), or None while it is off: dict with depth, stamp int64
        [depth][cap], sample float64 [depth*3][cap] (slot-major, then x, y, yaw), count and newest int32 [1][cap], held
        float64 [7][cap] (x, y, theta, v, vn, w, steer)."""
        ptrs = [ctypes.c_void_p() for _ in range(5)]
        depth, stride = ctypes.c_int(), ctypes.c_int()
        check(lib().nmpc_batch_input_state(self._h, *[ctypes.byref(p) for p in ptrs], ctypes.byref(depth),
                                           ctypes.byref(stride)), "nmpc_batch_input_state")
        if not depth.value:
            return None
        D, S = depth.value, stride.value
        shapes = (("stamp", (D, S), I64), ("sample", (3 * D, S), F64), ("count", (1, S), I32), ("newest", (1, S), I32),
                  ("held", (7, S), F64))
        out = {k: _DeviceView(p.value, shape, self.device, dt) for p, (k, shape, dt) in zip(ptrs, shapes)}
        out["depth"] = D
        return out

    def push_samples(self, stamp_ns, sample, mask=None, dropped=None, stream=None):
        """The listener (nmpc_batch_push_samples): stamp_ns int64 [B] nanoseconds, sample float64 [3][B] {x, y, yaw} in
        map coordinates; mask uint8 [B] selects the robots (None: all). A sample whose stamp is not after the robot's
        newest one, or that is not finite, is dropped: dropped uint8 [B] (optional) receives 1 there."""
        B = self._batch_of(sample)
        check(lib().nmpc_batch_push_samples(self._h, B, _ptr(stamp_ns, I64, (B,), "stamp_ns"),
                                            _ptr(sample, F64, (3, B), "sample"), _ptr(mask, U8, (B,), "mask"),
                                            _ptr(dropped, torch.uint8, (B,), "dropped"), _stream(stream)),
              "nmpc_batch_push_samples")

    def node_input(self, node_input, mode, goal_map=None, goal_out=None, stream=None):
        """The node's input stage, getInputData (nmpc_batch_node_input), for the robots of mode uint8 [B]: pose with
        the heading hack, finite-difference velocity and data ages from the sample rings into the held values, the
        optional recentre, and the float32 frame values of node_input.pose / vel / steer_out / valid (a NodeInput);
        goal_map float64 [3][B] becomes goal_out float32 [3][B] in the robots' frames."""
        B = self._batch_of(mode, 0)
        check(lib().nmpc_batch_node_input(self._h, B, ctypes.byref(node_input.struct(B)),
                                          _ptr(mode, torch.uint8, (B,), "mode"), _ptr(goal_map, F64, (3, B), "goal_map"),
                                          _ptr(goal_out, F32, (3, B), "goal_out"), _stream(stream)),
              "nmpc_batch_node_input")

    def node_cycle(self, node_params, node_input, mode, goal_map=None, segs=None, nseg=None, path_u=None, queue=None,
                   reset=None, event=None, err=None, traj_out=None, n_solved=None, cmd=None, u0=None, status=None,
                   qp_iter=None, qp_res=None, stream=None):
        """The whole control cycle in one call (nmpc_batch_node_cycle): node_input's stage, then node_tick (or, with
        queue, a nmpc_nav_control_amd.path.PathQueue, node_tick_queue) on the stage's outputs, then the status rule
        for the robots whose input data were invalid (node_input.strict). goal_map float64 [3][B] in map coordinates;
        everything else as node_tick / node_tick_queue."""
        B = self._batch_of(mode, 0)
        if queue is not None:
            if queue.B != B:
                raise ValueError(f"queue: built for {queue.B} robots, the cycle has {B}")
            segs, path_u, stride, q = queue.segs, queue.path_u, queue.S, ctypes.byref(queue.struct())
        else:
            stride, q = (_segs_stride(segs, B) if segs is not None else 1), None
        check(lib().nmpc_batch_node_cycle(
            self._h, B, ctypes.byref(node_params.c), q, ctypes.byref(node_input.struct(B)),
            _ptr(mode, torch.uint8, (B,), "mode"), _ptr(goal_map, F64, (3, B), "goal_map"),
            _ptr(segs, torch.float64, None, "segs"), stride, _ptr(nseg, I32, (B,), "nseg"),
            _ptr(path_u, torch.float64, (B,), "path_u"), _ptr(reset, torch.uint8, (B,), "reset"),
            _ptr(event, torch.uint8, (B,), "event"), _ptr(err, torch.float64, (2, B), "err"),
            _ptr(traj_out, F32, (self.N + 1, 3, B), "traj_out"), _ptr(n_solved, I32, (1,), "n_solved"),
            *self._outputs(B, cmd, u0, status, qp_iter, qp_res, stream)), "nmpc_batch_node_cycle")

    def fleet_sim_step(self, path, s, pose, vel, steer, u0, status, traj, traj_len, advance=True, stream=None):
        B = self._batch_of(pose)
        check(lib().nmpc_fleet_sim_step(
            self._h, B, _ptr(path, F32, (6, B), "path"), _ptr(s, F32, (B,), "s"), _ptr(pose, F32, (3, B), "pose"),
            _ptr(vel, F32, (3, B), "vel"), _ptr(steer, F32, (B,), "steer"), _ptr(u0, F32, (self.nu, B), "u0"),
            _ptr(status, I32, (B,), "status"), _ptr(traj, F32, (self.N + 1, 3, B), "traj"),
            _ptr(traj_len, I32, (B,), "traj_len"), int(bool(advance)), _stream(stream)), "nmpc_fleet_sim_step")


    def fleet_sim_step_renew(self, path, s, pose, vel, steer, u0, status, traj, traj_len, ev, ttl, reset, seed, start,
                             renew, stream=None, stats=None):
        """fleet_sim_step (advance) followed by the stationary loop's goal / path renewal (nmpc_fleet_sim_step_renew):
        ev, ttl int32 [B] in/out, reset uint8 [B] in (the flags the last solve ran with) / out (the next run's reset
        mask); renew: scenario.RENEW keys + kappa_max, speed (lo, hi). stats (optional): dict of device tensors the
        same launch accumulates the last solve's statistics into (nmpc_fleet_stats): qp_iter int32 [B] (in),
        iters_sum int64 [B], iters_max int32 [B], fail_cnt int64 [B], hist int64 [64], cold_cnt / cold_iters
        int64 [B]."""
        B = self._batch_of(pose)
        S = None
        if stats is not None:
            S = FleetStats(qp_iter=_ptr(stats["qp_iter"], I32, (B,), "qp_iter"),
                           iters_sum=_ptr(stats["iters_sum"], I64, (B,), "iters_sum"),
                           iters_max=_ptr(stats["iters_max"], I32, (B,), "iters_max"),
                           fail_cnt=_ptr(stats["fail_cnt"], I64, (B,), "fail_cnt"),
                           hist=_ptr(stats["hist"], I64, (64,), "hist"),
                           cold_cnt=_ptr(stats["cold_cnt"], I64, (B,), "cold_cnt"),
                           cold_iters=_ptr(stats["cold_iters"], I64, (B,), "cold_iters"))
        R = FleetRenew(seed=int(seed) & 0xFFFFFFFF, start=int(start), ttl_min=int(renew["ttl_min"]),
                       ttl_max=int(renew["ttl_max"]), goal_r_lo=renew["goal_r_lo"], goal_r_hi=renew["goal_r_hi"],
                       kappa_max=renew["kappa_max"], speed_lo=renew["speed"][0], speed_hi=renew["speed"][1],
                       len_lo=renew["len_lo"], len_hi=renew["len_hi"], pos_tol=renew["pos_tol"],
                       ang_tol=renew["ang_tol"], ev=_ptr(ev, I32, (B,), "ev"), ttl=_ptr(ttl, I32, (B,), "ttl"),
                       reset=_ptr(reset, U8, (B,), "reset"),
                       stats=ctypes.cast(ctypes.pointer(S), ctypes.c_void_p) if S is not None else None)
        check(lib().nmpc_fleet_sim_step_renew(
            self._h, B, _ptr(path, F32, (6, B), "path"), _ptr(s, F32, (B,), "s"), _ptr(pose, F32, (3, B), "pose"),
            _ptr(vel, F32, (3, B), "vel"), _ptr(steer, F32, (B,), "steer"), _ptr(u0, F32, (self.nu, B), "u0"),
            _ptr(status, I32, (B,), "status"), _ptr(traj, F32, (self.N + 1, 3, B), "traj"),
            _ptr(traj_len, I32, (B,), "traj_len"), ctypes.byref(R), _stream(stream)), "nmpc_fleet_sim_step_renew")


class _DeviceView:
    """Copy helpers for device memory owned by the library (no torch tensor aliases it)."""

    def __init__(self, addr, shape, device, dtype=torch.float32):
        self.addr, self.shape, self.device, self.dtype = addr, shape, device, dtype
        self.itemsize = torch.empty(0, dtype=dtype).element_size()

    def to_tensor(self):
        rows, S = self.shape
        out = torch.empty(rows, S, dtype=self.dtype, device=self.device)
        _memcpy(out.data_ptr(), self.addr, rows * S * self.itemsize)
        return out

    def copy_from(self, t):
        rows, S = self.shape
        t = t.to(device=self.device, dtype=self.dtype).contiguous()
        assert t.numel() == rows * S
        _memcpy(self.addr, t.data_ptr(), rows * S * self.itemsize)


def _memcpy(dst, src, nbytes):
    torch.cuda.synchronize()
    hip = _hip()
    rc = hip.hipMemcpy(ctypes.c_void_p(dst), ctypes.c_void_p(src), ctypes.c_size_t(nbytes), 3)  # DeviceToDevice
    if rc != 0:
        raise RuntimeError(f"hipMemcpy failed ({rc})")


_hip_lib = None


def _hip():
    global _hip_lib
    if _hip_lib is None:
        lib()  # libnmpc_amd pulls in libamdhip64
        _hip_lib = ctypes.CDLL("libamdhip64.so", mode=ctypes.RTLD_GLOBAL)
        _hip_lib.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    return _hip_lib


__all__ = ["BatchSolver", "ModelParams", "NodeInput", "NodeParams", "SepGuard", "SpeedMap", "Tracks", "default_params"]
