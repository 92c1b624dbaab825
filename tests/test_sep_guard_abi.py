"""Checks of the separation guard's ABI (nmpc_sep_guard, nmpc_batch_stage_limits_from_tracks_ex, nmpc_batch_sep_hold,
nmpc_batch_set_sep_guard, nmpc_batch_sep_state). The payload checks run before the handle is looked at and need no GPU;
the checks that need a handle are marked gpu."""
import ctypes
import re
import subprocess

import numpy as np
import pytest

from nmpc_nav_control_amd import _lib
from tests.test_separation_abi import good_tracks, sep
from tests.test_speed_map_abi import header

NEW = ["nmpc_sep_guard_default", "nmpc_batch_stage_limits_from_tracks_ex", "nmpc_batch_sep_hold",
       "nmpc_batch_set_sep_guard", "nmpc_batch_sep_state"]


def guard(**kw):
    g = _lib.SepGuardStruct(priority=None, own_priority=None, stop_gap=0.45, release_gap=0.55, hold_stages=4, hold=1)
    for k, v in kw.items():
        setattr(g, k, v)
    return g


def test_symbols_are_declared_exported_and_bound(built):
    text = header()
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True,
                              check=True).stdout
    L = _lib.lib()
    for s in NEW:
        assert s in _lib.BATCH_SYMBOLS
        assert re.search(rf"\bint {s}\(", text), s
        assert re.search(rf" T {s}$", exported, re.M), s
    assert len(L.nmpc_batch_stage_limits_from_tracks_ex.argtypes) == 14
    assert len(L.nmpc_batch_sep_hold.argtypes) == 7
    assert len(L.nmpc_batch_set_sep_guard.argtypes) == 2
    assert re.search(r"#define NMPC_NODE_EV_HELD \(9\)", text) and _lib.NODE_EV_HELD == 9
    # the existing writer's declaration is unchanged
    assert len(L.nmpc_batch_stage_limits_from_tracks.argtypes) == 12


def test_mirror_follows_the_header(built):
    body = re.search(r"typedef struct nmpc_sep_guard \{(.*?)\} nmpc_sep_guard;", header(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    decls = [re.match(r"(const int\*|float|int)\s+(\w+)$", d.strip()) for d in body.split(";") if d.strip()]
    assert all(decls)
    types = {"const int*": ctypes.c_void_p, "float": ctypes.c_float, "int": ctypes.c_int}
    assert [(m.group(2), types[m.group(1)]) for m in decls] == list(_lib.SepGuardStruct._fields_)
    off = [getattr(_lib.SepGuardStruct, n).offset for n, _ in _lib.SepGuardStruct._fields_]
    assert off == [0, 8, 16, 20, 24, 28] and ctypes.sizeof(_lib.SepGuardStruct) == 32  # LP64


def test_defaults(built):
    L = _lib.lib()
    n = ctypes.sizeof(_lib.SepGuardStruct)
    buf = (ctypes.c_ubyte * (n + 16))(*([0xAB] * (n + 16)))
    g = _lib.SepGuardStruct.from_buffer(buf)
    assert L.nmpc_sep_guard_default(ctypes.byref(g)) == 0
    f = lambda v: ctypes.c_float(v).value  # noqa: E731
    assert (g.priority, g.own_priority, g.stop_gap, g.release_gap, g.hold_stages, g.hold) == \
        (None, None, f(0.45), f(0.55), 4, 1)
    assert bytes(buf[n:]) == b"\xab" * 16  # (the library writes the struct and nothing past it)
    assert L.nmpc_sep_guard_default(None) == -1 and b"separation guard is NULL" in L.nmpc_last_error()


def test_argument_errors(built):
    """every argument error that needs no device, each with its message; the payload first, then the handle"""
    L = _lib.lib()
    ptr = ctypes.cast((ctypes.c_ubyte * 64)(), ctypes.c_void_p)
    ref = lambda x: ctypes.byref(x) if x is not None else None  # noqa: E731
    inf, nan = float("inf"), float("nan")

    def writer(g, tr=None, r=None, B=4, pose=ptr, reset=None, gap_all=None):
        tr = good_tracks(own_first=0) if tr is None else tr
        return L.nmpc_batch_stage_limits_from_tracks_ex(None, B, ref(tr), ref(r), ref(g), None, None, pose, reset, None,
                                                        None, None, gap_all, None)

    def hold(g, B=4):
        return L.nmpc_batch_sep_hold(None, B, ref(g), None, None, None, None)

    def attach(g):
        return L.nmpc_batch_set_sep_guard(None, ref(g))

    payload = [("stop_gap must be finite and > 0", dict(stop_gap=0.0)),
               ("stop_gap must be finite and > 0", dict(stop_gap=-0.1)),
               ("stop_gap must be finite and > 0", dict(stop_gap=nan)),
               ("stop_gap must be finite and > 0", dict(stop_gap=inf, release_gap=inf)),
               ("release_gap must be finite and >= stop_gap", dict(release_gap=0.44)),
               ("release_gap must be finite and >= stop_gap", dict(release_gap=nan)),
               ("release_gap must be finite and >= stop_gap", dict(release_gap=inf)),
               ("hold_stages must be >= 0", dict(hold_stages=-1))]
    for call in (writer, hold, attach):
        for msg, kw in payload:
            assert call(guard(**kw)) == -1, (call.__name__, msg)  # NMPC_ERR_ARG
            assert msg.encode() in L.nmpc_last_error(), (call.__name__, msg, L.nmpc_last_error())
        assert call(guard(release_gap=0.45, hold_stages=0, hold=0)) == -1 and b"batch is NULL" in L.nmpc_last_error()
    # release_gap against the rule's range: the writer knows the rule
    assert writer(guard(release_gap=3.5)) == -1 and b"release_gap must be <= range" in L.nmpc_last_error()
    assert writer(guard(release_gap=1.1), r=sep(range=1.0)) == -1 and b"release_gap must be <= range" in L.nmpc_last_error()
    assert writer(guard(release_gap=1.0), r=sep(range=1.0)) == -1 and b"batch is NULL" in L.nmpc_last_error()
    # priority without own_priority reads priority[own_first + i]
    assert writer(guard(priority=ptr), tr=good_tracks()) == -1
    assert b"priority without own_priority needs own_first >= 0" in L.nmpc_last_error()
    assert writer(guard(priority=ptr, own_priority=ptr), tr=good_tracks()) == -1 and b"batch is NULL" in L.nmpc_last_error()
    assert writer(guard(priority=ptr)) == -1 and b"batch is NULL" in L.nmpc_last_error()
    # the existing writer's own checks, in its order, before the guard's
    assert writer(guard(stop_gap=0.0), tr=good_tracks(M=-1)) == -1 and b"M must be >= 0" in L.nmpc_last_error()
    assert writer(guard(stop_gap=0.0), r=sep(gain=0.0)) == -1 and b"gain must be finite" in L.nmpc_last_error()
    assert writer(guard(), B=-1) == -1 and b"B out of range" in L.nmpc_last_error()
    assert writer(guard(), tr=good_tracks(own_first=5)) == -1 and b"own_first + B exceeds M" in L.nmpc_last_error()
    assert writer(guard(), pose=None, reset=ptr) == -1 and b"reset needs pose" in L.nmpc_last_error()
    assert writer(guard(), pose=None) == -1 and b"pose is required" in L.nmpc_last_error()
    assert writer(None, gap_all=ptr) == -1 and b"gap_all needs a guard" in L.nmpc_last_error()
    assert writer(None, pose=None) == -1 and b"batch is NULL" in L.nmpc_last_error()  # (no guard: the plain writer)
    assert hold(None) == -1 and b"separation guard is NULL" in L.nmpc_last_error()
    assert hold(guard(), B=-1) == -1 and b"B out of range" in L.nmpc_last_error()
    assert attach(None) == -1 and b"batch is NULL" in L.nmpc_last_error()  # (detach: the handle is all it needs)
    assert L.nmpc_batch_sep_state(None, None) == -1 and b"batch is NULL" in L.nmpc_last_error()


def test_header_states_the_contract(built):
    text = " ".join(re.sub(r"\n \*", "\n", header()).split())
    for phrase in ("priority[j] >= own_i", "gap_k = sqrtf(qy_k)", "gapa_k = sqrtf(qa_k)", "qy_k == qa_k",
                   "gets INT_MAX: that is the caller's duty", "Priorities are meant for crossings",
                   "gives a convoy one priority", "\"stands\" is reset || held and \"has no direction\" is reset",
                   "held' = reset[i] ? 0 : (held ? m < release_gap : m < stop_gap)",
                   "m = min over k = 0..min(hold_stages, N) of gapa_k", "A reset robot is never held",
                   "is judged from the next cycle on", "The hold never writes reset", "it is state",
                   "A guard without tracks attached is inert", "allocates nothing", "deadlock resolution",
                   "zeroes its carried speed refs", "keep creeping", "with the separation guard below attached they stop"):
        assert phrase in text, phrase


# ---- on a handle ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_hold_needs_a_guarded_writer_call_and_attach_starts_from_zero(built):
    import torch

    from nmpc_nav_control_amd.batch import BatchSolver, SepGuard, Tracks
    dev = torch.device("cuda:0")
    B, N = 4, 20
    s = BatchSolver("diff", N, B, device=dev)
    g = SepGuard()
    with pytest.raises(RuntimeError, match="no nmpc_batch_stage_limits_from_tracks_ex call"):
        s.sep_hold(g)
    assert s.stage_bounds() is None
    assert not s.sep_state().to_tensor().any()
    # every robot stands (reset is not given, the iterate is the initial one) 0.3 m from a static track: held
    xy = torch.zeros(1, 2, 1, dtype=torch.float64, device=dev)
    xy[0, 0, 0] = 0.3
    pose = torch.zeros(3, B, device=dev)
    s.state()[0].copy_from(torch.zeros((N + 1) * s.nx, B, device=dev))
    tr = Tracks(xy)
    s.stage_limits_from_tracks(tr, pose=pose, guard=g)  # (before any attach: the call brings its scratch)
    out = torch.full((B,), 7, dtype=torch.uint8, device=dev)
    s.sep_hold(g, held_out=out)
    torch.cuda.synchronize()
    assert out.tolist() == [1] * B and s.sep_state().to_tensor()[0].tolist() == [1] * B
    s.set_sep_guard(g)  # attach clears
    assert not s.sep_state().to_tensor().any()
    s.sep_hold(g)
    torch.cuda.synchronize()
    assert s.sep_state().to_tensor().all()
    s.set_sep_guard(None)  # detach clears
    assert not s.sep_state().to_tensor().any()
    s.sep_hold(g)
    torch.cuda.synchronize()
    assert s.sep_state().to_tensor().all()
    s.set_sep_guard(g)  # attach again starts from held == 0
    assert not s.sep_state().to_tensor().any()
    with pytest.raises(RuntimeError, match="release_gap must be <= range"):
        s.stage_limits_from_tracks(tr, pose=pose, guard=g, range=0.5, clearance=0.1)
    assert np.isfinite(s.stage_bounds().to_tensor().cpu().numpy().view(np.float32)).all()
