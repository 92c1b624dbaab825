"""CPU checks of the speed map ABI (nmpc_speed_map, nmpc_speed_rule, nmpc_batch_stage_limits_from_map,
nmpc_batch_set_speed_map): the calls that need no GPU. The payload checks run before the handle is looked at."""
import ctypes
import math
import os
import re
import subprocess

import pytest

from nmpc_nav_control_amd import _lib
from nmpc_nav_control_amd.batch import BatchSolver

NEW = ["nmpc_speed_map_default", "nmpc_speed_rule_default", "nmpc_batch_stage_limits_from_map",
       "nmpc_batch_set_speed_map"]
C_TYPES = {"double": ctypes.c_double, "int": ctypes.c_int, "float": ctypes.c_float, "const float*": ctypes.c_void_p}


def header():
    return open(os.path.join(os.path.dirname(_lib._HERE), "include", "nmpc_amd", "nmpc_batch.h")).read()


def c_fields(name):
    """(type, name) of every member of a struct, from the header's own text"""
    body = re.search(rf"typedef struct {name} \{{(.*?)\}} {name};", header(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for decl in body.split(";"):
        m = re.match(r"\s*(const float\*|double|int|float)\s+(.+)$", decl.strip(), re.S)
        if m:
            out += [(m.group(1), n.strip()) for n in m.group(2).split(",")]
    return out


def test_symbols_are_declared_exported_and_bound(built):
    text = header()
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True,
                              check=True).stdout
    L = _lib.lib()
    for s in NEW:
        assert s in _lib.BATCH_SYMBOLS
        assert re.search(rf"\bint {s}\(", text), s
        assert re.search(rf" T {s}$", exported, re.M), s
    assert len(L.nmpc_batch_stage_limits_from_map.argtypes) == 9
    assert len(L.nmpc_batch_set_speed_map.argtypes) == 3


@pytest.mark.parametrize("name,mirror,size", [("nmpc_speed_map", _lib.SpeedMapStruct, 48),
                                              ("nmpc_speed_rule", _lib.SpeedRuleStruct, 8)])
def test_mirrors_follow_the_header(built, name, mirror, size):
    """field order and types from the header's text; offsets and size by the C rules for them (LP64): x0 y0 res at 0,
    8, 16; w h at 24, 28; vmax at 32; outside at 40, padded to 48"""
    fields = c_fields(name)
    assert [n for _, n in fields] == [n for n, _ in mirror._fields_]
    off = 0
    for (ctype, n), (_, py) in zip(fields, mirror._fields_):
        assert py is C_TYPES[ctype], n
        al = ctypes.alignment(py)
        off = (off + al - 1) // al * al
        assert getattr(mirror, n).offset == off, n
        off += ctypes.sizeof(py)
    assert ctypes.sizeof(mirror) == size


def test_defaults(built):
    L = _lib.lib()
    n = ctypes.sizeof(_lib.SpeedMapStruct)
    buf = (ctypes.c_ubyte * (n + 16))(*([0xAB] * (n + 16)))
    m = _lib.SpeedMapStruct.from_buffer(buf)
    assert L.nmpc_speed_map_default(ctypes.byref(m)) == 0
    assert (m.x0, m.y0, m.res, m.w, m.h, m.vmax) == (0.0, 0.0, 0.0, 0, 0, None)
    assert math.isinf(m.outside) and m.outside > 0
    assert bytes(buf[n:]) == b"\xab" * 16  # (the library writes the struct and nothing past it)
    r = _lib.SpeedRuleStruct()
    assert L.nmpc_speed_rule_default(ctypes.byref(r)) == 0
    assert r.slope == ctypes.c_float(0.8).value and r.v_floor == ctypes.c_float(0.05).value
    assert L.nmpc_speed_map_default(None) == -1 and b"speed map is NULL" in L.nmpc_last_error()
    assert L.nmpc_speed_rule_default(None) == -1 and b"speed rule is NULL" in L.nmpc_last_error()


def good_map():
    buf = (ctypes.c_float * 8)()
    m = _lib.SpeedMapStruct(x0=0.0, y0=0.0, res=0.5, w=4, h=2, vmax=ctypes.cast(buf, ctypes.c_void_p),
                            outside=float("inf"))
    m._keep = buf
    return m


def test_argument_errors(built):
    """every argument error that needs no device, each with its message; the payload first, then the handle"""
    L = _lib.lib()
    ptr = ctypes.cast((ctypes.c_ubyte * 64)(), ctypes.c_void_p)

    def writer(m, r=None, B=4, pose=None, reset=None):
        return L.nmpc_batch_stage_limits_from_map(None, B, ctypes.byref(m) if m is not None else None,
                                                  ctypes.byref(r) if r is not None else None, pose, reset, None, None,
                                                  None)

    def attach(m, r=None):
        return L.nmpc_batch_set_speed_map(None, ctypes.byref(m) if m is not None else None,
                                          ctypes.byref(r) if r is not None else None)

    def changed(**kw):
        m = good_map()
        for k, v in kw.items():
            setattr(m, k, v)
        return m

    rule = lambda s, f: _lib.SpeedRuleStruct(slope=s, v_floor=f)  # noqa: E731
    payload = [
        ("res must be finite and > 0", changed(res=0.0), None),
        ("res must be finite and > 0", changed(res=-0.25), None),
        ("res must be finite and > 0", changed(res=float("inf")), None),
        ("res must be finite and > 0", changed(res=float("nan")), None),
        ("w and h must be >= 1", changed(w=0), None),
        ("w and h must be >= 1", changed(h=0), None),
        ("vmax is NULL", changed(vmax=None), None),
        ("slope must be in (0, 1]", good_map(), rule(0.0, 0.05)),
        ("slope must be in (0, 1]", good_map(), rule(1.5, 0.05)),
        ("slope must be in (0, 1]", good_map(), rule(float("nan"), 0.05)),
        ("v_floor must be > 0", good_map(), rule(0.8, 0.0)),
        ("v_floor must be > 0", good_map(), rule(0.8, -1.0)),
    ]
    for call in (writer, attach):
        for msg, m, r in payload:
            assert call(m, r) == -1, (call.__name__, msg)  # NMPC_ERR_ARG
            assert msg.encode() in L.nmpc_last_error(), (call.__name__, msg, L.nmpc_last_error())
    assert writer(None) == -1 and b"speed map is NULL" in L.nmpc_last_error()
    assert writer(good_map(), B=-1) == -1 and b"B out of range" in L.nmpc_last_error()
    assert writer(good_map(), reset=ptr) == -1 and b"reset needs pose" in L.nmpc_last_error()
    assert writer(good_map(), pose=ptr, reset=ptr) == -1 and b"batch is NULL" in L.nmpc_last_error()
    assert writer(good_map(), rule(1.0, 0.05)) == -1 and b"batch is NULL" in L.nmpc_last_error()  # slope 1 is allowed
    assert attach(good_map()) == -1 and b"batch is NULL" in L.nmpc_last_error()
    assert attach(None) == -1 and b"batch is NULL" in L.nmpc_last_error()  # (detach: the handle is all it needs)


def test_header_states_the_duties_and_the_scope(built):
    text = " ".join(re.sub(r"\n \*", "\n", header()).split())  # (the comment's line breaks and its margin)
    for phrase in ("must be flagged in reset", "configuration, not state", "Out of scope: rotated or per-robot maps",
                   "allocates no stage table", "floor((X - x0) / res)"):
        assert phrase in text, phrase


def test_python_wrapper_refuses_reset_without_pose():
    s = BatchSolver.__new__(BatchSolver)  # (no handle: the check comes before the library call)
    s.N, s.capacity = 20, 4
    with pytest.raises(ValueError, match="reset needs pose"):
        s.stage_limits_from_map(None, reset=object())
    s._h = None
