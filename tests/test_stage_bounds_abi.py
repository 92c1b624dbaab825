"""CPU checks of the stage-bound ABI (nmpc_stage_bounds, nmpc_batch_set_stage_bounds and its companions): the calls that
need no GPU. The writers run the checks that need no handle before they look at the handle."""
import ctypes
import os
import re
import subprocess

import pytest

from nmpc_nav_control_amd import _lib
from nmpc_nav_control_amd.batch import BatchSolver
from tests import stage_bound_cases as sc

NEW = ["nmpc_batch_set_stage_bounds", "nmpc_batch_set_stage_limits", "nmpc_batch_shift_stage_bounds",
       "nmpc_batch_stage_bounds", "nmpc_batch_clear_stage_bounds"]


def header():
    return open(os.path.join(os.path.dirname(_lib._HERE), "include", "nmpc_amd", "nmpc_batch.h")).read()


def test_struct_layout_follows_the_header(built):
    """field order and types from the header's own text, offsets and size by the C rules for them (LP64)"""
    body = re.search(r"typedef struct nmpc_stage_bounds \{(.*?)\} nmpc_stage_bounds;", header(), re.S).group(1)
    fields = re.findall(r"^\s*(const float\*)\s+(\w+);", body, re.M)
    assert [n for _, n in fields] == [n for n, _ in _lib.StageBoundsStruct._fields_] == list(sc.FIELDS)
    for k, (name, py) in enumerate(_lib.StageBoundsStruct._fields_):
        assert py is ctypes.c_void_p and getattr(_lib.StageBoundsStruct, name).offset == 8 * k, name
    assert ctypes.sizeof(_lib.StageBoundsStruct) == 32


def test_symbols_are_declared_exported_and_bound(built):
    text = header()
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True,
                              check=True).stdout
    L = _lib.lib()
    for s in NEW:
        assert s in _lib.BATCH_SYMBOLS
        assert re.search(rf"\bint {s}\(", text), s
        assert re.search(rf" T {s}$", exported, re.M), s
    assert len(L.nmpc_batch_set_stage_bounds.argtypes) == 5
    assert len(L.nmpc_batch_set_stage_limits.argtypes) == 9
    assert len(L.nmpc_batch_shift_stage_bounds.argtypes) == 5
    assert len(L.nmpc_batch_stage_bounds.argtypes) == 3
    assert len(L.nmpc_batch_clear_stage_bounds.argtypes) == 1


def test_header_states_the_size_and_the_shift_rule(built):
    text = header()
    assert "(N+1) * (2 NBX + 2 NBU) * capacity * 4 bytes" in text and "5.4 MB" in text and "86 MB" in text
    assert (40 + 1) * 8 * 4096 * 4 == 5_373_952 and round((40 + 1) * 8 * 65536 * 4 / 1e6) == 86
    assert "dt_ctrl == dt" in text


def test_argument_errors(built):
    L = _lib.lib()
    buf = (ctypes.c_float * 8)()
    ptr = ctypes.cast(buf, ctypes.c_void_p)
    some = _lib.StageBoundsStruct(ubx=ptr)
    none = _lib.StageBoundsStruct()
    cases = {
        "B out of range": lambda: L.nmpc_batch_set_stage_bounds(None, -1, ctypes.byref(some), None, None),
        "stage bounds is NULL": lambda: L.nmpc_batch_set_stage_bounds(None, 4, None, None, None),
        "every field is NULL": lambda: L.nmpc_batch_set_stage_bounds(None, 4, ctypes.byref(none), None, None),
        "batch is NULL": lambda: L.nmpc_batch_set_stage_bounds(None, 4, ctypes.byref(some), None, None),
    }
    for msg, call in cases.items():
        assert call() == -1, msg  # NMPC_ERR_ARG
        assert msg.encode() in L.nmpc_last_error(), (msg, L.nmpc_last_error())
    lim = lambda B, v: L.nmpc_batch_set_stage_limits(None, B, v, None, None, None, None, None, None)  # noqa: E731
    assert lim(-1, ptr) == -1 and b"B out of range" in L.nmpc_last_error()
    assert lim(4, None) == -1 and b"every array is NULL" in L.nmpc_last_error()
    assert lim(4, ptr) == -1 and b"batch is NULL" in L.nmpc_last_error()
    shift = lambda B, n: L.nmpc_batch_shift_stage_bounds(None, B, n, None, None)  # noqa: E731
    assert shift(-1, 1) == -1 and b"B out of range" in L.nmpc_last_error()
    assert shift(4, -1) == -1 and b"n must be >= 0" in L.nmpc_last_error()
    assert shift(4, 1) == -1 and b"batch is NULL" in L.nmpc_last_error()
    assert L.nmpc_batch_stage_bounds(None, None, None) == -1 and b"batch is NULL" in L.nmpc_last_error()
    assert L.nmpc_batch_clear_stage_bounds(None) == -1 and b"batch is NULL" in L.nmpc_last_error()


def test_python_wrappers_refuse_empty_calls():
    s = BatchSolver.__new__(BatchSolver)  # (no handle: the checks come before the library call)
    s.nbx = s.nbu = 2
    s.N, s.capacity = 20, 4
    with pytest.raises(ValueError, match="no field"):
        s.set_stage_bounds()
    with pytest.raises(ValueError, match="no limit"):
        s.set_stage_limits()
    with pytest.raises(ValueError, match="n must be >= 0"):
        s.shift_stage_bounds(-1)
    s._h = None
