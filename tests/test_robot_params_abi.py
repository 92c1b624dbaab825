"""CPU checks of the per-robot parameter ABI (nmpc_robot_params, nmpc_batch_set_robot_params and its companions): the
calls that need no GPU. The writers run the checks that need no handle before they look at the handle."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from nmpc_nav_control_amd import _lib
from nmpc_nav_control_amd.batch import BatchSolver
from tests import robot_param_cases as rc

NEW = ["nmpc_batch_set_robot_params", "nmpc_batch_set_robot_limits", "nmpc_batch_robot_params",
       "nmpc_batch_clear_robot_params"]


def header():
    return open(os.path.join(os.path.dirname(_lib._HERE), "include", "nmpc_amd", "nmpc_batch.h")).read()


def test_struct_layout_follows_the_header(built):
    """field order and types from the header's own text, offsets and size by the C rules for them (LP64)"""
    body = re.search(r"typedef struct nmpc_robot_params \{(.*?)\} nmpc_robot_params;", header(), re.S).group(1)
    fields = re.findall(r"^\s*(const float\*)\s+(\w+);", body, re.M)
    assert [n for _, n in fields] == [n for n, _ in _lib.RobotParamsStruct._fields_] == list(rc.FIELDS)
    for k, (name, py) in enumerate(_lib.RobotParamsStruct._fields_):
        assert py is ctypes.c_void_p and getattr(_lib.RobotParamsStruct, name).offset == 8 * k, name
    assert ctypes.sizeof(_lib.RobotParamsStruct) == 48


def test_symbols_are_declared_exported_and_bound(built):
    text = header()
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True,
                              check=True).stdout
    L = _lib.lib()
    for s in NEW:
        assert s in _lib.BATCH_SYMBOLS
        assert re.search(rf"\bint {s}\(", text), s
        assert re.search(rf" T {s}$", exported, re.M), s
    assert len(L.nmpc_batch_set_robot_params.argtypes) == 5
    assert len(L.nmpc_batch_set_robot_limits.argtypes) == 9
    assert len(L.nmpc_batch_robot_params.argtypes) == 4
    assert len(L.nmpc_batch_clear_robot_params.argtypes) == 1


def test_argument_errors(built):
    L = _lib.lib()
    buf = (ctypes.c_float * 8)()
    ptr = ctypes.cast(buf, ctypes.c_void_p)
    some = _lib.RobotParamsStruct(W=ptr)
    none = _lib.RobotParamsStruct()
    cases = {
        "B out of range": lambda: L.nmpc_batch_set_robot_params(None, -1, ctypes.byref(some), None, None),
        "robot params is NULL": lambda: L.nmpc_batch_set_robot_params(None, 4, None, None, None),
        "every field is NULL": lambda: L.nmpc_batch_set_robot_params(None, 4, ctypes.byref(none), None, None),
        "batch is NULL": lambda: L.nmpc_batch_set_robot_params(None, 4, ctypes.byref(some), None, None),
    }
    for msg, call in cases.items():
        assert call() == -1, msg  # NMPC_ERR_ARG
        assert msg.encode() in L.nmpc_last_error(), (msg, L.nmpc_last_error())
    lim = lambda B, v: L.nmpc_batch_set_robot_limits(None, B, v, None, None, None, None, None, None)  # noqa: E731
    assert lim(-1, ptr) == -1 and b"B out of range" in L.nmpc_last_error()
    assert lim(4, None) == -1 and b"every array is NULL" in L.nmpc_last_error()
    assert lim(4, ptr) == -1 and b"batch is NULL" in L.nmpc_last_error()
    assert L.nmpc_batch_robot_params(None, None, None, None) == -1 and b"batch is NULL" in L.nmpc_last_error()
    assert L.nmpc_batch_clear_robot_params(None) == -1 and b"batch is NULL" in L.nmpc_last_error()


def test_python_wrappers_refuse_empty_calls():
    s = BatchSolver.__new__(BatchSolver)  # (no handle: the checks come before the library call)
    s.nbx = s.nbu = 2
    s.nx, s.ny, s.capacity = 7, 9, 4
    with pytest.raises(ValueError, match="no field"):
        s.set_robot_params()
    with pytest.raises(ValueError, match="no limit"):
        s.set_robot_limits()
    s._h = None


@pytest.mark.parametrize("model", ["diff", "omni4", "tric"])
def test_rule_keeps_every_start_inside_its_box(built, model):
    """the shared rule of the GPU tests: every robot differs from the handle's parameters, boxes are proper and hold
    the robot's starting reference state, and the input weights stay positive"""
    N, B = 20, 15
    P, H = rc.robot_params(model, N, B), rc.handle_params(model, N, B)
    c = rc.make_fleet(model, B, seed=rc.SEED)["carried"].T.astype(np.float64)
    assert (P["lbx"] < -np.abs(c)).all() and (np.abs(c) < P["ubx"]).all()
    assert (P["lbu"] < 0).all() and (P["ubu"] > 0).all() and (P["W"][:, P["W_e"].shape[1]:] > 0).all()
    differs = np.zeros(B, bool)
    for k in rc.FIELDS:
        assert P[k].shape == H[k].shape and (P[k] == P[k].astype(np.float32)).all()
        differs |= (P[k] != H[k]).any(axis=1)
    assert differs.sum() >= B - 1  # (robot i with every scale 1 is the handle's own set)
