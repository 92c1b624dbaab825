"""CPU checks of the frame-table ABI (nmpc_batch_set_robot_frame and its companions): the calls that need no GPU. The
entry points run the checks that need no handle before they look at the handle."""
import ctypes
import inspect
import os
import re
import subprocess

from nmpc_nav_control_amd import _lib
from nmpc_nav_control_amd.batch import BatchSolver

NEW = ["nmpc_batch_set_robot_frame", "nmpc_batch_recentre", "nmpc_batch_to_frame", "nmpc_batch_from_frame",
       "nmpc_batch_robot_frame", "nmpc_batch_clear_robot_frame"]
ROOT = os.path.dirname(_lib._HERE)


def header():
    return open(os.path.join(ROOT, "include", "nmpc_amd", "nmpc_batch.h")).read()


def test_symbols_are_declared_exported_and_bound(built):
    text = header()
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True,
                              check=True).stdout
    L = _lib.lib()
    for s in NEW:
        assert s in _lib.BATCH_SYMBOLS
        assert re.search(rf"\bint {s}\(", text), s
        assert re.search(rf" T {s}$", exported, re.M), s
    decls = [
        r"int nmpc_batch_set_robot_frame\(nmpc_batch\* b, int B, const double\* origin, const unsigned char\* mask,\s*"
        r"void\* stream\);",
        r"int nmpc_batch_recentre\(nmpc_batch\* b, int B, const double\* pose_map, double radius, "
        r"const unsigned char\* mask,\s*unsigned char\* moved, void\* stream\);",
        r"int nmpc_batch_to_frame\(nmpc_batch\* b, int B, const double\* map, int n, int c, float\* out, "
        r"void\* stream\);",
        r"int nmpc_batch_from_frame\(nmpc_batch\* b, int B, const float\* in, int n, int c, double\* map, "
        r"void\* stream\);",
        r"int nmpc_batch_robot_frame\(nmpc_batch\* b, double\*\* table, int\* stride\);",
        r"int nmpc_batch_clear_robot_frame\(nmpc_batch\* b, void\* stream\);",
    ]
    for d in decls:
        assert re.search(d, text), d
    want = dict(zip(NEW, (5, 7, 7, 7, 3, 2)))
    for s, n in want.items():
        assert len(getattr(L, s).argtypes) == n, s
    assert L.nmpc_batch_recentre.argtypes[3] is ctypes.c_double


def test_argument_errors(built):
    L = _lib.lib()
    buf = (ctypes.c_double * 8)()
    ptr = ctypes.cast(buf, ctypes.c_void_p)
    cases = {
        "B out of range": [lambda: L.nmpc_batch_set_robot_frame(None, -1, ptr, None, None),
                           lambda: L.nmpc_batch_recentre(None, -1, ptr, 1.0, None, None, None),
                           lambda: L.nmpc_batch_to_frame(None, -1, ptr, 1, 3, ptr, None),
                           lambda: L.nmpc_batch_from_frame(None, -1, ptr, 1, 3, ptr, None)],
        "origin is NULL": [lambda: L.nmpc_batch_set_robot_frame(None, 4, None, None, None)],
        "pose_map is NULL": [lambda: L.nmpc_batch_recentre(None, 4, None, 1.0, None, None, None)],
        "n must be >= 0": [lambda: L.nmpc_batch_to_frame(None, 4, ptr, -1, 3, ptr, None),
                           lambda: L.nmpc_batch_from_frame(None, 4, ptr, -1, 3, ptr, None)],
        "c must be >= 2": [lambda: L.nmpc_batch_to_frame(None, 4, ptr, 1, 1, ptr, None),
                           lambda: L.nmpc_batch_from_frame(None, 4, ptr, 1, 1, ptr, None)],
        "arrays are required": [lambda: L.nmpc_batch_to_frame(None, 4, None, 1, 3, ptr, None),
                                lambda: L.nmpc_batch_to_frame(None, 4, ptr, 1, 3, None, None),
                                lambda: L.nmpc_batch_from_frame(None, 4, None, 1, 3, ptr, None),
                                lambda: L.nmpc_batch_from_frame(None, 4, ptr, 1, 3, None, None)],
        "batch is NULL": [lambda: L.nmpc_batch_set_robot_frame(None, 4, ptr, None, None),
                          lambda: L.nmpc_batch_recentre(None, 4, ptr, 1.0, None, None, None),
                          lambda: L.nmpc_batch_recentre(None, 4, ptr, float("nan"), None, None, None),  # (no API error)
                          lambda: L.nmpc_batch_to_frame(None, 4, ptr, 1, 3, ptr, None),
                          lambda: L.nmpc_batch_from_frame(None, 4, ptr, 1, 3, ptr, None),
                          lambda: L.nmpc_batch_robot_frame(None, None, None),
                          lambda: L.nmpc_batch_clear_robot_frame(None, None)],
    }
    for msg, calls in cases.items():
        for k, call in enumerate(calls):
            assert call() == -1, (msg, k)  # NMPC_ERR_ARG
            assert msg.encode() in L.nmpc_last_error(), (msg, k, L.nmpc_last_error())


def test_python_layer_has_the_frame_methods_and_checkpoints_the_table():
    for m in ("set_robot_frame", "recentre", "to_frame", "from_frame", "robot_frame", "clear_robot_frame"):
        assert callable(getattr(BatchSolver, m)), m
    src = inspect.getsource(BatchSolver._tables)
    assert '"robot_frame"' in src
    # the frame table is restored before the iterate that is relative to it
    src = inspect.getsource(BatchSolver.restore_state)
    assert src.index("self._tables()") < src.index("self.state()")
