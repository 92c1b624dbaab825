"""CPU checks of the node-tick ABI (nmpc_node_params_default, nmpc_batch_node_tick's argument errors): the calls that
need no GPU. nmpc_batch_node_tick runs the checks that need no handle before it looks at the handle, so they are
reachable here, where no handle can be created."""
import ctypes
import math

from nmpc_nav_control_amd import _lib
from tests import node_ref


def tick(L, h, B, np_, mode, segs=None, seg_stride=1):
    return L.nmpc_batch_node_tick(h, B, np_, mode, None, None, None, None, segs, seg_stride, None, None, None, None,
                                  None, None, None, None, None, None, None, None, None)


def test_default_params_are_the_shipped_yaml(built):
    L = _lib.lib()
    p = _lib.NodeParamsStruct()
    assert L.nmpc_node_params_default(ctypes.byref(p)) == 0
    assert p.final_pos_err == 0.01 and p.max_goal_dist == 2.0 and p.max_pos_err == 0.5
    assert p.final_ori_err == 1.0 * math.pi / 180.0 and p.max_ori_err == 60.0 * math.pi / 180.0
    assert p.enable_safe_conditions == 1 and p.final_ori_signed == 1
    assert p.sample_period == 1.0 / 40.0 and p.is_holonomic == 0
    # the oracle's defaults are the same numbers
    for k, v in node_ref.DEFAULT.items():
        assert getattr(p, k) == v, k
    assert L.nmpc_node_params_default(None) == -1 and b"NULL" in L.nmpc_last_error()


def test_constants_follow_the_header(built):
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(_lib._HERE), "include", "nmpc_amd", "nmpc_batch.h")).read()
    got = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define NMPC_(NODE_\w+) (\d+)", hdr)}
    assert len(got) == 12
    import nmpc_nav_control_amd as pkg
    for k, v in got.items():
        assert getattr(_lib, k) == v and getattr(pkg, k) == v and getattr(node_ref, k[5:]) == v, k


def test_argument_errors(built):
    L = _lib.lib()
    p = _lib.NodeParamsStruct()
    L.nmpc_node_params_default(ctypes.byref(p))
    mode = (ctypes.c_ubyte * 4)()
    segs = (ctypes.c_double * 16)()
    ok = ctypes.byref(p)
    vp = lambda a: ctypes.cast(a, ctypes.c_void_p)  # noqa: E731
    cases = {
        "node params": lambda: tick(L, None, 4, None, vp(mode)),
        "B out of range": lambda: tick(L, None, -1, ok, vp(mode)),
        "mode": lambda: tick(L, None, 4, ok, None),
        "seg_stride": lambda: tick(L, None, 4, ok, vp(mode), vp(segs), 0),
        "batch is NULL": lambda: tick(L, None, 4, ok, vp(mode)),
    }
    for msg, call in cases.items():
        assert call() == -1, msg  # NMPC_ERR_ARG
        assert msg.encode() in L.nmpc_last_error(), (msg, L.nmpc_last_error())
    for bad in (math.nan, math.inf, -math.inf, -1.0):
        q = _lib.NodeParamsStruct()
        L.nmpc_node_params_default(ctypes.byref(q))
        q.sample_period = bad
        assert tick(L, None, 4, ctypes.byref(q), vp(mode)) == -1
        assert b"sample_period" in L.nmpc_last_error()
    # a stride is only read with segments
    assert tick(L, None, 4, ok, vp(mode), None, 0) == -1 and b"batch is NULL" in L.nmpc_last_error()


def test_symbols_are_bound(built):
    assert "nmpc_batch_node_tick" in _lib.BATCH_SYMBOLS and "nmpc_node_params_default" in _lib.BATCH_SYMBOLS
    assert len(_lib.lib().nmpc_batch_node_tick.argtypes) == 23
