"""CPU checks of the node input ABI (nmpc_batch_enable_input, _input_state, _push_samples, nmpc_node_input_default,
nmpc_batch_node_input, _node_cycle): the calls that need no GPU. The entry points run the checks that need no handle
before they look at the handle. The two argument errors that need a live handle (a second depth, and a stage or cycle
without enabled state) are in tests/test_gpu_node_input.py::test_argument_errors_on_a_handle."""
import ctypes
import inspect
import math
import os
import re
import subprocess

from nmpc_nav_control_amd import _lib
from nmpc_nav_control_amd.batch import BatchSolver, NodeInput

NEW = ["nmpc_batch_enable_input", "nmpc_batch_input_state", "nmpc_batch_push_samples", "nmpc_node_input_default",
       "nmpc_batch_node_input", "nmpc_batch_node_cycle"]
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
        r"int nmpc_batch_enable_input\(nmpc_batch\* b, int depth\);",
        r"int nmpc_batch_input_state\(nmpc_batch\* b, long long\*\* stamp, double\*\* sample, int\*\* count, "
        r"int\*\* newest, double\*\* held,\s*int\* depth, int\* stride\);",
        r"int nmpc_batch_push_samples\(nmpc_batch\* b, int B, const long long\* stamp_ns, const double\* sample "
        r"/\* \[3\]\[B\] x, y, yaw \*/,\s*const unsigned char\* mask, unsigned char\* dropped /\* \[B\] or NULL \*/, "
        r"void\* stream\);",
        r"int nmpc_node_input_default\(nmpc_node_input\* in\);",
        r"int nmpc_batch_node_input\(nmpc_batch\* b, int B, const nmpc_node_input\* in, const unsigned char\* mode,",
        r"int nmpc_batch_node_cycle\(nmpc_batch\* b, int B, const nmpc_node_params\* np, const nmpc_path_queue\* q",
        r"#define NMPC_NODE_EV_INPUT_INVALID \(8\)",
    ]
    for d in decls:
        assert re.search(d, text), d
    want = dict(zip(NEW, (2, 8, 7, 1, 7, 22)))
    for s, n in want.items():
        assert len(getattr(L, s).argtypes) == n, s
    assert _lib.NODE_EV_INPUT_INVALID == 8
    # the sentence that put getInputData out of scope is gone
    assert "Out of scope for both" not in text and "nmpc_batch_node_input below" in text


def test_node_input_struct_mirrors_the_header_and_its_defaults(built):
    text = header()
    body = re.search(r"typedef struct nmpc_node_input \{(.*?)\} nmpc_node_input;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n.strip(" *") for decl in body.split(";") if decl.strip()
             for n in re.sub(r"^\s*(const\s+)?(unsigned\s+)?(long long|\w+)\s*\**", "", decl.strip()).split(",")]
    assert names == [f for f, _ in _lib.NodeInputStruct._fields_]
    c = _lib.NodeInputStruct()
    c.strict, c.now_ns = 5, 77
    assert _lib.lib().nmpc_node_input_default(ctypes.byref(c)) == 0
    assert (c.now_ns, c.period_ns, c.transform_timeout, c.pose_valid_overwritten, c.strict) == (0, 25000000, 0.1, 1, 0)
    assert c.recentre_radius == math.inf
    assert all(getattr(c, k) is None for k in ("steer", "steer_ok", "valid", "pose", "vel", "steer_out", "moved"))
    n = NodeInput.default(strict=1, recentre_radius=8.0)
    assert n.strict == 1 and n.recentre_radius == 8.0 and n.period_ns == 25000000 and n.pose is None
    try:
        NodeInput.default(nonsense=1)
    except AttributeError:
        pass
    else:
        raise AssertionError("an unknown field was accepted")


def test_argument_errors(built):
    L = _lib.lib()
    buf = (ctypes.c_double * 8)()
    ptr = ctypes.cast(buf, ctypes.c_void_p)
    nin, npar, q = _lib.NodeInputStruct(), _lib.NodeParamsStruct(), _lib.PathQueueStruct()
    L.nmpc_node_input_default(ctypes.byref(nin))
    L.nmpc_node_params_default(ctypes.byref(npar))
    L.nmpc_path_queue_default(ctypes.byref(q))
    rin, rnp, rq = ctypes.byref(nin), ctypes.byref(npar), ctypes.byref(q)
    tail = [None] * 12  # reset .. stream

    def cycle(B, np_, q_, in_, mode):
        return L.nmpc_batch_node_cycle(None, B, np_, q_, in_, mode, None, None, 1, None, None, *tail)

    cases = {
        "B out of range": [lambda: L.nmpc_batch_push_samples(None, -1, ptr, ptr, None, None, None),
                           lambda: L.nmpc_batch_node_input(None, -1, rin, ptr, None, None, None),
                           lambda: cycle(-1, rnp, None, rin, ptr),
                           lambda: cycle(-1, rnp, rq, rin, ptr)],
        "stamp_ns and sample are required": [lambda: L.nmpc_batch_push_samples(None, 4, None, ptr, None, None, None),
                                             lambda: L.nmpc_batch_push_samples(None, 4, ptr, None, None, None, None)],
        "node input is NULL": [lambda: L.nmpc_batch_node_input(None, 4, None, ptr, None, None, None),
                               lambda: cycle(4, rnp, None, None, ptr),
                               lambda: L.nmpc_node_input_default(None)],
        "node params is NULL": [lambda: cycle(4, None, None, rin, ptr)],
        "mode is required": [lambda: L.nmpc_batch_node_input(None, 4, rin, None, None, None, None),
                             lambda: cycle(4, rnp, None, rin, None)],
        "input depth out of range": [lambda: L.nmpc_batch_enable_input(None, 1),
                                     lambda: L.nmpc_batch_enable_input(None, 65),
                                     lambda: L.nmpc_batch_enable_input(None, -3)],
        "batch is NULL": [lambda: L.nmpc_batch_enable_input(None, 4),
                          lambda: L.nmpc_batch_input_state(None, None, None, None, None, None, None, None),
                          lambda: L.nmpc_batch_push_samples(None, 4, ptr, ptr, None, None, None),
                          lambda: L.nmpc_batch_node_input(None, 4, rin, ptr, None, None, None),
                          lambda: cycle(4, rnp, None, rin, ptr),
                          lambda: cycle(4, rnp, rq, rin, ptr)],
    }
    for msg, calls in cases.items():
        for k, call in enumerate(calls):
            assert call() == -1, (msg, k)  # NMPC_ERR_ARG
            assert msg.encode() in L.nmpc_last_error(), (msg, k, L.nmpc_last_error())


def test_python_layer_has_the_input_methods_and_checkpoints_the_state():
    for m in ("enable_input", "input_state", "push_samples", "node_input", "node_cycle"):
        assert callable(getattr(BatchSolver, m)), m
    assert '"node_input"' in inspect.getsource(BatchSolver.save_state)
    src = inspect.getsource(BatchSolver.restore_state)
    assert '"node_input"' in src and "enable_input" in src
