"""CPU checks of the path-queue ABI (nmpc_path_queue, nmpc_path_queue_default, nmpc_batch_node_tick_queue's argument
errors): the calls that need no GPU. Like nmpc_batch_node_tick, the queue tick runs the checks that need no handle
before it looks at the handle."""
import ctypes
import math
import os
import re

import nmpc_nav_control_amd as pkg
from nmpc_nav_control_amd import _lib
from tests import queue_ref


def header():
    return open(os.path.join(os.path.dirname(_lib._HERE), "include", "nmpc_amd", "nmpc_batch.h")).read()


def tick(L, h, B, np_, q, mode, segs=None, seg_stride=1):
    return L.nmpc_batch_node_tick_queue(h, B, np_, q, mode, None, None, None, None, segs, seg_stride, None, None, None,
                                        None, None, None, None, None, None, None, None, None)


def test_struct_layout_follows_the_header(built):
    """field order and types from the header's own text, offsets and size by the C rules for them (LP64)"""
    body = re.search(r"typedef struct nmpc_path_queue \{(.*?)\} nmpc_path_queue;", header(), re.S).group(1)
    fields = re.findall(r"^\s*(const int\*|int\*|const double\*|double\*|double)\s+(\w+);", body, re.M)
    assert [n for _, n in fields] == [n for n, _ in _lib.PathQueueStruct._fields_]
    off = 0
    for (ctype, name), (_, py) in zip(fields, _lib.PathQueueStruct._fields_):
        assert py is (ctypes.c_double if ctype == "double" else ctypes.c_void_p), name
        assert getattr(_lib.PathQueueStruct, name).offset == off, name
        off += 8
    assert ctypes.sizeof(_lib.PathQueueStruct) == off == 64


def test_defaults(built):
    L = _lib.lib()
    q = _lib.PathQueueStruct(npart=1, head=2, tail=3, frame=4, length=5, remains=6)
    assert L.nmpc_path_queue_default(ctypes.byref(q)) == 0
    assert q.part_length == 1000.0 and q.max_active_len == 5.0
    assert [getattr(q, n) for n in ("npart", "head", "tail", "frame", "length", "remains")] == [None] * 6
    assert queue_ref.QDEFAULT == dict(part_length=q.part_length, max_active_len=q.max_active_len)
    assert L.nmpc_path_queue_default(None) == -1 and b"NULL" in L.nmpc_last_error()


def test_event_constant_follows_the_header(built):
    m = re.search(r"#define NMPC_NODE_EV_NEXT_PART \((\d+)\)", header())
    assert int(m.group(1)) == 7 == _lib.NODE_EV_NEXT_PART == pkg.NODE_EV_NEXT_PART == queue_ref.EV_NEXT_PART


def test_argument_errors(built):
    L = _lib.lib()
    p = _lib.NodeParamsStruct()
    L.nmpc_node_params_default(ctypes.byref(p))
    q = _lib.PathQueueStruct()
    L.nmpc_path_queue_default(ctypes.byref(q))
    mode = (ctypes.c_ubyte * 4)()
    segs = (ctypes.c_double * 16)()
    ints = (ctypes.c_int * 4)()
    vp = lambda a: ctypes.cast(a, ctypes.c_void_p)  # noqa: E731
    ok, okq = ctypes.byref(p), ctypes.byref(q)

    def full():
        f = _lib.PathQueueStruct()
        L.nmpc_path_queue_default(ctypes.byref(f))
        f.npart = f.head = f.tail = ctypes.addressof(ints)
        return f

    fq = full()
    cases = {
        "path queue is NULL": lambda: tick(L, None, 4, ok, None, vp(mode)),
        "node params": lambda: tick(L, None, 4, None, okq, vp(mode)),
        "B out of range": lambda: tick(L, None, -1, ok, okq, vp(mode)),
        "mode": lambda: tick(L, None, 4, ok, okq, None),
        "npart, head and tail": lambda: tick(L, None, 4, ok, okq, vp(mode), vp(segs), 2),
        "seg_stride": lambda: tick(L, None, 4, ok, ctypes.byref(fq), vp(mode), vp(segs), 0),
        "batch is NULL": lambda: tick(L, None, 4, ok, ctypes.byref(fq), vp(mode), vp(segs), 2),
    }
    for msg, call in cases.items():
        assert call() == -1, msg  # NMPC_ERR_ARG
        assert msg.encode() in L.nmpc_last_error(), (msg, L.nmpc_last_error())
    for missing in ("npart", "head", "tail"):
        f = full()
        setattr(f, missing, None)
        assert tick(L, None, 4, ok, ctypes.byref(f), vp(mode), vp(segs), 2) == -1
        assert b"npart, head and tail" in L.nmpc_last_error()
    for field in ("part_length", "max_active_len"):
        for bad in (math.nan, math.inf, -math.inf):
            f = full()
            setattr(f, field, bad)
            assert tick(L, None, 4, ok, ctypes.byref(f), vp(mode)) == -1
            assert b"must be finite" in L.nmpc_last_error()
    # the window arrays are only read with segments
    assert tick(L, None, 4, ok, okq, vp(mode)) == -1 and b"batch is NULL" in L.nmpc_last_error()
    # nmpc_batch_node_tick's own checks still come first in its own order
    p.sample_period = math.nan
    assert tick(L, None, 4, ok, okq, vp(mode)) == -1 and b"sample_period" in L.nmpc_last_error()


def test_symbols_are_bound(built):
    assert "nmpc_batch_node_tick_queue" in _lib.BATCH_SYMBOLS and "nmpc_path_queue_default" in _lib.BATCH_SYMBOLS
    assert len(_lib.lib().nmpc_batch_node_tick_queue.argtypes) == 23
    assert len(_lib.lib().nmpc_batch_node_tick.argtypes) == 23  # (the plain tick's signature is unchanged)
