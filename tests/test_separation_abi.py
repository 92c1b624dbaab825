"""CPU checks of the fleet separation ABI (nmpc_tracks, nmpc_sep_rule, nmpc_batch_export_tracks,
nmpc_batch_stage_limits_from_tracks, nmpc_batch_set_tracks): the calls that need no GPU. The payload checks run before
the handle is looked at."""
import ctypes
import re
import subprocess

import pytest

from nmpc_nav_control_amd import _lib
from nmpc_nav_control_amd.batch import BatchSolver
from tests.test_speed_map_abi import good_map, header

NEW = ["nmpc_tracks_default", "nmpc_sep_rule_default", "nmpc_batch_export_tracks",
       "nmpc_batch_stage_limits_from_tracks", "nmpc_batch_set_tracks"]
C_TYPES = {"const double*": ctypes.c_void_p, "int": ctypes.c_int, "float": ctypes.c_float}


def c_fields(name):
    """(type, name) of every member of a struct, from the header's own text"""
    body = re.search(rf"typedef struct {name} \{{(.*?)\}} {name};", header(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for decl in body.split(";"):
        m = re.match(r"\s*(const double\*|int|float)\s+(.+)$", decl.strip(), re.S)
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
    assert len(L.nmpc_batch_export_tracks.argtypes) == 10
    assert len(L.nmpc_batch_stage_limits_from_tracks.argtypes) == 12
    assert len(L.nmpc_batch_set_tracks.argtypes) == 4


@pytest.mark.parametrize("name,mirror,size", [("nmpc_tracks", _lib.TracksStruct, 24),
                                              ("nmpc_sep_rule", _lib.SepRuleStruct, 16)])
def test_mirrors_follow_the_header(built, name, mirror, size):
    """field order and types from the header's text; offsets and size by the C rules for them (LP64): xy at 0, M K
    own_first at 8, 12, 16, padded to 24; four 4-byte members"""
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
    n = ctypes.sizeof(_lib.TracksStruct)
    buf = (ctypes.c_ubyte * (n + 16))(*([0xAB] * (n + 16)))
    tr = _lib.TracksStruct.from_buffer(buf)
    assert L.nmpc_tracks_default(ctypes.byref(tr)) == 0
    assert (tr.xy, tr.M, tr.K, tr.own_first) == (None, 0, 0, -1)
    assert bytes(buf[n:]) == b"\xab" * 16  # (the library writes the struct and nothing past it)
    r = _lib.SepRuleStruct()
    assert L.nmpc_sep_rule_default(ctypes.byref(r)) == 0
    f = lambda v: ctypes.c_float(v).value  # noqa: E731
    assert (r.clearance, r.gain, r.range, r.ahead_only) == (f(0.6), f(1.0), f(3.0), 1)
    assert L.nmpc_tracks_default(None) == -1 and b"tracks is NULL" in L.nmpc_last_error()
    assert L.nmpc_sep_rule_default(None) == -1 and b"separation rule is NULL" in L.nmpc_last_error()


def good_tracks(**kw):
    buf = (ctypes.c_double * 64)()
    tr = _lib.TracksStruct(xy=ctypes.cast(buf, ctypes.c_void_p), M=8, K=3, own_first=-1)
    tr._keep = buf
    for k, v in kw.items():
        setattr(tr, k, v)
    return tr


def sep(clearance=0.6, gain=1.0, range=3.0, ahead_only=1):
    return _lib.SepRuleStruct(clearance=clearance, gain=gain, range=range, ahead_only=ahead_only)


def test_argument_errors(built):
    """every argument error that needs no device, each with its message; the payload first, then the handle"""
    L = _lib.lib()
    ptr = ctypes.cast((ctypes.c_ubyte * 64)(), ctypes.c_void_p)
    ref = lambda x: ctypes.byref(x) if x is not None else None  # noqa: E731

    def writer(tr, r=None, m=None, rule=None, B=4, pose=None, reset=None):
        return L.nmpc_batch_stage_limits_from_tracks(None, B, ref(tr), ref(r), ref(m), ref(rule), pose, reset, None,
                                                     None, None, None)

    def attach(tr, r=None, export_own=0):
        return L.nmpc_batch_set_tracks(None, ref(tr), ref(r), export_own)

    inf, nan = float("inf"), float("nan")
    payload = [
        ("M must be >= 0", good_tracks(M=-1), None),
        ("K must be >= 0", good_tracks(K=-1), None),
        ("xy is NULL", good_tracks(xy=None), None),
        ("own_first must be >= -1", good_tracks(own_first=-2), None),
        ("gain must be finite and > 0", good_tracks(), sep(gain=0.0)),
        ("gain must be finite and > 0", good_tracks(), sep(gain=-1.0)),
        ("gain must be finite and > 0", good_tracks(), sep(gain=inf)),
        ("gain must be finite and > 0", good_tracks(), sep(gain=nan)),
        ("clearance must be finite and >= 0", good_tracks(), sep(clearance=-0.1)),
        ("clearance must be finite and >= 0", good_tracks(), sep(clearance=nan)),
        ("clearance must be finite and >= 0", good_tracks(), sep(clearance=inf)),
        ("range must be finite and > clearance", good_tracks(), sep(range=0.6)),
        ("range must be finite and > clearance", good_tracks(), sep(range=0.5)),
        ("range must be finite and > clearance", good_tracks(), sep(range=inf)),
        ("range must be finite and > clearance", good_tracks(), sep(range=nan)),
    ]
    for call in (writer, attach):
        for msg, tr, r in payload:
            assert call(tr, r) == -1, (call.__name__, msg)  # NMPC_ERR_ARG
            assert msg.encode() in L.nmpc_last_error(), (call.__name__, msg, L.nmpc_last_error())
        assert call(good_tracks(M=0, xy=None), sep(clearance=0.0)) == -1 and b"batch is NULL" in L.nmpc_last_error()
    assert writer(None) == -1 and b"tracks is NULL" in L.nmpc_last_error()
    assert writer(good_tracks(), B=-1) == -1 and b"B out of range" in L.nmpc_last_error()
    assert writer(good_tracks(own_first=5), B=4) == -1 and b"own_first + B exceeds M" in L.nmpc_last_error()
    assert writer(good_tracks(own_first=4), B=4) == -1 and b"batch is NULL" in L.nmpc_last_error()
    # the speed map's payload checks when a map is given, the speed rule's when a rule is given
    bad_map = good_map()
    bad_map.res = 0.0
    assert writer(good_tracks(), m=bad_map) == -1 and b"res must be finite and > 0" in L.nmpc_last_error()
    rule = _lib.SpeedRuleStruct(slope=1.5, v_floor=0.05)
    assert writer(good_tracks(), rule=rule) == -1 and b"slope must be in (0, 1]" in L.nmpc_last_error()
    assert writer(good_tracks(), m=good_map(), rule=rule) == -1 and b"slope must be in (0, 1]" in L.nmpc_last_error()
    assert writer(good_tracks(), reset=ptr) == -1 and b"reset needs pose" in L.nmpc_last_error()
    assert writer(good_tracks(), m=good_map(), pose=ptr, reset=ptr) == -1 and b"batch is NULL" in L.nmpc_last_error()
    assert attach(good_tracks(), export_own=1) == -1 and b"export_own needs own_first >= 0" in L.nmpc_last_error()
    assert attach(good_tracks(own_first=0), export_own=1) == -1 and b"batch is NULL" in L.nmpc_last_error()
    assert attach(None) == -1 and b"batch is NULL" in L.nmpc_last_error()  # (detach: the handle is all it needs)

    def export(B=4, pose=None, reset=None, mode=None, xy=ptr, M=8, K=3, first=0):
        return L.nmpc_batch_export_tracks(None, B, pose, reset, mode, xy, M, K, first, None)

    for kw in (dict(first=-1), dict(first=5), dict(M=3)):
        assert export(**kw) == -1 and b"first out of range" in L.nmpc_last_error(), kw
    assert export(K=-1) == -1 and b"K must be >= 0" in L.nmpc_last_error()
    assert export(xy=None) == -1 and b"xy is NULL" in L.nmpc_last_error()
    assert export(reset=ptr) == -1 and b"reset and mode need pose" in L.nmpc_last_error()
    assert export(mode=ptr) == -1 and b"reset and mode need pose" in L.nmpc_last_error()
    assert export(B=-1) == -1 and b"B out of range" in L.nmpc_last_error()
    assert export(first=4, pose=ptr, reset=ptr, mode=ptr) == -1 and b"batch is NULL" in L.nmpc_last_error()


def test_header_states_the_rule_and_the_scope(built):
    text = " ".join(re.sub(r"\n \*", "\n", header()).split())  # (the comment's line breaks and its margin)
    for phrase in ("h_k = p_{min(k+1, N)} - p_{min(k, N-1)}", "dx = (float)(Tx - X_k)", "q = dx*dx + dy*dy",
                   "q <= range*range", "hx == 0 && hy == 0 or dx*hx + dy*hy > 0", "gap_k = sqrtf(q_k)",
                   "s_k = gain * (gap_k - clearance)", "z_k = fminf(zmap_k, fmaxf(v_floor, s_k))",
                   "zmap_k = fminf(cap, fmaxf(v_floor, m_k))", "kk = min(k, K)",
                   "speed limiting, not collision avoidance", "keep creeping", "No general constraints in the QP",
                   "no change to the solve kernels", "no per-track radii", "no rotated footprints",
                   "not the capsule ABI", "caller-held iterate", "configuration, not state",
                   "no spatial index over the map", "export_own requires own_first >= 0"):
        assert phrase in text, phrase


def test_python_wrapper_refuses_reset_without_pose():
    s = BatchSolver.__new__(BatchSolver)  # (no handle: the check comes before the library call)
    s.N, s.capacity = 20, 4
    with pytest.raises(ValueError, match="reset needs pose"):
        s.stage_limits_from_tracks(None, reset=object())
    with pytest.raises(ValueError, match="reset and mode need pose"):
        s.export_tracks(None, mode=object())
    s._h = None
