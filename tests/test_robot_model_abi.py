"""CPU checks of the model-table ABI (nmpc_batch_set_robot_model and its companions): the calls that need no GPU. The
writer runs the checks that need no handle before it looks at the handle."""
import ctypes
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest

from nmpc_nav_control_amd import _lib
from nmpc_nav_control_amd.scenario import PARAMS
from tests import robot_model_cases as mc

NEW = ["nmpc_batch_set_robot_model", "nmpc_batch_robot_model", "nmpc_batch_clear_robot_model"]
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
    assert re.search(r"int nmpc_batch_set_robot_model\(nmpc_batch\* b, int B, const float\* p, const unsigned char\* "
                     r"mask,\s*void\* stream\);", text)
    assert re.search(r"int nmpc_batch_robot_model\(nmpc_batch\* b, float\*\* table, int\* rows, int\* stride\);", text)
    assert re.search(r"int nmpc_batch_clear_robot_model\(nmpc_batch\* b\);", text)
    assert len(L.nmpc_batch_set_robot_model.argtypes) == 5
    assert len(L.nmpc_batch_robot_model.argtypes) == 4
    assert len(L.nmpc_batch_clear_robot_model.argtypes) == 1


def test_argument_errors(built):
    L = _lib.lib()
    buf = (ctypes.c_float * 8)()
    ptr = ctypes.cast(buf, ctypes.c_void_p)
    cases = {
        "B out of range": lambda: L.nmpc_batch_set_robot_model(None, -1, ptr, None, None),
        "p is NULL": lambda: L.nmpc_batch_set_robot_model(None, 4, None, None, None),
        "batch is NULL": lambda: L.nmpc_batch_set_robot_model(None, 4, ptr, None, None),
    }
    for msg, call in cases.items():
        assert call() == -1, msg  # NMPC_ERR_ARG
        assert msg.encode() in L.nmpc_last_error(), (msg, L.nmpc_last_error())
    assert L.nmpc_batch_robot_model(None, None, None, None) == -1 and b"batch is NULL" in L.nmpc_last_error()
    assert L.nmpc_batch_clear_robot_model(None) == -1 and b"batch is NULL" in L.nmpc_last_error()


@pytest.mark.parametrize("model", ["diff", "omni4", "tric"])
def test_rule_changes_every_parameter_of_most_robots(built, model):
    """the shared rule of the GPU tests: fp32 values, positive, every parameter differs from the handle's on at least
    half of nine robots, and the four robots of each full wave hold four different columns"""
    N, B = 20, 9
    Pm, H = mc.robot_model(model, N, B), mc.handle_model(model, N, B)
    assert Pm.shape == H.shape == (B, mc.NP[model]) == (B, _lib.model_dims(model)["np"])
    assert np.allclose(H[0], PARAMS[model][:mc.NP[model]])
    assert (Pm == Pm.astype(np.float32)).all() and (Pm > 0).all()
    assert ((Pm != H).sum(axis=0) >= B // 2).all()
    for w in (0, 4):
        assert len({tuple(r) for r in Pm[w:w + 4]}) == 4
    for j in range(Pm.shape[1]):
        rv = mc.robot_model(model, N, B, revert=j)
        assert (rv[:, j] == H[:, j]).all() and (np.delete(rv, j, 1) == np.delete(Pm, j, 1)).all()


def test_team_asm_header_is_regenerated_by_its_generator():
    """tools/gen_team_asm.py regenerates the committed csrc/team_asm_gen.hpp byte for byte"""
    spec = importlib.util.spec_from_file_location("gen_team_asm", os.path.join(ROOT, "tools", "gen_team_asm.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    with open(gen.OUT) as fh:
        assert fh.read() == gen.generate()
