"""The C ABI of the device strength graph at BFS depth > 1 (amg_pattern_ball_device,
amg_strength_graph_device_depth, amg_sa_level_info): declared, exported and bound;
the Python wrappers; and the argument errors that need no live operator come back as
AMG_ERR_INVALID before a device is touched (on a machine without a GPU a touched
device answers AMG_ERR_HIP instead).  What the functions compute:
tests/test_gpu_sa_depth.py."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "faer-amg_amd", "libfaer_amg_amd.so")
HDR = os.path.join(ROOT, "include", "amg.h")
NEW = ("amg_pattern_ball_device", "amg_strength_graph_device_depth", "amg_sa_level_info")
OK, INVALID = 0, 1


def fa():
    import faer_amg_amd
    return faer_amg_amd


def test_sa_depth_symbols_declared_exported_and_bound():
    src = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    declared = set(re.findall(r"\b(amg_[a-z0-9_]+)\s*\(", src))
    exported = set(re.findall(r" T (amg_\w+)", subprocess.check_output(["nm", "-D", "--defined-only", LIB]).decode()))
    for name in NEW:
        assert name in declared, name
        assert name in exported, name
        assert name in fa().SIGNATURES, name
    assert "amg_strength_graph_device" in declared and "amg_strength_graph_device" in exported  # stays: depth 1


def test_sa_depth_python_wrappers():
    F = fa()
    assert callable(F.pattern_ball_device)
    assert callable(F.Multigrid.sa_level_info)
    p = inspect.signature(F.strength_graph_device).parameters
    assert list(p)[:3] == ["A", "near_null", "weights"]
    assert p["block_size"].default == 1 and p["depth"].default == 1
    assert p["max_bytes"].default == 0 and p["info"].default is False
    assert "any strength depth" in " ".join(F.set_sa_setup.__doc__.split())


def test_pattern_ball_arguments_rejected_without_a_device():
    L = fa().lib()
    out = C.c_void_p()
    # a null out comes first: nothing about A is looked at
    assert L.amg_pattern_ball_device(None, 2, None) == INVALID
    assert b"null output" in L.amg_last_error()
    for depth in (0, -3):
        assert L.amg_pattern_ball_device(None, depth, C.byref(out)) == INVALID
        assert b"depth must be >= 1" in L.amg_last_error()
    assert L.amg_pattern_ball_device(None, 2, C.byref(out)) == INVALID
    assert b"null amg_linop" in L.amg_last_error()
    assert out.value is None


def test_strength_graph_depth_arguments_rejected_without_a_device():
    L = fa().lib()
    out = C.c_void_p()
    nn = np.ones(4)
    w = np.ones(1)
    info = np.full(6, -3, np.int64)
    pnn, pw, pinfo = nn.ctypes.data_as(C.c_void_p), w.ctypes.data_as(C.c_void_p), info.ctypes.data_as(C.c_void_p)
    f = L.amg_strength_graph_device_depth
    assert f(None, pnn, 4, 1, pw, 2, 1, 0, 0, None, pinfo) == INVALID
    assert b"null output" in L.amg_last_error()
    for depth in (0, -1):
        assert f(None, pnn, 4, 1, pw, depth, 1, 0, 0, C.byref(out), pinfo) == INVALID
        assert b"depth must be >= 1" in L.amg_last_error()
    assert f(None, pnn, 4, 1, pw, 2, 1, 0, -1, C.byref(out), pinfo) == INVALID
    assert b"byte budget" in L.amg_last_error()
    assert f(None, pnn, 4, 1, pw, 2, 1, 0, 0, C.byref(out), pinfo) == INVALID
    assert b"null amg_linop" in L.amg_last_error()
    assert f(None, pnn, 4, 1, pw, 2, 1, 0, 0, C.byref(out), None) == INVALID  # info6 is optional
    assert b"null amg_linop" in L.amg_last_error()
    assert out.value is None and (info == -3).all()


def test_sa_level_info_arguments_rejected_without_a_device():
    L = fa().lib()
    out = np.full(8, -3, np.int64)
    pout = out.ctypes.data_as(C.c_void_p)
    assert L.amg_sa_level_info(None, 0, None) == INVALID
    assert b"null output" in L.amg_last_error()
    assert L.amg_sa_level_info(None, -1, pout) == INVALID
    assert b"level out of range" in L.amg_last_error()
    assert L.amg_sa_level_info(None, 0, pout) == INVALID
    assert b"null amg_linop" in L.amg_last_error()
    assert (out == -3).all()
