"""The C ABI of the device SA setup (amg_set_sa_setup, amg_get_sa_setup,
amg_strength_graph_device, amg_aggregate_mis_device): declared, exported and bound;
the policy's default and range; and the argument errors that need no live operator
come back as AMG_ERR_INVALID before a device is touched (on a machine without a GPU
a touched device answers AMG_ERR_HIP instead).  What the functions compute:
tests/test_gpu_sa_device.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "faer-amg_amd", "libfaer_amg_amd.so")
HDR = os.path.join(ROOT, "include", "amg.h")
NEW = ("amg_set_sa_setup", "amg_get_sa_setup", "amg_strength_graph_device", "amg_aggregate_mis_device")
OK, INVALID = 0, 1


def fa():
    import faer_amg_amd
    return faer_amg_amd


def test_sa_device_symbols_declared_exported_and_bound():
    src = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    declared = set(re.findall(r"\b(amg_[a-z0-9_]+)\s*\(", src))
    exported = set(re.findall(r" T (amg_\w+)", subprocess.check_output(["nm", "-D", "--defined-only", LIB]).decode()))
    for name in NEW:
        assert name in declared, name
        assert name in exported, name
        assert name in fa().SIGNATURES, name
    for name in ("set_sa_setup", "get_sa_setup", "strength_graph_device", "aggregate_mis_device"):
        assert callable(getattr(fa(), name)), name


def test_sa_setup_policy_default_and_range():
    F = fa()
    L = F.lib()
    v = C.c_int32(-7)
    assert L.amg_get_sa_setup(C.byref(v)) == OK and v.value == 0  # the host, by default
    assert F.get_sa_setup() == 0
    assert L.amg_get_sa_setup(None) == INVALID
    assert b"null output" in L.amg_last_error()
    try:
        for bad in (2, -1):
            assert L.amg_set_sa_setup(bad) == INVALID
            assert b"policy must be 0" in L.amg_last_error()
            assert F.get_sa_setup() == 0  # a refused value changes nothing
        assert L.amg_set_sa_setup(1) == OK and F.get_sa_setup() == 1
        F.set_sa_setup("host")
        assert F.get_sa_setup() == 0
        F.set_sa_setup("device")
        assert F.get_sa_setup() == 1
    finally:
        assert L.amg_set_sa_setup(0) == OK
    assert F.get_sa_setup() == 0


def test_sa_config_keeps_its_layout():
    """The policy is process-wide because amg_sa_config has no slot left: 64 bytes, as before."""
    assert C.sizeof(fa().SaConfig()) == 64
    assert C.sizeof(fa().AdaptiveConfig()) == 80


def test_sa_device_arguments_rejected_without_a_device():
    L = fa().lib()
    out = C.c_void_p()
    nn = np.ones(4)
    w = np.ones(1)
    pnn, pw = nn.ctypes.data_as(C.c_void_p), w.ctypes.data_as(C.c_void_p)
    # a null A
    assert L.amg_strength_graph_device(None, pnn, 4, 1, pw, 1, 0, C.byref(out)) == INVALID
    assert b"null amg_linop" in L.amg_last_error()
    # a null out comes first: nothing about A is looked at
    assert L.amg_strength_graph_device(None, pnn, 4, 1, pw, 1, 0, None) == INVALID
    assert b"null output" in L.amg_last_error()
    assert out.value is None
    agg = np.full(4, -3, np.int64)
    info = np.full(4, -3, np.int64)
    na = C.c_int64(-3)
    pagg, pinfo = agg.ctypes.data_as(C.c_void_p), info.ctypes.data_as(C.c_void_p)
    assert L.amg_aggregate_mis_device(None, 0, pagg, C.byref(na), pinfo) == INVALID
    assert b"null amg_linop" in L.amg_last_error()
    assert L.amg_aggregate_mis_device(None, 0, pagg, C.byref(na), None) == INVALID  # info4 is optional
    assert b"null amg_linop" in L.amg_last_error()
    assert L.amg_aggregate_mis_device(None, 0, None, C.byref(na), pinfo) == INVALID
    assert b"null output" in L.amg_last_error()
    assert L.amg_aggregate_mis_device(None, 0, pagg, None, pinfo) == INVALID
    assert b"null output" in L.amg_last_error()
    assert (agg == -3).all() and (info == -3).all() and na.value == -3
