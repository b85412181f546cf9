"""The C ABI of the numeric re-setup (amg_sa_refresh, amg_sa_level_aggregates,
amg_spgemm_refill, amg_transpose_perm, amg_transpose_refill): declared, exported and
bound; the Python wrappers; and the argument errors that need no live operator come
back as AMG_ERR_INVALID before a device is touched.  What the functions compute:
tests/test_gpu_sa_refresh.py and tests/test_gpu_spgemm_refill.py."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "faer-amg_amd", "libfaer_amg_amd.so")
HDR = os.path.join(ROOT, "include", "amg.h")
NEW = ("amg_sa_refresh", "amg_sa_level_aggregates", "amg_spgemm_refill", "amg_transpose_perm",
       "amg_transpose_refill")
INVALID = 1


def fa():
    import faer_amg_amd
    return faer_amg_amd


def test_refresh_symbols_declared_exported_and_bound():
    src = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    declared = set(re.findall(r"\b(amg_[a-z0-9_]+)\s*\(", src))
    exported = set(re.findall(r" T (amg_\w+)", subprocess.check_output(["nm", "-D", "--defined-only", LIB]).decode()))
    for name in NEW:
        assert name in declared, name
        assert name in exported, name
        assert name in fa().SIGNATURES, name
    # in-place value updates of a handle stay out of the interface: A_new is a second handle
    assert "amg_csr_update_values" not in declared and "amg_csr_update_values" not in exported


def test_refresh_python_wrappers():
    F = fa()
    assert list(inspect.signature(F.Multigrid.refresh).parameters) == ["self", "A_new", "near_null"]
    assert list(inspect.signature(F.Multigrid.sa_aggregates).parameters) == ["self", "level"]
    assert list(inspect.signature(F.spgemm_refill).parameters) == ["A", "B", "C_"]
    assert list(inspect.signature(F.transpose_perm).parameters) == ["P_", "R"]
    assert list(inspect.signature(F.transpose_refill).parameters) == ["P_", "R", "perm"]
    assert "keep the old operators" in " ".join(F.Multigrid.refresh.__doc__.split())


def test_header_documents_aliasing_and_atomicity():
    text = " ".join(open(HDR).read().replace("*", " ").split())  # without the comment frame
    assert "leaves the multigrid exactly as it was" in text
    assert "keep the operators of the hierarchy they were taken from" in text


def test_refresh_arguments_rejected_without_a_device():
    L = fa().lib()
    nn = np.ones(4)
    info = np.full(8, -3, np.int64)
    pnn, pinfo = nn.ctypes.data_as(C.c_void_p), info.ctypes.data_as(C.c_void_p)
    assert L.amg_sa_refresh(None, None, pnn, 4, 1, pinfo) == INVALID
    assert b"null amg_linop" in L.amg_last_error()
    assert L.amg_sa_refresh(None, None, None, 4, 1, None) == INVALID
    assert (info == -3).all()
    agg = np.full(4, -3, np.int64)
    na = C.c_int64(-3)
    assert L.amg_sa_level_aggregates(None, 0, agg.ctypes.data_as(C.c_void_p), C.byref(na)) == INVALID
    assert b"null amg_linop" in L.amg_last_error()
    assert (agg == -3).all() and na.value == -3


def test_refill_arguments_rejected_without_a_device():
    L = fa().lib()
    perm = np.full(4, -3, np.int32)
    pperm = perm.ctypes.data_as(C.c_void_p)
    assert L.amg_spgemm_refill(None, None, None) == INVALID
    assert b"null amg_linop" in L.amg_last_error()
    assert L.amg_transpose_perm(None, None, pperm) == INVALID
    assert b"null amg_linop" in L.amg_last_error()
    assert L.amg_transpose_refill(None, None, pperm) == INVALID
    assert b"null amg_linop" in L.amg_last_error()
    assert (perm == -3).all()
