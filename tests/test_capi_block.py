"""The C ABI of the block V-cycle and the adaptive build: the four new entry
points are declared and exported, flag 11 is bound, and bad arguments come back as
the documented status before a device is touched (the checks that need a live
handle -- a leading dimension below the operator's rows -- are in
tests/test_gpu_block_cycle.py)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "faer-amg_amd", "libfaer_amg_amd.so")
HDR = os.path.join(ROOT, "include", "amg.h")
NEW = ("amg_csr_spmm_epilogue", "amg_multigrid_block_plan", "amg_adaptive_config_default", "amg_adaptive_build")
INVALID, DIM, UNSUPPORTED = 1, 2, 3


def fa():
    import faer_amg_amd
    return faer_amg_amd


def test_new_symbols_declared_exported_and_bound():
    src = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    declared = set(re.findall(r"\b(amg_[a-z0-9_]+)\s*\(", src))
    exported = set(re.findall(r" T (amg_\w+)", subprocess.check_output(["nm", "-D", "--defined-only", LIB]).decode()))
    for name in NEW:
        assert name in declared, name
        assert name in exported, name
        assert name in fa().SIGNATURES, name
    assert "amg_adaptive_config" in src and "max_components" in src and "test_iters" in src
    assert fa().FLAGS["block_cycle"] == 11


def test_adaptive_config_defaults():
    cfg = fa().AdaptiveConfig()
    assert (cfg.max_components, cfg.test_iters) == (5, 50)
    ref = fa().SaConfig()
    for name, _ in fa().SaConfig._fields_:
        assert getattr(cfg.sa, name) == getattr(ref, name), name
    cfg = fa().AdaptiveConfig(max_components=3, test_iters=6, block_size=3, coarsest_dim=60, smoother="jacobi")
    assert (cfg.max_components, cfg.test_iters, cfg.sa.block_size, cfg.sa.coarsest_dim, cfg.sa.smoother) == (3, 6, 3, 60, 0)
    assert fa().lib().amg_adaptive_config_default(None) == INVALID
    try:
        fa().AdaptiveConfig(max_component=3)  # a misspelt option is an error, not ignored
    except TypeError as e:
        assert "max_component" in str(e)
    else:
        raise AssertionError("unknown AdaptiveConfig option accepted")
    assert callable(fa().csr_spmm_epilogue)


def test_block_arguments_rejected_without_a_device():
    L = fa().lib()
    x = np.zeros((70, 65), order="F")
    p = x.ctypes.data_as(C.c_void_p)
    n = C.c_int64()
    out = C.c_void_p()
    cfg = fa().AdaptiveConfig()
    # amg_csr_spmm_epilogue: k < 0, a bad mode, then the null handle
    assert L.amg_csr_spmm_epilogue(None, 0, p, 70, p, 70, None, 0, None, -1) == INVALID
    assert b"negative column count" in L.amg_last_error()
    assert L.amg_csr_spmm_epilogue(None, 4, p, 70, p, 70, None, 0, None, 1) == INVALID
    assert L.amg_csr_spmm_epilogue(None, 0, p, 70, p, 70, None, 0, None, 1) == INVALID
    assert b"null amg_linop" in L.amg_last_error()
    # amg_multigrid_block_plan: k < 1, null count, null handle
    assert L.amg_multigrid_block_plan(None, 0, None, 0, C.byref(n)) == INVALID
    assert b"k >= 1" in L.amg_last_error()
    assert L.amg_multigrid_block_plan(None, 8, None, 0, None) == INVALID
    assert L.amg_multigrid_block_plan(None, 8, None, 0, C.byref(n)) == INVALID
    assert b"null amg_linop" in L.amg_last_error()
    # amg_adaptive_build: dim, config and null arguments, then the null handle
    assert L.amg_adaptive_build(None, p, 70, 65, C.byref(cfg), None, C.byref(out)) == UNSUPPORTED
    assert L.amg_adaptive_build(None, p, 70, 1, C.byref(cfg), None, C.byref(out)) == INVALID
    assert b"dim must be >= 2" in L.amg_last_error()
    bad = fa().AdaptiveConfig(max_components=0)
    assert L.amg_adaptive_build(None, p, 70, 4, C.byref(bad), None, C.byref(out)) == INVALID
    assert b"max_components" in L.amg_last_error()
    assert L.amg_adaptive_build(None, p, 70, 4, None, None, C.byref(out)) == INVALID
    assert L.amg_adaptive_build(None, None, 70, 4, C.byref(cfg), None, C.byref(out)) == INVALID
    assert L.amg_adaptive_build(None, p, 70, 4, C.byref(cfg), None, None) == INVALID
    assert L.amg_adaptive_build(None, p, 70, 4, C.byref(cfg), None, C.byref(out)) == INVALID
    assert b"null amg_linop" in L.amg_last_error()
    # k > 1 through the generic entry points still rejects null handles and k < 0 first
    assert L.amg_linop_apply(None, p, 70, p, 70, 4, 1) == INVALID
    assert L.amg_multigrid_apply(None, p, 70, p, 70, -1, 1) == INVALID
    assert L.amg_precond_apply_in_place(None, p, 70, 4, 1) == INVALID
