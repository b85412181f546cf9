"""The C ABI of the Chebyshev smoother (amg_chebyshev_config_default,
amg_chebyshev_create, amg_chebyshev_info): declared, exported and bound; the
defaults; and the argument errors that need no live operator come back as
AMG_ERR_INVALID before a device is touched (on a machine without a GPU a touched
device answers AMG_ERR_HIP instead).  The config values out of range, the shape
and the diagonal checks need a live operator: tests/test_gpu_chebyshev.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "faer-amg_amd", "libfaer_amg_amd.so")
HDR = os.path.join(ROOT, "include", "amg.h")
NEW = ("amg_chebyshev_config_default", "amg_chebyshev_create", "amg_chebyshev_info")
OK, INVALID = 0, 1


def fa():
    import faer_amg_amd
    return faer_amg_amd


def test_chebyshev_symbols_declared_exported_and_bound():
    src = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    declared = set(re.findall(r"\b(amg_[a-z0-9_]+)\s*\(", src))
    exported = set(re.findall(r" T (amg_\w+)", subprocess.check_output(["nm", "-D", "--defined-only", LIB]).decode()))
    for name in NEW:
        assert name in declared, name
        assert name in exported, name
        assert name in fa().SIGNATURES, name
    assert re.search(r"AMG_KIND_CHEBYSHEV\s*=\s*9\b", src)
    assert fa().KINDS[9] == "chebyshev" and fa().SMOOTHERS["chebyshev"] == 4
    assert callable(fa().new_chebyshev) and callable(fa().chebyshev_info)


def test_chebyshev_config_default():
    F = fa()
    cfg = F.ChebyshevConfig()
    assert (cfg.steps, cfg.eig_iters, cfg.eig_ratio, cfg.boost, cfg.lambda_max) == (2, 10, 20.0, 1.1, 0.0)
    assert C.sizeof(cfg) == 40  # two int64 and three doubles, no padding
    assert F.lib().amg_chebyshev_config_default(None) == INVALID
    assert b"null" in F.lib().amg_last_error()


def test_sa_config_carries_chebyshev_steps_in_the_reserved_slot():
    """amg_sa_config keeps its layout: chebyshev_steps is the int32 after smoother, 0 by default."""
    F = fa()
    cfg = F.SaConfig()
    assert C.sizeof(cfg) == 64 and F.SaConfig.chebyshev_steps.offset == 60 and F.SaConfig.smoother.offset == 56
    assert cfg.chebyshev_steps == 0 and cfg.smoother == 1
    assert F.SaConfig(smoother="chebyshev", chebyshev_steps=3).smoother == 4
    assert F.AdaptiveConfig(smoother=4, chebyshev_steps=3).sa.chebyshev_steps == 3


def test_chebyshev_arguments_rejected_without_a_device():
    F = fa()
    L = F.lib()
    out = C.c_void_p()
    cfg = F.ChebyshevConfig()
    info = np.full(6, -3.0)
    pinfo = info.ctypes.data_as(C.c_void_p)
    # a null A, with and without a config
    assert L.amg_chebyshev_create(None, None, C.byref(out)) == INVALID
    assert b"null amg_linop" in L.amg_last_error()
    assert L.amg_chebyshev_create(None, C.byref(cfg), C.byref(out)) == INVALID
    assert b"null amg_linop" in L.amg_last_error()
    # a null out comes first: nothing about A is looked at
    assert L.amg_chebyshev_create(None, None, None) == INVALID
    assert b"null output" in L.amg_last_error()
    assert out.value is None
    assert L.amg_chebyshev_info(None, pinfo) == INVALID
    assert b"null amg_linop" in L.amg_last_error()
    assert L.amg_chebyshev_info(None, None) == INVALID
    assert b"null output" in L.amg_last_error()
    assert (info == -3.0).all()
