"""The C ABI of the block solve drivers (amg_pcg_solve_block,
amg_stationary_solve_block): both are declared, exported and bound, and every
argument error that needs no live handle comes back as AMG_ERR_INVALID before a
device is touched (the checks that need an operator -- leading dimensions, DIM,
UNSUPPORTED -- are in tests/test_gpu_block_solve.py)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "faer-amg_amd", "libfaer_amg_amd.so")
HDR = os.path.join(ROOT, "include", "amg.h")
NEW = ("amg_pcg_solve_block", "amg_stationary_solve_block")
OK, INVALID = 0, 1


def fa():
    import faer_amg_amd
    return faer_amg_amd


def test_block_solve_symbols_declared_exported_and_bound():
    src = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    declared = set(re.findall(r"\b(amg_[a-z0-9_]+)\s*\(", src))
    exported = set(re.findall(r" T (amg_\w+)", subprocess.check_output(["nm", "-D", "--defined-only", LIB]).decode()))
    for name in NEW:
        assert name in declared, name
        assert name in exported, name
        assert name in fa().SIGNATURES, name
    assert callable(fa().pcg_solve_block) and callable(fa().stationary_solve_block)


def test_block_solve_arguments_rejected_without_a_device():
    L = fa().lib()
    b = np.zeros((10, 4), order="F")
    x = np.zeros((10, 4), order="F")
    hist = np.zeros((5, 4), order="F")
    it = np.zeros(4, np.int64)
    pb, px, ph, pi = (a.ctypes.data_as(C.c_void_p) for a in (b, x, hist, it))

    def pcg(B=pb, ldb=10, X=px, ldx=10, k=4, max_iter=5, hist=ph, ldh=5, iters=pi):
        return L.amg_pcg_solve_block(None, None, B, ldb, X, ldx, k, max_iter, 1e-8, 0.0, hist, ldh, iters)

    def stat(B=pb, ldb=10, X=px, ldx=10, k=4, max_iter=5, hist=ph, ldh=5, iters=pi):
        return L.amg_stationary_solve_block(None, None, B, ldb, X, ldx, k, max_iter, 1e-8, hist, ldh, iters)

    for f in (pcg, stat):
        for bad in (dict(B=None), dict(X=None), dict(iters=None)):
            assert f(**bad) == INVALID, bad
            assert b"null B, X or iters" in L.amg_last_error()
        assert f(k=-1) == INVALID
        assert b"negative column count" in L.amg_last_error()
        assert f(max_iter=-1) == INVALID
        assert b"max_iter" in L.amg_last_error()
        assert f(ldh=4) == INVALID
        assert b"ld_hist" in L.amg_last_error()
        assert f(X=pb) == INVALID
        assert b"alias" in L.amg_last_error()
        # a leading dimension below the rows cannot be told without the operator:
        # with a null handle the call fails all the same
        assert f(ldx=-1) == INVALID
        # everything valid (hist may be null; k = 0 too): the null handle is what is wrong
        for good in (dict(), dict(hist=None, ldh=0), dict(k=0)):
            assert f(**good) == INVALID, good
            assert b"null amg_linop" in L.amg_last_error()
    # max_iter = 0 is a PCG call (amg_pcg_solve takes it), not a stationary one
    assert pcg(max_iter=0) == INVALID and b"null amg_linop" in L.amg_last_error()
    assert stat(max_iter=0) == INVALID and b"max_iter must be positive" in L.amg_last_error()
    assert not b.any() and not x.any() and not hist.any() and not it.any()
