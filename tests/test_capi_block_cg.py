"""The C ABI of the coupled block CG (amg_block_cg_solve) and of its two kernel
primitives (amg_block_gram, amg_block_gemm_update): declared, exported and bound,
and every argument error that needs no live handle comes back with its status
before a device is touched (the checks that need an operator are in
tests/test_gpu_block_cg.py)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "faer-amg_amd", "libfaer_amg_amd.so")
HDR = os.path.join(ROOT, "include", "amg.h")
NEW = ("amg_block_cg_solve", "amg_block_gram", "amg_block_gemm_update")
OK, INVALID, DIM, UNSUPPORTED = 0, 1, 2, 3


def fa():
    import faer_amg_amd
    return faer_amg_amd


def test_block_cg_symbols_declared_exported_and_bound():
    src = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    declared = set(re.findall(r"\b(amg_[a-z0-9_]+)\s*\(", src))
    exported = set(re.findall(r" T (amg_\w+)", subprocess.check_output(["nm", "-D", "--defined-only", LIB]).decode()))
    for name in NEW:
        assert name in declared, name
        assert name in exported, name
        assert name in fa().SIGNATURES, name
    F = fa()
    assert callable(F.block_cg_solve) and callable(F.block_gram) and callable(F.block_gemm_update)


def test_block_cg_arguments_rejected_without_a_device():
    L = fa().lib()
    b = np.zeros((10, 4), order="F")
    x = np.zeros((10, 4), order="F")
    hist = np.zeros((5, 4), order="F")
    ranks = np.full(5, -7, np.int64)
    it = np.full(1, -7, np.int64)
    pb, px, ph, pr = (a.ctypes.data_as(C.c_void_p) for a in (b, x, hist, ranks))
    pi = it.ctypes.data_as(C.POINTER(C.c_int64))

    def bcg(B=pb, ldb=10, X=px, ldx=10, k=4, max_iter=5, rank_tol=0.0, hist=ph, ldh=5, ranks=pr, iters=pi):
        return L.amg_block_cg_solve(None, None, B, ldb, X, ldx, k, max_iter, 1e-8, 0.0, rank_tol, hist, ldh, ranks,
                                    iters)

    for bad in (dict(B=None), dict(X=None), dict(iters=None)):
        assert bcg(**bad) == INVALID, bad
        assert b"null B, X or iters" in L.amg_last_error()
    assert bcg(k=-1) == INVALID and b"negative column count" in L.amg_last_error()
    assert bcg(k=33) == UNSUPPORTED and b"32 columns" in L.amg_last_error()
    assert bcg(max_iter=-1) == INVALID and b"max_iter" in L.amg_last_error()
    assert bcg(ldh=4) == INVALID and b"ld_hist" in L.amg_last_error()
    for rt in (1.0, 2.5, float("nan"), float("inf")):
        assert bcg(rank_tol=rt) == INVALID, rt
        assert b"rank_tol" in L.amg_last_error()
    assert bcg(X=pb) == INVALID and b"alias" in L.amg_last_error()
    # the order of the checks: the column count before max_iter, ld_hist, rank_tol and the alias
    assert bcg(k=33, max_iter=-1, ldh=0, rank_tol=2.0, X=pb) == UNSUPPORTED
    assert bcg(k=-1, max_iter=-1) == INVALID and b"negative column count" in L.amg_last_error()
    # everything valid (hist and ranks may be null; k = 0 and k = 32 too; a negative
    # rank_tol is the default): the null handle is what is wrong
    for good in (dict(), dict(hist=None, ldh=0), dict(ranks=None), dict(k=0), dict(k=32), dict(rank_tol=-1.0),
                 dict(rank_tol=0.5), dict(max_iter=0)):
        assert bcg(**good) == INVALID, good
        assert b"null amg_linop" in L.amg_last_error()
    assert not b.any() and not x.any() and not hist.any()
    assert (ranks == -7).all() and (it == -7).all()


def test_block_kernel_primitives_rejected_without_a_device():
    L = fa().lib()
    x = np.zeros((10, 4), order="F")
    y = np.zeros((10, 4), order="F")
    c = np.full((4, 8), 3.25, order="F")
    px, py, pc = (a.ctypes.data_as(C.c_void_p) for a in (x, y, c))

    def gram(X=px, ldx=10, w=4, Y1=py, ld1=10, m1=4, Y2=py, ld2=10, m2=4, n=10, Cm=pc):
        return L.amg_block_gram(None, X, ldx, w, Y1, ld1, m1, Y2, ld2, m2, n, Cm)

    def upd(Y=py, ldy=10, X=px, ldx=10, Cm=pc, w=4, m=4, n=10, sign=1):
        return L.amg_block_gemm_update(None, Y, ldy, X, ldx, Cm, w, m, n, sign)

    for bad in (dict(X=None), dict(Y1=None), dict(Cm=None), dict(w=0), dict(m1=0), dict(m2=-1), dict(n=-1),
                dict(Y2=None), dict(ldx=9), dict(ld1=9), dict(ld2=9)):
        assert gram(**bad) == INVALID, bad
    for bad in (dict(w=33), dict(m1=33), dict(m2=33)):
        assert gram(**bad) == UNSUPPORTED, bad
    for good in (dict(), dict(Y2=None, m2=0, ld2=0), dict(w=32, m1=32, m2=32, n=0, ldx=0, ld1=0, ld2=0)):
        assert gram(**good) == INVALID, good
        assert b"null context" in L.amg_last_error()

    for bad in (dict(Y=None), dict(X=None), dict(Cm=None), dict(w=0), dict(m=0), dict(n=-1), dict(sign=0),
                dict(sign=2), dict(ldx=9), dict(ldy=9)):
        assert upd(**bad) == INVALID, bad
    assert upd(X=py) == INVALID and b"alias" in L.amg_last_error()
    for bad in (dict(w=33), dict(m=33)):
        assert upd(**bad) == UNSUPPORTED, bad
    for good in (dict(), dict(sign=-1)):
        assert upd(**good) == INVALID, good
        assert b"null context" in L.amg_last_error()
    assert not x.any() and not y.any() and (c == 3.25).all()
