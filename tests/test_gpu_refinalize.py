"""Re-finalizing one handle across SpMV storages (csr_finalize, csr.hip).

A handle that amg_csr_set_grid re-finalizes under another format policy must end
in exactly the state of a handle created fresh under that policy: finalize
resets every storage struct of GpuCsr (gpu_csr.hpp) before it builds, so nothing
of the storage the handle had before may show -- not in spmv_info(), not in one
bit of an SpMV.  Each walk leaves a storage and comes back to it.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MODES = ("set", "add", "resid", "jacobi")


def fa():
    import faer_amg_amd
    return faer_amg_amd


def _vectors(n):
    rng = np.random.default_rng(20241)
    return {k: rng.uniform(-1.0, 1.0, n) for k in ("x", "b", "y0")} | {"d": rng.uniform(0.05, 0.3, n)}


def _apply(ctx, A, v, dev):
    import torch
    T = lambda a: torch.tensor(a, dtype=torch.float64, device=dev)  # noqa: E731
    x, b, d = T(v["x"]), T(v["b"]), T(v["d"])
    out = {}
    for mode in MODES:
        y = T(v["y0"])
        A.spmv_epilogue(mode, x, y, b, d)
        ctx.synchronize()
        out[mode] = y
    return out


def _walk(ctx, dev, make, grid, policies, kernels, regrid_fresh, ignore=()):
    """One handle through `policies` (re-finalized by set_grid(*grid) after each
    change) against a handle made fresh under each (and, regrid_fresh, given the
    same hint); the kernel names along the walk must be `kernels`.  `ignore`: keys
    of spmv_info() that two builds of one matrix do not share."""
    import torch
    F = fa()
    seen = []
    try:
        walked = None
        for pol in policies:
            F.set_spmv_format(pol)
            if walked is None:
                walked = make()
            walked.set_grid(*grid)
            fresh = make()
            if regrid_fresh:
                fresh.set_grid(*grid)
            iw, ifr = walked.spmv_info(), fresh.spmv_info()
            seen.append(iw["kernel"])
            print(pol, iw)
            for key in ignore:
                assert (key in iw) == (key in ifr), (pol, key)
                iw.pop(key, None)
                ifr.pop(key, None)
            assert iw == ifr, (pol, iw, ifr)
            n = walked.dims()[0]
            v = _vectors(n)
            yw, yf = _apply(ctx, walked, v, dev), _apply(ctx, fresh, v, dev)
            for mode in MODES:
                assert torch.equal(yw[mode], yf[mode]), (pol, mode)
                assert bool(torch.isfinite(yw[mode]).all()), (pol, mode)
    finally:
        F.set_spmv_format("auto")
        F.set_value_codes(1)
    assert tuple(seen) == tuple(kernels), seen


def test_refinalize_walks_dia_sell_vector_stream(ctx, dev):
    """7-point Laplacian on 64 x 32 x 32 (65536 rows: the smallest at which DIA
    builds) through auto, sell, vector, csr, auto."""
    make = lambda: fa().SparseMatOp.laplace3d_7pt(ctx, 64, 32, 32)  # noqa: E731
    _walk(ctx, dev, make, (64, 32, 32), ("auto", "sell", "vector", "csr", "auto"),
          ("dia", "sell", "vector", "csr-stream", "dia"), regrid_fresh=False)


def test_refinalize_leaves_and_retakes_block_storage(ctx, dev):
    """Q1 elasticity on 8 x 8 x 8 elements (2187 rows): 3x3 blocks, wave-per-row, blocks."""
    H = fa().elasticity_q1((8, 8, 8))
    _walk(ctx, dev, lambda: H.upload(ctx), (0, 0, 0), ("auto", "vector", "auto"), ("bsr", "vector", "bsr"),
          regrid_fresh=True)


def test_refinalize_leaves_and_retakes_pattern_and_class_storage(ctx, dev):
    """27-point anisotropic operator on 16 x 16 x 16 (4096 rows; random7 on 32^3 takes
    plain SELL-64, which the first walk covers).  With its grid hint cleared it takes
    the pattern SELL: left for CSR-stream and taken again, whole spmv_info() equal.

    With the hint it takes the x-staged stencil classes, whose tile on a shape outside
    the frozen table is chosen by timing candidates at every build (scs.hip
    xscs_autotune; it changes the launch shape, not one bit of a result): two builds
    of this matrix reported tiles (8, 8, 1) and (8, 4, 4) in one process, before this
    test's change as after it.  That walk therefore compares everything but `tile`."""
    make = lambda: fa().SparseMatOp.aniso27(ctx, 16, 16, 16)  # noqa: E731
    _walk(ctx, dev, make, (0, 0, 0), ("auto", "csr", "auto"), ("sellp", "csr-stream", "sellp"),
          regrid_fresh=True)
    _walk(ctx, dev, make, (16, 16, 16), ("auto", "csr", "auto"), ("classes", "csr-stream", "classes"),
          regrid_fresh=True, ignore=("tile",))
