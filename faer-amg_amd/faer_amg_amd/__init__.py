"""Python front end of libfaer_amg_amd.so (the MI355X-native faer-amg V-cycle path).

Mirrors the reference's public surface (aujxn/faer-amg) by name so tests read
like the reference's own usage:

  reference (Rust)                                  here
  SparseMatOp::new (core.rs:56)                     SparseMatOp.from_scipy / from_arrays
  new_jacobi / new_l1 / new_l2 (smoothers.rs:43-86) new_jacobi / new_l1 / new_l2
  SmootherKind::SymGaussSeidel (smoothers.rs:20)    SymGaussSeidel
  CoarseSolverKind::Cholesky (coarse_solvers.rs:29) CoarseCholesky
  Multigrid::new/add_level/with_cycle_type/
      with_smoothing_steps (multigrid.rs:190-239)   Multigrid (same method names)
  LinOp::apply / Precond::apply_in_place            LinOp.apply / LinOp.apply_in_place

Every compute call goes through the C ABI (include/amg.h) into hand-written
HIP kernels; there is no CPU fallback.  If the shared library is missing this
module raises at import time.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_PKG_DIR = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("FAMG_LIB") or os.path.join(os.path.dirname(_PKG_DIR), "libfaer_amg_amd.so")

if not os.path.exists(LIB_PATH):
    raise ImportError(
        f"{LIB_PATH} not found: build the HIP library first "
        "(python -c 'import __graft_entry__ as g; g.build()' or make -C faer-amg_amd)")

_lib = C.CDLL(LIB_PATH)


def source_hash(root=None):
    """sha256[:16] over the library's sources in the Makefile's order (SRCFILES)."""
    import glob
    import hashlib
    root = root or os.path.dirname(_PKG_DIR)
    src = os.path.join(root, "csrc")
    files = []
    for pat in ("*.hip", "*.cpp", "*.hpp", "*.inc"):
        files += sorted(glob.glob(os.path.join(src, pat)))
    files.append(os.path.join(root, "..", "include", "amg.h"))
    h = hashlib.sha256()
    for f in files:
        with open(f, "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


def library_hash():
    f = _lib.amg_source_hash
    f.restype = C.c_char_p
    return f().decode()


# a prebuilt library must match the sources beside it (it travels with the tree
# to the GPU box): a stale one is refused instead of silently running old kernels
if not os.environ.get("FAMG_LIB") and os.path.isdir(os.path.join(os.path.dirname(_PKG_DIR), "csrc")):
    if library_hash() != source_hash():
        raise ImportError(f"{LIB_PATH} was built from other sources (library {library_hash()}, tree "
                          f"{source_hash()}): rebuild with make -C faer-amg_amd")

i32, i64, dbl, vp = C.c_int32, C.c_int64, C.c_double, C.c_void_p
P = C.POINTER

AMG_MEM_HOST, AMG_MEM_DEVICE = 0, 1
KINDS = {0: "csr", 1: "diag", 2: "sgs", 3: "coarse", 4: "multigrid", 5: "dist_csr",
         6: "dist_multigrid", 7: "composite", 8: "block", 9: "chebyshev"}

# name -> (restype, argtypes); every exported symbol of include/amg.h
SIGNATURES = {
    "amg_last_error": (C.c_char_p, []),
    "amg_version": (C.c_char_p, []),
    "amg_ctx_create": (i32, [C.c_int, vp, P(vp)]),
    "amg_ctx_destroy": (i32, [vp]),
    "amg_ctx_synchronize": (i32, [vp]),
    "amg_ctx_stream": (i32, [vp, P(vp)]),
    "amg_set_spmv_format": (i32, [i32]),
    "amg_set_value_codes": (i32, [i32]),
    "amg_set_alloc_policy": (i32, [i32]),
    "amg_ctx_join_stream": (i32, [vp, vp, i32]),
    "amg_csr_create": (i32, [vp, i64, i64, vp, vp, vp, P(vp)]),
    "amg_csr_create_device_i32": (i32, [vp, i64, i64, vp, vp, vp, P(vp)]),
    "amg_csr_nnz": (i32, [vp, P(i64)]),
    "amg_csr_spmv_info": (i32, [vp, vp]),
    "amg_csr_value_codes": (i32, [vp, vp]),
    "amg_csr_download": (i32, [vp, vp, vp, vp]),
    "amg_csr_dia_range": (i32, [vp, vp]),
    "amg_csr_class_info": (i32, [vp, vp]),
    "amg_csr_set_grid": (i32, [vp, i64, i64, i64]),
    "amg_csr_spmv_epilogue": (i32, [vp, i32, vp, vp, vp, vp]),
    "amg_csr_grid_info": (i32, [vp, vp]),
    "amg_csr_row_lanes": (i32, [vp, P(i64)]),
    "amg_grid_from_offsets": (i32, [vp, i64, i64, vp, P(i32)]),
    "amg_set_flag": (i32, [i32, i64]),
    "amg_source_hash": (C.c_char_p, []),
    "amg_multigrid_level_reordered": (i32, [vp, i64, P(i32)]),
    "amg_multigrid_get_run_level": (i32, [vp, i64, P(vp), P(vp), P(vp), P(vp)]),
    "amg_get_flag": (i32, [i32, P(i64)]),
    "amg_gen_laplace3d_7pt": (i32, [vp, i64, i64, i64, P(vp)]),
    "amg_gen_aniso27": (i32, [vp, i64, i64, i64, dbl, dbl, dbl, P(vp)]),
    "amg_gen_random_7pt": (i32, [vp, i64, i64, i64, C.c_uint64, i64, P(vp)]),
    "amg_linop_kind_of": (i32, [vp, P(i32)]),
    "amg_linop_dims": (i32, [vp, P(i64), P(i64)]),
    "amg_linop_apply": (i32, [vp, vp, i64, vp, i64, i64, C.c_int]),
    "amg_linop_transpose_apply": (i32, [vp, vp, i64, vp, i64, i64, C.c_int]),
    "amg_precond_apply_in_place": (i32, [vp, vp, i64, i64, C.c_int]),
    "amg_precond_transpose_apply_in_place": (i32, [vp, vp, i64, i64, C.c_int]),
    "amg_linop_destroy": (i32, [vp]),
    "amg_jacobi_create": (i32, [vp, dbl, P(vp)]),
    "amg_l1_create": (i32, [vp, P(vp)]),
    "amg_l2_create": (i32, [vp, P(vp)]),
    "amg_diag_create": (i32, [vp, i64, vp, P(vp)]),
    "amg_sgs_create": (i32, [vp, vp, P(vp)]),
    "amg_sgs_ncolors": (i32, [vp, P(i64)]),
    "amg_sgs_info": (i32, [vp, vp]),
    "amg_coarse_chol_create": (i32, [vp, P(vp)]),
    "amg_multigrid_create": (i32, [vp, vp, P(vp)]),
    "amg_multigrid_add_level": (i32, [vp, vp, vp, vp, vp]),
    "amg_multigrid_set": (i32, [vp, i64, i64]),
    "amg_multigrid_levels": (i32, [vp, P(i64)]),
    "amg_multigrid_set_graph": (i32, [vp, i32]),
    "amg_multigrid_set_option": (i32, [vp, i32, i64]),
    "amg_multigrid_apply": (i32, [vp, vp, i64, vp, i64, i64, C.c_int]),
    "amg_multigrid_get_level": (i32, [vp, i64, P(vp), P(vp), P(vp), P(vp)]),
    "amg_spgemm": (i32, [vp, vp, P(vp)]),
    "amg_transpose": (i32, [vp, P(vp)]),
    "amg_galerkin_rap": (i32, [vp, vp, vp, P(vp)]),
    "amg_smooth_interpolation": (i32, [vp, vp, dbl, P(vp)]),
    "amg_sa_tentative": (i32, [vp, i64, vp, i64, vp, P(vp), vp]),
    "amg_nn_stationary_l1": (i32, [vp, i64, vp]),
    "amg_sa_build_box": (i32, [vp, i64, i64, i64, i64, i64, i64, i64, i64, dbl, i32, P(vp)]),
    "amg_stationary_solve": (i32, [vp, vp, vp, vp, i64, dbl, vp, P(i64)]),
    "amg_pcg_solve": (i32, [vp, vp, vp, vp, i64, dbl, dbl, vp, P(i64)]),
    "amg_composite_create": (i32, [vp, vp, i64, P(vp)]),
    "amg_block_smoother_create": (i32, [vp, vp, i64, i64, P(vp)]),
    "amg_block_smoother_to_csr": (i32, [vp, P(vp)]),
    "amg_block_smoother_info": (i32, [vp, P(i64)]),
    "amg_composite_push": (i32, [vp, vp]),
    "amg_composite_ncomponents": (i32, [vp, P(i64)]),
    "amg_comm_unique_id_size": (i32, []),
    "amg_rccl_library": (C.c_char_p, []),
    "amg_comm_get_unique_id": (i32, [vp]),
    "amg_comm_create": (i32, [vp, i32, i32, vp, P(vp)]),
    "amg_loopback_hub_create": (i32, [i32, P(vp)]),
    "amg_loopback_hub_destroy": (i32, [vp]),
    "amg_comm_create_loopback": (i32, [vp, vp, i32, P(vp)]),
    "amg_comm_destroy": (i32, [vp]),
    "amg_comm_rank": (i32, [vp, P(i32), P(i32)]),
    "amg_comm_barrier": (i32, [vp]),
    "amg_comm_allreduce_max": (i32, [vp, P(dbl)]),
    "amg_comm_allreduce_sum": (i32, [vp, P(dbl)]),
    "amg_dist_multigrid_create": (i32, [vp, vp, vp, i64, P(vp)]),
    "amg_dist_local_rows": (i32, [vp, P(i64), P(i64)]),
    "amg_dist_level_info": (i32, [vp, i64, vp]),
    "amg_dist_level_operator": (i32, [vp, i64, P(vp)]),
    "amg_dist_level_matrix": (i32, [vp, i64, i32, P(vp)]),
    "amg_dist_set_option": (i32, [vp, i32, i64]),
    "amg_mtx_read": (i32, [C.c_char_p, P(vp)]),
    "amg_host_csr_dims": (i32, [vp, P(i64), P(i64), P(i64)]),
    "amg_host_csr_create": (i32, [i64, i64, vp, vp, vp, P(vp)]),
    "amg_host_csr_arrays": (i32, [vp, vp, vp, vp]),
    "amg_host_csr_upload": (i32, [vp, vp, P(vp)]),
    "amg_host_csr_destroy": (i32, [vp]),
    "amg_mfem_load": (i32, [C.c_char_p, C.c_char_p, i32, P(vp)]),
    "amg_mfem_info": (i32, [vp, vp]),
    "amg_mfem_matrix": (i32, [vp, P(vp)]),
    "amg_mfem_rhs": (i32, [vp, vp, i64]),
    "amg_mfem_coords": (i32, [vp, vp, i64]),
    "amg_mfem_boundary": (i32, [vp, vp]),
    "amg_mfem_index_maps": (i32, [vp, vp, vp]),
    "amg_mfem_destroy": (i32, [vp]),
    "amg_dist_stationary_solve": (i32, [vp, vp, vp, i64, dbl, vp, P(i64)]),
    "amg_sa_config_default": (i32, [vp]),
    "amg_sa_build": (i32, [vp, vp, i64, i64, vp, vp, P(vp)]),
    "amg_strength_graph": (i32, [vp, vp, i64, i64, vp, i64, i64, P(vp)]),
    "amg_aggregate_mis": (i32, [vp, vp, P(i64)]),
    "amg_set_sa_setup": (i32, [i32]),
    "amg_get_sa_setup": (i32, [P(i32)]),
    "amg_strength_graph_device": (i32, [vp, vp, i64, i64, vp, i64, C.c_int, P(vp)]),
    "amg_aggregate_mis_device": (i32, [vp, i64, vp, P(i64), vp]),
    "amg_pattern_ball_device": (i32, [vp, i64, P(vp)]),
    "amg_strength_graph_device_depth": (i32, [vp, vp, i64, i64, vp, i64, i64, C.c_int, i64, P(vp), vp]),
    "amg_sa_level_info": (i32, [vp, i64, vp]),
    "amg_sa_level_aggregates": (i32, [vp, i64, vp, P(i64)]),
    "amg_sa_refresh": (i32, [vp, vp, vp, i64, i64, vp]),
    "amg_spgemm_refill": (i32, [vp, vp, vp]),
    "amg_transpose_perm": (i32, [vp, vp, vp]),
    "amg_transpose_refill": (i32, [vp, vp, vp]),
    "amg_partitioner_config_default": (i32, [vp]),
    "amg_partition_modularity": (i32, [vp, vp, vp, P(i64), vp]),
    "amg_partition_modularity_device": (i32, [vp, vp, vp, P(i64), vp]),
    "amg_set_sa_partitioner": (i32, [i32, vp]),
    "amg_get_sa_partitioner": (i32, [P(i32), vp]),
    "amg_sa_tentative_block": (i32, [vp, i64, i64, vp, i64, vp, i64, i64, i64, P(vp), vp]),
    "amg_block_jacobi_smooth": (i32, [vp, vp, i64, dbl, P(vp)]),
    "amg_nn_postprocess": (i32, [vp, i64, vp, i64, i64]),
    "amg_gen_elasticity_q1": (i32, [i64, i64, i64, dbl, dbl, C.c_uint64, i32, P(vp)]),
    "amg_dist_pcg_solve": (i32, [vp, i32, vp, vp, i64, dbl, dbl, vp, P(i64)]),
    "amg_multigrid_cycle_plan": (i32, [vp, vp, i64, P(i64)]),
    "amg_multigrid_fine_launch": (i32, [vp, i32, vp, vp]),
    "amg_multigrid_set_fine_timer": (i32, [vp, i32]),
    "amg_multigrid_fine_timer_ms": (i32, [vp, vp]),
    "amg_dist_cycle_plan": (i32, [vp, vp, i64, P(i64)]),
    "amg_set_sgs_fused": (i32, [i32]),
    "amg_sgs_fused": (i32, [vp, P(i32)]),
    "amg_halo_plan_create": (i32, [i32, i32, vp, P(vp)]),
    "amg_halo_plan_destroy": (i32, [vp]),
    "amg_halo_plan_add_columns": (i32, [vp, i64, vp]),
    "amg_halo_plan_requests": (i32, [vp, vp, P(i64)]),
    "amg_halo_plan_ghost_ids": (i32, [vp, vp]),
    "amg_halo_plan_set_incoming": (i32, [vp, vp, vp]),
    "amg_halo_plan_info": (i32, [vp, vp]),
    "amg_halo_plan_neighbors": (i32, [vp, vp, vp, vp, vp, vp]),
    "amg_halo_plan_send_indices": (i32, [vp, vp]),
    "amg_halo_plan_remap": (i32, [vp, i64, vp, vp, vp, P(i64), P(i64)]),
    "amg_dist_first_redundant_level": (i32, [i64, vp, i64, P(i64)]),
    "amg_trace_mark": (i32, [vp, i32]),
    "amg_thin_qr": (i32, [vp, vp, i64, i64, i64, vp, C.c_int]),
    "amg_smooth_vectors": (i32, [vp, vp, vp, i64, i64, i64, vp, C.c_int]),
    "amg_create_weights": (i32, [vp, vp, i64, i64, vp, C.c_int]),
    "amg_find_near_null": (i32, [vp, vp, i64, i64, i64, i64, i64, vp, C.c_int]),
    "amg_csr_spmm_epilogue": (i32, [vp, i32, vp, i64, vp, i64, vp, i64, vp, i64]),
    "amg_multigrid_block_plan": (i32, [vp, i64, vp, i64, P(i64)]),
    "amg_adaptive_config_default": (i32, [vp]),
    "amg_adaptive_build": (i32, [vp, vp, i64, i64, vp, vp, P(vp)]),
    "amg_pcg_solve_block": (i32, [vp, vp, vp, i64, vp, i64, i64, i64, dbl, dbl, vp, i64, vp]),
    "amg_stationary_solve_block": (i32, [vp, vp, vp, i64, vp, i64, i64, i64, dbl, vp, i64, vp]),
    "amg_chebyshev_config_default": (i32, [vp]),
    "amg_chebyshev_create": (i32, [vp, vp, P(vp)]),
    "amg_chebyshev_info": (i32, [vp, vp]),
    "amg_block_cg_solve": (i32, [vp, vp, vp, i64, vp, i64, i64, i64, dbl, dbl, dbl, vp, i64, vp, P(i64)]),
    "amg_block_gram": (i32, [vp, vp, i64, i64, vp, i64, i64, vp, i64, i64, i64, vp]),
    "amg_block_gemm_update": (i32, [vp, vp, i64, vp, i64, vp, i64, i64, i64, i32]),
    "amg_classical_config_default": (i32, [vp]),
    "amg_cr_mis": (i32, [vp, vp, vp, P(i64)]),
    "amg_cr_split": (i32, [vp, vp, vp, vp, vp, P(i64), vp]),
    "amg_classical_build": (i32, [vp, vp, i64, i64, vp, vp, P(vp), vp]),
    "amg_ls_candidates": (i32, [vp, vp, i64, P(vp)]),
    "amg_ls_search": (i32, [vp, vp, vp, i64, i64, vp, i64, i32, i64, vp, vp, vp, vp, vp]),
    "amg_ls_accept": (i32, [i64, vp, i64, i64, vp, i64, dbl, vp, vp, vp]),
    "amg_ls_interpolation": (i32, [vp, vp, vp, i64, i64, vp, vp, P(vp), vp, vp, vp]),
}

for _name, (_res, _args) in SIGNATURES.items():
    _f = getattr(_lib, _name)
    _f.restype = _res
    _f.argtypes = _args


class LaunchRec(C.Structure):
    """amg_launch_rec (include/amg.h)."""
    _fields_ = [("level", i32), ("role", i32), ("kernel", i32), ("mode", i32), ("rows", i64),
                ("bytes", i64), ("csr_bytes", i64), ("name", C.c_char * 32)]


ROLES = {0: "smooth", 1: "resid", 2: "restrict", 3: "interp", 4: "coarse", 5: "other"}
MODES = {-1: "-", 0: "SET", 1: "ADD", 2: "RESID", 3: "JACOBI", 4: "SGS", 5: "RESID0", 6: "ADD0", 7: "SETDF"}


class AmgError(RuntimeError):
    """Non-OK amg_status (the reference panics in these cases)."""

    def __init__(self, status, msg):
        super().__init__(f"amg status {status}: {msg}")
        self.status = status


def _ck(status):
    if status != 0:
        raise AmgError(status, _lib.amg_last_error().decode())


def lib():
    return _lib


def version():
    return _lib.amg_version().decode()


SPMV_FORMATS = {"auto": 0, "csr": 1, "sell": 2, "vector": 3}


def set_spmv_format(policy):
    """SpMV storage for matrices built afterwards: 'auto', 'csr', 'sell' or 'vector'."""
    _ck(_lib.amg_set_spmv_format(SPMV_FORMATS[policy]))


def set_value_codes(enable):
    """SELL matrices built afterwards store 4/8/16-bit codes into a per-matrix
    table of distinct values when they have <= 65536 of them (default True)."""
    _ck(_lib.amg_set_value_codes(1 if enable else 0))


def set_alloc_policy(contiguous):
    """Physically contiguous device allocations for large buffers: refused (True
    raises) -- they read stale data across kernels on gfx950."""
    _ck(_lib.amg_set_alloc_policy(1 if contiguous else 0))


def _dptr(x):
    """(pointer, mem kind, nrows, ncols, ld) of a torch tensor or numpy array."""
    try:
        import torch
        if isinstance(x, torch.Tensor):
            if x.dtype != torch.float64:
                raise TypeError("vectors must be float64")
            if x.dim() == 1:
                if not x.is_contiguous():
                    raise ValueError("vector must be contiguous")
                n, k, ld = x.shape[0], 1, x.shape[0]
            else:
                # column-major n x k (torch: a (k, n) row-major tensor transposed)
                n, k = x.shape
                if x.stride(0) != 1:
                    raise ValueError("matrix must be column-major (stride(0) == 1)")
                ld = x.stride(1) if k > 1 else n
            return vp(x.data_ptr()), (AMG_MEM_DEVICE if x.is_cuda else AMG_MEM_HOST), n, k, ld
    except ImportError:
        pass
    if not isinstance(x, np.ndarray) or x.dtype != np.float64:
        raise TypeError("vectors must be float64 numpy arrays or torch tensors")
    if x.ndim == 1:
        if not x.flags.c_contiguous:
            raise ValueError("vector must be contiguous")
        return x.ctypes.data_as(vp), AMG_MEM_HOST, x.shape[0], 1, x.shape[0]
    if not x.flags.f_contiguous:
        raise ValueError("matrix must be Fortran (column-major) ordered")
    return x.ctypes.data_as(vp), AMG_MEM_HOST, x.shape[0], x.shape[1], x.shape[0]


class Context:
    """One device per process (amg_ctx).  `stream` may be a raw hipStream_t int.

    Device-memory calls made through this module are ordered against the
    caller's torch.cuda.current_stream() automatically (amg_ctx_join_stream)."""

    def __init__(self, device=0, stream=None):
        h = vp()
        _ck(_lib.amg_ctx_create(device, vp(stream) if stream else None, C.byref(h)))
        self.h = h
        self.device = device
        s = vp()
        _ck(_lib.amg_ctx_stream(self.h, C.byref(s)))
        self._stream = s.value or 0

    def synchronize(self):
        _ck(_lib.amg_ctx_synchronize(self.h))

    def trace_mark(self, tag):
        """Launch k_trace_mark with `tag` blocks (brackets a region of a kernel trace)."""
        _ck(_lib.amg_trace_mark(self.h, tag))

    @property
    def stream(self):
        return self._stream

    def join_torch(self, ctx_waits):
        """Order the library stream with torch's current stream (see amg_ctx_join_stream)."""
        import torch
        cur = torch.cuda.current_stream(self.device).cuda_stream
        if cur != self._stream:
            _ck(_lib.amg_ctx_join_stream(self.h, vp(cur) if cur else None, 1 if ctx_waits else 0))

    def __del__(self, _destroy=_lib.amg_ctx_destroy):
        if getattr(self, "h", None):
            _destroy(self.h)
            self.h = None


class _ordered:
    """Context manager: library stream waits for torch's stream before a device
    call, torch's stream waits for the library stream after it."""

    def __init__(self, ctx, mem):
        self.ctx, self.on = ctx, (mem == AMG_MEM_DEVICE and ctx is not None)

    def __enter__(self):
        if self.on:
            self.ctx.join_torch(True)

    def __exit__(self, *exc):
        if self.on:
            self.ctx.join_torch(False)
        return False


class LinOp:
    """Handle on any library operator (faer matrix_free LinOp/Precond/BiPrecond)."""

    def __init__(self, handle, ctx, refs=()):
        self.h = handle
        self.ctx = ctx
        self._refs = refs  # python-side references (the C side holds its own)

    def __del__(self, _destroy=_lib.amg_linop_destroy):
        if getattr(self, "h", None):
            _destroy(self.h)
            self.h = None

    @property
    def kind(self):
        k = i32()
        _ck(_lib.amg_linop_kind_of(self.h, C.byref(k)))
        return KINDS[k.value]

    def dims(self):
        r, c = i64(), i64()
        _ck(_lib.amg_linop_dims(self.h, C.byref(r), C.byref(c)))
        return r.value, c.value

    @property
    def nrows(self):
        return self.dims()[0]

    @property
    def ncols(self):
        return self.dims()[1]

    def apply(self, out, rhs):
        """LinOp::apply: out = M rhs (out overwritten)."""
        po, mo, no, ko, lo = _dptr(out)
        pr, mr, nr, kr, lr = _dptr(rhs)
        if mo != mr or ko != kr:
            raise ValueError("out and rhs must live in the same memory with equal columns")
        with _ordered(self.ctx, mo):
            _ck(_lib.amg_linop_apply(self.h, po, lo, pr, lr, ko, mo))
        return out

    def transpose_apply(self, out, rhs):
        po, mo, no, ko, lo = _dptr(out)
        pr, mr, nr, kr, lr = _dptr(rhs)
        with _ordered(self.ctx, mo):
            _ck(_lib.amg_linop_transpose_apply(self.h, po, lo, pr, lr, ko, mo))
        return out

    def apply_in_place(self, rhs):
        """Precond::apply_in_place: rhs <- M rhs."""
        p, m, n, k, ld = _dptr(rhs)
        with _ordered(self.ctx, m):
            _ck(_lib.amg_precond_apply_in_place(self.h, p, ld, k, m))
        return rhs

    def transpose_apply_in_place(self, rhs):
        p, m, n, k, ld = _dptr(rhs)
        with _ordered(self.ctx, m):
            _ck(_lib.amg_precond_transpose_apply_in_place(self.h, p, ld, k, m))
        return rhs

    def __matmul__(self, x):
        """Host convenience: M @ numpy vector (staged through the device)."""
        x = np.ascontiguousarray(x, np.float64)
        out = np.zeros(self.nrows)
        return self.apply(out, x)


class SparseMatOp(LinOp):
    """Device CSR operator (SparseMatOp / ParSpmmOp of the reference)."""

    @classmethod
    def from_arrays(cls, ctx, nrows, ncols, rowptr, col, val):
        rp = np.ascontiguousarray(rowptr, np.int64)
        ci = np.ascontiguousarray(col, np.int64)
        va = np.ascontiguousarray(val, np.float64)
        h = vp()
        _ck(_lib.amg_csr_create(ctx.h, int(nrows), int(ncols), rp.ctypes.data_as(vp),
                                ci.ctypes.data_as(vp), va.ctypes.data_as(vp), C.byref(h)))
        return cls(h, ctx)

    @classmethod
    def from_scipy(cls, ctx, M):
        M = M.tocsr()
        M.sort_indices()
        return cls.from_arrays(ctx, M.shape[0], M.shape[1], M.indptr, M.indices, M.data)

    @classmethod
    def laplace3d_7pt(cls, ctx, nx, ny, nz):
        h = vp()
        _ck(_lib.amg_gen_laplace3d_7pt(ctx.h, nx, ny, nz, C.byref(h)))
        return cls(h, ctx)

    @classmethod
    def aniso27(cls, ctx, nx, ny, nz, ex=1.0, ey=1.0, ez=0.01):
        h = vp()
        _ck(_lib.amg_gen_aniso27(ctx.h, nx, ny, nz, ex, ey, ez, C.byref(h)))
        return cls(h, ctx)

    @classmethod
    def random7(cls, ctx, nx, ny, nz, seed=42, window=4096):
        """Random-coefficient 7-pt SPD operator, symmetrically permuted
        (window < 0 none, 0 all rows, > 0 within windows of that many rows)."""
        h = vp()
        _ck(_lib.amg_gen_random_7pt(ctx.h, nx, ny, nz, seed, window, C.byref(h)))
        return cls(h, ctx)

    @property
    def nnz(self):
        v = i64()
        _ck(_lib.amg_csr_nnz(self.h, C.byref(v)))
        return v.value

    def spmv_info(self):
        """SpMV storage chosen for this matrix (kernel, bytes streamed per SpMV, SELL stats)."""
        info = np.zeros(8, np.int64)
        _ck(_lib.amg_csr_spmv_info(self.h, info.ctypes.data_as(vp)))
        keys = ("kernel", "stream_bytes", "csr_bytes", "slices", "stored_entries",
                "slices_implicit", "slices_u16", "slices_i32")
        d = dict(zip(keys, (int(v) for v in info)))
        d["kernel"] = ("csr-stream", "sell", "vector", "dia", "bsr", "sellp", "classes", "xsell", "gtc")[d["kernel"]]
        vc = np.zeros(2, np.int64)
        _ck(_lib.amg_csr_value_codes(self.h, vc.ctypes.data_as(vp)))
        d["value_bits"], d["value_table"] = int(vc[0]), int(vc[1])
        dr = np.zeros(4, np.int64)
        _ck(_lib.amg_csr_dia_range(self.h, dr.ctypes.data_as(vp)))
        d["dia_rows"] = (int(dr[0]), int(dr[1]))
        d["dia_diagonals"], d["dia_bits"] = int(dr[2]), int(dr[3])
        ci = np.zeros(4, np.int64)
        _ck(_lib.amg_csr_class_info(self.h, ci.ctypes.data_as(vp)))
        d["classes"], d["class_offsets"], d["class_id_bits"] = int(ci[0]), int(ci[1]), int(ci[2])
        g = np.zeros(13, np.int64)
        _ck(_lib.amg_csr_grid_info(self.h, g.ctypes.data_as(vp)))
        d["grid"] = tuple(int(v) for v in g[:3])
        d["grid_source"] = ("none", "given", "inferred")[int(g[10])]
        d["gtc"] = ("none", "P", "R", "P", "R")[int(g[11])]
        d["gtc_kind"] = ("none", "gtc", "gtc", "gtx", "gtx")[int(g[11])]
        d["xstaged"] = bool(g[3])
        if d["xstaged"]:
            d["tile"], d["halo"] = tuple(int(v) for v in g[4:7]), tuple(int(v) for v in g[7:10])
            d["tile_source"] = ("none", "table", "timed", "env", "rule")[int(g[12])]
        rl = i64()
        _ck(_lib.amg_csr_row_lanes(self.h, C.byref(rl)))
        d["row_lanes"] = rl.value
        return d

    def spmv_epilogue(self, mode, x, y, b=None, d=None):
        """amg_csr_spmv_epilogue on device tensors: mode "set" y = A x, "add" y += A x,
        "resid" y = b - A x, "jacobi" y = x + d (b - A x)."""
        m = {"set": 0, "add": 1, "resid": 2, "jacobi": 3}[mode]
        ptr = lambda t: None if t is None else vp(t.data_ptr())  # noqa: E731
        with _ordered(self.ctx, AMG_MEM_DEVICE):  # y / b / d written on torch's stream
            _ck(_lib.amg_csr_spmv_epilogue(self.h, m, ptr(x), ptr(y), ptr(b), ptr(d)))

    def spmm_epilogue(self, mode, X, Y, B=None, d=None):
        """amg_csr_spmm_epilogue on column-major device blocks (n x k torch tensors
        with stride(0) == 1): the k-wide spmv_epilogue, each column bitwise that call."""
        m = {"set": 0, "add": 1, "resid": 2, "jacobi": 3}[mode]
        px, _, _, k, ldx = _dptr(X)
        py, _, _, ky, ldy = _dptr(Y)
        if k != ky:
            raise ValueError("X and Y must have equal columns")
        pb, ldb = (None, 0) if B is None else (_dptr(B)[0], _dptr(B)[4])
        with _ordered(self.ctx, AMG_MEM_DEVICE):
            _ck(_lib.amg_csr_spmm_epilogue(self.h, m, px, ldx, py, ldy, pb, ldb,
                                           None if d is None else vp(d.data_ptr()), k))

    def set_grid(self, nx, ny, nz):
        """Grid hint (amg_csr_set_grid): the rows are an nx x ny x nz grid; re-finalizes the storage."""
        _ck(_lib.amg_csr_set_grid(self.h, nx, ny, nz))

    def arrays(self):
        m, n = self.dims()
        nnz = self.nnz
        rp = np.zeros(m + 1, np.int64)
        ci = np.zeros(max(nnz, 1), np.int64)
        va = np.zeros(max(nnz, 1), np.float64)
        _ck(_lib.amg_csr_download(self.h, rp.ctypes.data_as(vp), ci.ctypes.data_as(vp),
                                  va.ctypes.data_as(vp)))
        return rp, ci[:nnz], va[:nnz]

    def to_scipy(self):
        import scipy.sparse as sp
        rp, ci, va = self.arrays()
        return sp.csr_matrix((va, ci, rp), shape=self.dims())


def csr_spmm_epilogue(A, mode, X, Y, B=None, d=None):
    """amg_csr_spmm_epilogue: the k-wide csr spmv_epilogue (SparseMatOp.spmm_epilogue, the
    method beside SparseMatOp.spmv_epilogue, is the same call)."""
    A.spmm_epilogue(mode, X, Y, B, d)


FLAGS = {"fold_xscs": 0, "dia_dk": 1, "vec_wpr": 2, "gtx_time": 3, "sgs27_march": 4, "xs_pipe": 5, "bsr_kernel": 6,
         "bsr_long": 7,
         "dia7_rp": 8, "fine_fuse": 9, "dense_tail": 10, "block_cycle": 11,
         "block_smoother_cols": 12}


def set_flag(name, value):
    """amg_set_flag: a run-time A/B switch (bitwise neutral); multigrids re-capture
    their graphs at the next apply."""
    _ck(_lib.amg_set_flag(FLAGS[name], int(value)))


def get_flag(name):
    v = i64()
    _ck(_lib.amg_get_flag(FLAGS[name], C.byref(v)))
    return v.value


def grid_from_offsets(offsets, n):
    """amg_grid_from_offsets (host only): the (nx, ny, nz) grid the library infers
    for an n-row square operator whose stencil has these col - row offsets, or None."""
    o = np.ascontiguousarray(np.asarray(offsets, dtype=np.int64))
    g = np.zeros(3, np.int64)
    found = C.c_int32(0)
    _ck(_lib.amg_grid_from_offsets(o.ctypes.data_as(vp), len(o), int(n), g.ctypes.data_as(vp), C.byref(found)))
    return tuple(int(v) for v in g) if found.value else None


def _wrap(h, ctx, cls=LinOp, refs=()):
    return cls(h, ctx, refs)


def new_jacobi(A, omega=0.66):
    h = vp()
    _ck(_lib.amg_jacobi_create(A.h, omega, C.byref(h)))
    return _wrap(h, A.ctx)


def new_l1(A):
    h = vp()
    _ck(_lib.amg_l1_create(A.h, C.byref(h)))
    return _wrap(h, A.ctx)


def new_l2(A):
    h = vp()
    _ck(_lib.amg_l2_create(A.h, C.byref(h)))
    return _wrap(h, A.ctx)


def diag(ctx, d):
    d = np.ascontiguousarray(d, np.float64)
    h = vp()
    _ck(_lib.amg_diag_create(ctx.h, len(d), d.ctypes.data_as(vp), C.byref(h)))
    return _wrap(h, ctx)


class SymGaussSeidel(LinOp):
    def __init__(self, A, colors=None):
        h = vp()
        cp = None
        if colors is not None:
            colors = np.ascontiguousarray(colors, np.int32)
            cp = colors.ctypes.data_as(vp)
        _ck(_lib.amg_sgs_create(A.h, cp, C.byref(h)))
        super().__init__(h, A.ctx)

    @property
    def ncolors(self):
        v = i64()
        _ck(_lib.amg_sgs_ncolors(self.h, C.byref(v)))
        return v.value

    def sweep_storage(self):
        """{'colors', 'kernel' ('sell', 'dia', ...), 'diagonals', 'bits'} of the color sweeps."""
        return sgs_info(self)


def sgs_info(S):
    info = np.zeros(4, np.int64)
    _ck(_lib.amg_sgs_info(S.h, info.ctypes.data_as(vp)))
    return {"colors": int(info[0]), "kernel": ("csr-stream", "sell", "vector", "dia", "bsr", "sellp")[int(info[1])],
            "diagonals": int(info[2]), "bits": int(info[3])}


def set_sgs_fused(enable):
    """SGS smoothers built afterwards use the fused plane-parity phases where they
    apply (True / 1: three phases per step, 2: four phases, False / 0: colour launches)."""
    _ck(_lib.amg_set_sgs_fused(int(enable)))


def sgs_fused(S):
    v = i32()
    _ck(_lib.amg_sgs_fused(S.h, C.byref(v)))
    return bool(v.value)


class ChebyshevConfig(C.Structure):
    """amg_chebyshev_config (include/amg.h)."""
    _fields_ = [("steps", i64), ("eig_iters", i64), ("eig_ratio", dbl), ("boost", dbl), ("lambda_max", dbl)]

    def __init__(self, **kw):
        super().__init__()
        _ck(_lib.amg_chebyshev_config_default(C.byref(self)))
        for k, v in kw.items():
            setattr(self, k, v)


def new_chebyshev(A, steps=2, eig_ratio=20.0, eig_iters=10, boost=1.1, lambda_max=0.0):
    """Chebyshev polynomial smoother on D^-1 A over [lambda_max / eig_ratio, lambda_max]
    (amg_chebyshev_create): lambda_max = min(boost * Lanczos Ritz value, row-sum bound),
    or the caller's when lambda_max > 0."""
    cfg = ChebyshevConfig(steps=steps, eig_ratio=eig_ratio, eig_iters=eig_iters, boost=boost, lambda_max=lambda_max)
    h = vp()
    _ck(_lib.amg_chebyshev_create(A.h, C.byref(cfg), C.byref(h)))
    return _wrap(h, A.ctx)


def chebyshev_info(S):
    """{'lambda_max', 'lambda_min', 'steps', 'ritz' (0.0: Lanczos not run), 'row_sum_bound'
    (0.0: not computed), 'eig_iters' (Lanczos steps run)} of a Chebyshev smoother."""
    info = np.zeros(6, np.float64)
    _ck(_lib.amg_chebyshev_info(S.h, info.ctypes.data_as(vp)))
    return {"lambda_max": float(info[0]), "lambda_min": float(info[1]), "steps": int(info[2]),
            "ritz": float(info[3]), "row_sum_bound": float(info[4]), "eig_iters": int(info[5])}


def CoarseCholesky(A):
    """CoarseSolverKind::Cholesky.build_from_sparse (coarse_solvers.rs:22-33)."""
    h = vp()
    _ck(_lib.amg_coarse_chol_create(A.h, C.byref(h)))
    return _wrap(h, A.ctx)


class Multigrid(LinOp):
    """Multigrid (multigrid.rs:171-518)."""

    def __init__(self, op, smoother, _handle=None):
        if _handle is None:
            h = vp()
            _ck(_lib.amg_multigrid_create(op.h, smoother.h, C.byref(h)))
        else:
            h = _handle
        super().__init__(h, op.ctx)

    @classmethod
    def _from_handle(cls, h, ctx):
        obj = cls.__new__(cls)
        LinOp.__init__(obj, h, ctx)
        return obj

    def add_level(self, op, smoother, r, p):
        _ck(_lib.amg_multigrid_add_level(self.h, op.h, smoother.h, r.h, p.h))
        return self

    def with_cycle_type(self, mu):
        self._mu = mu
        _ck(_lib.amg_multigrid_set(self.h, mu, getattr(self, "_steps", 1)))
        return self

    def with_smoothing_steps(self, steps):
        self._steps = steps
        _ck(_lib.amg_multigrid_set(self.h, getattr(self, "_mu", 1), steps))
        return self

    def set_graph(self, enable):
        _ck(_lib.amg_multigrid_set_graph(self.h, 1 if enable else 0))

    def set_reorder(self, mode):
        """Locality reordering of general levels (multigrid option 5): 0 off, 1 auto, 2 force."""
        _ck(_lib.amg_multigrid_set_option(self.h, 5, int(mode)))

    def run_level(self, l):
        """(A, S, R, P) the cycle runs on level l: the renumbered copies of a renumbered level."""
        a, s, r, p = vp(), vp(), vp(), vp()
        _ck(_lib.amg_multigrid_get_run_level(self.h, l, C.byref(a), C.byref(s), C.byref(r), C.byref(p)))
        return (SparseMatOp(a, self.ctx), LinOp(s, self.ctx),
                SparseMatOp(r, self.ctx) if r.value else None,
                SparseMatOp(p, self.ctx) if p.value else None)

    def set_fine_timer(self, which):
        """In-cycle timing of fused fine-level launch `which` (0 / 1; -1 off):
        every cycle records HIP events around it (amg_multigrid_set_fine_timer)."""
        _ck(_lib.amg_multigrid_set_fine_timer(self.h, int(which)))

    def fine_timer_ms(self):
        """Milliseconds of the timed launch in the last completed cycle."""
        v = C.c_float()
        _ck(_lib.amg_multigrid_fine_timer_ms(self.h, C.byref(v)))
        return float(v.value)

    def fine_launch(self, which, out, rhs):
        """One fused fine-level launch as the cycle makes it (amg_multigrid_fine_launch):
        which 0 = residual + restriction, 1 = interpolation + post-smoothing; device
        tensors, asynchronous on the context stream.  False where the cycle has none."""
        import torch
        n = self.nrows
        for t in (rhs,) if out is None else (rhs, out):
            if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float64 and t.is_contiguous()
                    and t.numel() == n):
                raise ValueError("fine_launch: contiguous float64 device vectors of the fine level's size")
        st = _lib.amg_multigrid_fine_launch(self.h, int(which), None if out is None else C.c_void_p(out.data_ptr()),
                                            C.c_void_p(rhs.data_ptr()))
        if st == 0:
            return True
        if st == 3:  # AMG_ERR_UNSUPPORTED
            return False
        _ck(st)

    def reordered(self, l):
        """Whether level l runs in a renumbered (locality) numbering."""
        v = i32()
        _ck(_lib.amg_multigrid_level_reordered(self.h, l, C.byref(v)))
        return bool(v.value)

    def set_sgs_residual_form(self, enable):
        """Literal smooth() order for SGS (residual SpMV + SGS(r)) instead of the fused sweep."""
        _ck(_lib.amg_multigrid_set_option(self.h, 1, 1 if enable else 0))

    def set_fold_zero_guess(self, enable):
        """Fold the zero-guess Jacobi step into the residual/correction SpMVs (default on)."""
        _ck(_lib.amg_multigrid_set_option(self.h, 2, 1 if enable else 0))

    def set_restrict_df(self, enable):
        """R on wide grid-transfer classes also writes the next level's first Jacobi step
        from zero (SPMV_SETDF; default on; bitwise the separate d*f pass)."""
        _ck(_lib.amg_multigrid_set_option(self.h, 4, 1 if enable else 0))

    def levels(self):
        v = i64()
        _ck(_lib.amg_multigrid_levels(self.h, C.byref(v)))
        return v.value

    def cycle_plan(self):
        """The launches of one V-cycle in order (amg_multigrid_cycle_plan): list of
        dicts {level, role, kernel, mode, name, rows, bytes, csr_bytes}."""
        n = i64()
        _ck(_lib.amg_multigrid_cycle_plan(self.h, None, 0, C.byref(n)))
        recs = (LaunchRec * max(1, n.value))()
        _ck(_lib.amg_multigrid_cycle_plan(self.h, recs, n.value, C.byref(n)))
        return [{"level": r.level, "role": ROLES.get(r.role, "?"), "kernel": r.kernel,
                 "mode": MODES.get(r.mode, "?"), "name": r.name.decode(), "rows": r.rows,
                 "bytes": r.bytes, "csr_bytes": r.csr_bytes} for r in recs[:n.value]]

    def block_plan(self, k):
        """The launches of one block V-cycle of k columns (amg_multigrid_block_plan),
        as cycle_plan() lists its own."""
        n = i64()
        _ck(_lib.amg_multigrid_block_plan(self.h, k, None, 0, C.byref(n)))
        recs = (LaunchRec * max(1, n.value))()
        _ck(_lib.amg_multigrid_block_plan(self.h, k, recs, n.value, C.byref(n)))
        return [{"level": r.level, "role": ROLES.get(r.role, "?"), "kernel": r.kernel,
                 "mode": MODES.get(r.mode, "?"), "name": r.name.decode(), "rows": r.rows,
                 "bytes": r.bytes, "csr_bytes": r.csr_bytes} for r in recs[:n.value]]

    def sa_level_info(self, level):
        """amg_sa_level_info: the record smoothed_aggregation kept of coarsening step
        `level` as 8 integers -- (n, block size, nodes, aggregates, strength edges,
        built on the device 0/1, reason it stayed on the host, longest ball); reasons
        0 none, 1 policy, 2 ball cap, 3 byte budget, 4 index range."""
        out = np.zeros(8, np.int64)
        _ck(_lib.amg_sa_level_info(self.h, int(level), out.ctypes.data_as(vp)))
        return tuple(int(v) for v in out)

    def sa_aggregates(self, level):
        """amg_sa_level_aggregates: (agg_of, naggs) smoothed_aggregation recorded for
        coarsening step `level` -- the aggregate of every node (int64) and their count."""
        nodes = self.sa_level_info(level)[2]
        agg = np.zeros(nodes, np.int64)
        na = i64()
        _ck(_lib.amg_sa_level_aggregates(self.h, int(level), agg.ctypes.data_as(vp), C.byref(na)))
        return agg, na.value

    def refresh(self, A_new, near_null):
        """amg_sa_refresh: rebuild this smoothed_aggregation hierarchy for A_new (the
        build's sparsity pattern, new values) and near_null (n x k, the build's k) on the
        recorded aggregates.  The first call records the product patterns, later ones are
        numeric only; a failure leaves the hierarchy as it was.  Level handles taken
        before keep the old operators.  Returns {recorded, record_bytes, levels, steps}."""
        nn = _colmajor_host(near_null, A_new.nrows)
        out = np.zeros(8, np.int64)
        _ck(_lib.amg_sa_refresh(self.h, A_new.h, nn.ctypes.data_as(vp), nn.shape[0], nn.shape[1],
                                out.ctypes.data_as(vp)))
        return {"recorded": bool(out[0]), "record_bytes": int(out[1]), "levels": int(out[2]), "steps": int(out[3])}

    def level(self, l):
        """(A, S, R, P) handles of level l (R, P None on the coarsest)."""
        a, s, r, p = vp(), vp(), vp(), vp()
        _ck(_lib.amg_multigrid_get_level(self.h, l, C.byref(a), C.byref(s), C.byref(r), C.byref(p)))
        S = LinOp(s, self.ctx)
        if S.kind == "block":  # to_sparse() and info() of a level's BlockSmoother
            S.__class__ = BlockSmoother
        return (SparseMatOp(a, self.ctx), S,
                SparseMatOp(r, self.ctx) if r.value else None,
                SparseMatOp(p, self.ctx) if p.value else None)


def spgemm(A, B):
    h = vp()
    _ck(_lib.amg_spgemm(A.h, B.h, C.byref(h)))
    return SparseMatOp(h, A.ctx)


def transpose(P_):
    h = vp()
    _ck(_lib.amg_transpose(P_.h, C.byref(h)))
    return SparseMatOp(h, P_.ctx)


def spgemm_refill(A, B, C_):
    """amg_spgemm_refill: overwrite C_'s values with A B on C_'s given pattern (spgemm's
    values bit for bit, 0.0 outside the product); AmgError (invalid) if a product column
    is missing from C_."""
    _ck(_lib.amg_spgemm_refill(A.h, B.h, C_.h))
    return C_


def transpose_perm(P_, R):
    """amg_transpose_perm: int32 perm with R.val[q] = P_.val[perm[q]] for R = P_^T."""
    perm = np.zeros(P_.nnz, np.int32)
    _ck(_lib.amg_transpose_perm(P_.h, R.h, perm.ctypes.data_as(vp)))
    return perm


def transpose_refill(P_, R, perm):
    """amg_transpose_refill: overwrite R's values with P_'s through perm (transpose_perm)."""
    perm = np.ascontiguousarray(perm, np.int32)
    if perm.shape != (P_.nnz,):
        raise ValueError("perm must have one entry per stored entry of P")
    _ck(_lib.amg_transpose_refill(P_.h, R.h, perm.ctypes.data_as(vp)))
    return R


def galerkin_rap(R, A, P_):
    h = vp()
    _ck(_lib.amg_galerkin_rap(R.h, A.h, P_.h, C.byref(h)))
    return SparseMatOp(h, A.ctx)


def smooth_interpolation(A, P_, omega=0.66):
    h = vp()
    _ck(_lib.amg_smooth_interpolation(A.h, P_.h, omega, C.byref(h)))
    return SparseMatOp(h, A.ctx)


def sa_tentative(ctx, agg_of, naggs, near_null):
    agg = np.ascontiguousarray(agg_of, np.int64)
    nn = np.ascontiguousarray(near_null, np.float64)
    cnn = np.zeros(naggs)
    h = vp()
    _ck(_lib.amg_sa_tentative(ctx.h, len(agg), agg.ctypes.data_as(vp), naggs,
                              nn.ctypes.data_as(vp), C.byref(h), cnn.ctypes.data_as(vp)))
    return SparseMatOp(h, ctx), cnn


def nn_stationary_l1(A, x, iters=3):
    x = np.array(x, np.float64, copy=True)
    _ck(_lib.amg_nn_stationary_l1(A.h, iters, x.ctypes.data_as(vp)))
    return x


SMOOTHERS = {"jacobi": 0, "l1": 1, "sgs": 2, "block": 3, "chebyshev": 4}


def _smoother_code(smoother):
    return SMOOTHERS[smoother] if isinstance(smoother, str) else int(smoother)


def sa_build_box(A, dims, box=(2, 2, 2), coarsest_dim=1000, max_levels=0, omega=0.66,
                 smoother="jacobi"):
    """SA hierarchy + multigrid on a structured grid (Hierarchy::coarsen + Multigrid).
    smoother: a name of SMOOTHERS or its code (4 / 'chebyshev': the default config)."""
    h = vp()
    _ck(_lib.amg_sa_build_box(A.h, dims[0], dims[1], dims[2], box[0], box[1], box[2],
                              coarsest_dim, max_levels, omega, _smoother_code(smoother), C.byref(h)))
    return Multigrid._from_handle(h, A.ctx)


class SaConfig(C.Structure):
    """amg_sa_config: AggregationConfig + HierarchyConfig + the smoother choice
    (interpolation/mod.rs:62-79, hierarchy.rs:21-36)."""
    _fields_ = [("block_size", i64), ("candidate_dimension", i64), ("strength_depth", i64),
                ("smoothing_steps", i64), ("coarsest_dim", i64), ("max_levels", i64),
                ("omega", dbl), ("smoother", i32), ("chebyshev_steps", i32)]

    def __init__(self, **kw):
        super().__init__()
        _ck(_lib.amg_sa_config_default(C.byref(self)))
        for k, v in kw.items():
            if k == "smoother" and isinstance(v, str):
                v = SMOOTHERS[v]
            setattr(self, k, v)


def _colmajor_host(x, nrows):
    x = np.asarray(x, np.float64)
    if x.ndim == 1:
        x = x[:, None]
    x = np.asfortranarray(x)
    if x.shape[0] != nrows:
        raise ValueError("near-null space must have one row per matrix row")
    return x


def smoothed_aggregation(A, near_null, weights=None, **config):
    """SA hierarchy + multigrid for a general SPD matrix (Hierarchy::coarsen with
    AggregationConfig, hierarchy.rs:190-248; interpolation/mod.rs:730-836).
    near_null: n x k candidates; weights: k strength weights (None: 1/v^T A v);
    config: SaConfig fields (block_size, candidate_dimension, strength_depth,
    smoothing_steps, coarsest_dim, max_levels, omega, smoother -- a name of SMOOTHERS
    or its code -- and chebyshev_steps for smoother 4 / 'chebyshev')."""
    cfg = SaConfig(**config)
    nn = _colmajor_host(near_null, A.nrows)
    w = None if weights is None else np.ascontiguousarray(weights, np.float64)
    h = vp()
    _ck(_lib.amg_sa_build(A.h, nn.ctypes.data_as(vp), nn.shape[0], nn.shape[1],
                          None if w is None else w.ctypes.data_as(vp), C.byref(cfg), C.byref(h)))
    return Multigrid._from_handle(h, A.ctx)


def strength_graph(A, near_null, weights, depth=1, block_size=1):
    """Node-level strength graph (partitioners/mod.rs:337-393) as scipy CSR."""
    nn = _colmajor_host(near_null, A.nrows)
    w = np.ascontiguousarray(weights, np.float64)
    h = vp()
    _ck(_lib.amg_strength_graph(A.h, nn.ctypes.data_as(vp), nn.shape[0], nn.shape[1],
                                w.ctypes.data_as(vp), depth, block_size, C.byref(h)))
    return HostCsr(h).to_scipy()


def aggregate_mis(G):
    """MIS-seeded aggregates of a strength graph (scipy CSR): (agg_of, naggs)."""
    G = G.tocsr()
    n = G.shape[0]
    tmp = HostCsr(_host_csr_from_scipy(G))
    agg = np.zeros(n, np.int64)
    na = i64()
    _ck(_lib.amg_aggregate_mis(tmp.h, agg.ctypes.data_as(vp), C.byref(na)))
    return agg, na.value


SA_SETUP = {"host": 0, "device": 1}


def set_sa_setup(where):
    """amg_set_sa_setup (process-wide): where amg_sa_build and amg_find_near_null run
    the strength graph and the aggregation -- 'host' / 0 (default) or 'device' / 1, at
    any strength depth (depth > 1: the BFS balls are built on the device too).  A level
    whose candidate lists pass 4096, whose ball pattern passes half the free device
    memory or 2^31 entries keeps the host path; Multigrid.sa_level_info says which.
    Not bitwise neutral: the device weighs an edge with (t*t)*(t*t) where the host
    calls pow(t, 4.0)."""
    _ck(_lib.amg_set_sa_setup(SA_SETUP[where] if isinstance(where, str) else int(where)))


def get_sa_setup():
    v = i32()
    _ck(_lib.amg_get_sa_setup(C.byref(v)))
    return v.value


_SG_INFO = ("longest_ball", "wave_rows", "block_rows", "ball_entries", "dof_entries", "node_edges")


def pattern_ball_device(A, depth):
    """amg_pattern_ball_device: the BFS ball of every row of A's pattern (depth >= 1,
    stored entries only, without the row itself, columns ascending) as a SparseMatOp
    with unit values and no SpMV storage.  AmgError status 3 for a ball beyond 4096."""
    h = vp()
    _ck(_lib.amg_pattern_ball_device(A.h, int(depth), C.byref(h)))
    return SparseMatOp(h, A.ctx)


def strength_graph_device(A, near_null, weights, block_size=1, depth=1, max_bytes=0, info=False):
    """amg_strength_graph_device_depth: the node-level strength graph at `depth` built
    on the device, as a SparseMatOp without SpMV storage (read it with .arrays() /
    .to_scipy(), pass it to aggregate_mis_device).  near_null: n x k, numpy or a
    column-major torch tensor (host or device).  max_bytes: the budget of the ball
    pattern plus the dof graph at depth > 1 (0: half the free device memory).
    info=True: (graph, dict of _SG_INFO)."""
    if isinstance(near_null, np.ndarray):
        near_null = _colmajor_host(near_null, A.nrows)
    p, m, n, k, ld = _dptr(near_null)
    if n != A.nrows:
        raise ValueError("near-null space must have one row per matrix row")
    w = np.ascontiguousarray(weights, np.float64)
    if len(w) != k:
        raise ValueError("one weight per near-null column")
    h = vp()
    with _ordered(A.ctx, m):
        i6 = np.zeros(6, np.int64)
        _ck(_lib.amg_strength_graph_device_depth(A.h, p, ld, k, w.ctypes.data_as(vp), int(depth), block_size, m,
                                                 int(max_bytes), C.byref(h), i6.ctypes.data_as(vp)))
    G = SparseMatOp(h, A.ctx)
    return (G, dict(zip(_SG_INFO, (int(v) for v in i6)))) if info else G


def aggregate_mis_device(G, max_passes=0):
    """amg_aggregate_mis_device of a square SparseMatOp (a strength_graph_device result
    or an uploaded graph): (agg_of, naggs, info) -- exactly aggregate_mis's aggregates;
    info = {'passes', 'roots', 'singletons', 'fallback'} (fallback: past max_passes,
    0 = the default budget, the host sweep ran on the downloaded graph)."""
    agg = np.zeros(max(G.nrows, 1), np.int64)
    na = i64()
    info = np.zeros(4, np.int64)
    _ck(_lib.amg_aggregate_mis_device(G.h, int(max_passes), agg.ctypes.data_as(vp), C.byref(na),
                                      info.ctypes.data_as(vp)))
    return agg[:G.nrows], na.value, {"passes": int(info[0]), "roots": int(info[1]), "singletons": int(info[2]),
                                     "fallback": bool(info[3])}


class PartitionerConfig(C.Structure):
    """amg_partitioner_config: PartitionerConfig (partitioners/mod.rs:249-329) and the
    device pass budget of one matching round (max_passes, 0 = the default)."""
    _fields_ = [("coarsening_factor", dbl), ("agg_size_penalty", dbl), ("max_improvement_iters", i64),
                ("max_passes", i64)]

    def __init__(self, **kw):
        super().__init__()
        _ck(_lib.amg_partitioner_config_default(C.byref(self)))
        for k, v in kw.items():
            setattr(self, k, v)


_PART_INFO = ("rounds", "passes", "max_passes_in_round", "fallback", "improvement_passes", "swaps", "min_agg",
              "max_agg")


def _part_info(info):
    d = {k: int(v) for k, v in zip(_PART_INFO, info)}
    d["fallback"] = bool(d["fallback"])
    return d


def partition_modularity(G, **cfg):
    """amg_partition_modularity of a strength graph (scipy CSR, ascending columns, no self
    loops): (agg_of, naggs, info) -- aggregates of about coarsening_factor nodes, numbered
    by smallest node.  cfg: PartitionerConfig fields.  info: rounds, passes,
    max_passes_in_round, fallback, improvement_passes, swaps, min_agg, max_agg."""
    G = G.tocsr()
    n = G.shape[0]
    c = PartitionerConfig(**cfg)
    tmp = HostCsr(_host_csr_from_scipy(G))
    agg = np.zeros(max(n, 1), np.int64)
    na = i64()
    info = np.zeros(8, np.int64)
    _ck(_lib.amg_partition_modularity(tmp.h, C.byref(c), agg.ctypes.data_as(vp), C.byref(na),
                                      info.ctypes.data_as(vp)))
    return agg[:n], na.value, _part_info(info)


def partition_modularity_device(G, **cfg):
    """amg_partition_modularity_device of a square SparseMatOp (a strength_graph_device
    result or an uploaded graph): exactly partition_modularity's (agg_of, naggs, info),
    the matching rounds, contractions and swap proposals run on the device."""
    c = PartitionerConfig(**cfg)
    agg = np.zeros(max(G.nrows, 1), np.int64)
    na = i64()
    info = np.zeros(8, np.int64)
    _ck(_lib.amg_partition_modularity_device(G.h, C.byref(c), agg.ctypes.data_as(vp), C.byref(na),
                                             info.ctypes.data_as(vp)))
    return agg[:G.nrows], na.value, _part_info(info)


SA_PARTITIONER = {"mis": 0, "modularity": 1}


def set_sa_partitioner(kind, **cfg):
    """amg_set_sa_partitioner (process-wide): 'mis' / 0 (default) or 'modularity' / 1 with
    PartitionerConfig fields -- what amg_sa_build, find_near_null and adaptive_build run
    on the strength graph."""
    c = PartitionerConfig(**cfg)
    _ck(_lib.amg_set_sa_partitioner(SA_PARTITIONER[kind] if isinstance(kind, str) else int(kind), C.byref(c)))


def get_sa_partitioner():
    """(kind, PartitionerConfig) of amg_get_sa_partitioner."""
    v = i32()
    c = PartitionerConfig()
    _ck(_lib.amg_get_sa_partitioner(C.byref(v), C.byref(c)))
    return v.value, c


class ClassicalConfig(C.Structure):
    """amg_classical_config: LeastSquaresConfig + CompatibleRelaxationConfig
    (interpolation/mod.rs) + the hierarchy fields of SaConfig + where the search runs."""
    _fields_ = [("search_depth", i64), ("depth_ls", i64), ("max_interp", i64), ("tau_threshold", dbl),
                ("target_convergence", dbl), ("relax_steps", i64), ("smoother_coarsening_factor", dbl),
                ("max_cr_iters", i64), ("coarsest_dim", i64), ("max_levels", i64), ("omega", dbl),
                ("smoother", i32), ("chebyshev_steps", i32), ("where", i32), ("reserved", i32)]

    def __init__(self, **kw):
        super().__init__()
        _ck(_lib.amg_classical_config_default(C.byref(self)))
        for k, v in kw.items():
            if k == "smoother" and isinstance(v, str):
                v = SMOOTHERS[v]
            if k == "where" and isinstance(v, str):
                v = SA_SETUP[v]
            setattr(self, k, v)


def cr_mis(G, candidates):
    """amg_cr_mis: the C-points a compatible-relaxation round adds -- the greedy
    independent set of the strength graph G (scipy CSR) among the candidates (n
    booleans), by descending candidate degree, ties to the smaller index.  The chosen
    nodes in the order chosen."""
    G = G.tocsr()
    n = G.shape[0]
    mask = np.ascontiguousarray(np.asarray(candidates).astype(bool), np.uint8)
    if mask.shape != (n,):
        raise ValueError("one candidate flag per node")
    tmp = HostCsr(_host_csr_from_scipy(G))
    out = np.zeros(max(n, 1), np.int64)
    nn_ = i64()
    _ck(_lib.amg_cr_mis(tmp.h, mask.ctypes.data_as(vp), out.ctypes.data_as(vp), C.byref(nn_)))
    return out[:nn_.value].copy()


CR_STOP = {1: "converged", 2: "no_new_c", 3: "max_cr_iters", 4: "zero_vector"}


def cr_split(A, G, **config):
    """amg_cr_split: the compatible-relaxation C/F split of A with the strength graph G
    (scipy CSR): (point_type (0 F, 1 C, 2 N), n_coarse, info) -- info: rounds, reduction,
    stop (a CR_STOP name), c_per_round, c_round (per node: the round that made it a
    C-point, else -1).  config: ClassicalConfig fields (target_convergence, relax_steps,
    smoother_coarsening_factor, max_cr_iters)."""
    cfg = ClassicalConfig(**config)
    G = G.tocsr()
    n = A.nrows
    tmp = HostCsr(_host_csr_from_scipy(G))
    pt = np.zeros(max(n, 1), np.int8)
    cround = np.zeros(max(n, 1), np.int32)
    nc = i64()
    info = np.zeros(3 + max(int(cfg.max_cr_iters), 0))
    _ck(_lib.amg_cr_split(A.h, tmp.h, C.byref(cfg), pt.ctypes.data_as(vp), cround.ctypes.data_as(vp), C.byref(nc),
                          info.ctypes.data_as(vp)))
    rounds = int(info[0])
    return pt[:n], nc.value, {"rounds": rounds, "reduction": float(info[1]), "stop": CR_STOP.get(int(info[2])),
                              "c_per_round": [int(v) for v in info[3:3 + rounds]], "c_round": cround[:n]}


CLASSICAL_INFO_LEVELS = 32
_CLASSICAL_LEVEL = ("rows", "coarse_rows", "cr_rounds", "longest_list", "device_rows", "host_rows", "empty_rows")


def classical_build(A, near_null, weights=None, **config):
    """amg_classical_build: the classical hierarchy (compatible relaxation + least-squares
    interpolation; Hierarchy::coarsen with InterpolationConfig::Classical) as a Multigrid.
    near_null: n x k; weights: k strength weights (None: 1 / v^T A v); config:
    ClassicalConfig fields.  The result's classical_info lists, per coarsening, rows,
    coarse_rows, cr_rounds, longest_list, device_rows, host_rows (rows whose search ran
    on the host: with where 1 the lists beyond the kernel's cap) and empty_rows."""
    cfg = ClassicalConfig(**config)
    nn = _colmajor_host(near_null, A.nrows)
    w = None if weights is None else np.ascontiguousarray(weights, np.float64)
    h = vp()
    info = np.zeros(1 + 7 * CLASSICAL_INFO_LEVELS, np.int64)
    _ck(_lib.amg_classical_build(A.h, nn.ctypes.data_as(vp), nn.shape[0], nn.shape[1],
                                 None if w is None else w.ctypes.data_as(vp), C.byref(cfg), C.byref(h),
                                 info.ctypes.data_as(vp)))
    mg = Multigrid._from_handle(h, A.ctx)
    mg.classical_info = [dict(zip(_CLASSICAL_LEVEL, (int(v) for v in info[1 + 7 * l:8 + 7 * l])))
                         for l in range(min(int(info[0]), CLASSICAL_INFO_LEVELS))]
    return mg


def ls_candidates(A, point_type, depth):
    """amg_ls_candidates: per non-C row the C-points (point_type 1) within BFS depth
    `depth` of the pattern of A, ascending, as a scipy CSR of unit values."""
    pt = np.ascontiguousarray(point_type, np.int8)
    if pt.shape != (A.nrows,):
        raise ValueError("one point type per row")
    h = vp()
    _ck(_lib.amg_ls_candidates(A.h, pt.ctypes.data_as(vp), int(depth), C.byref(h)))
    return HostCsr(h).to_scipy()


def ls_search(lists, near_null, weights, max_interp=3, where=0, ctx=None, max_list=0):
    """amg_ls_search: the best interpolation subset of each size 1..max_interp for every
    row of `lists` (scipy CSR n x n, columns = candidate C-points).  where: 0 / 'host'
    or 1 / 'device' (needs ctx).  Returns (count (n, mi) int32, cols (n, mi, mi) int64,
    w (n, mi, mi), err (n, mi), info) -- the same bits on either path; info: device_rows,
    host_rows, longest_list, subsets."""
    lists = lists.tocsr()
    lists.sort_indices()
    n = lists.shape[0]
    nn = _colmajor_host(near_null, n)
    k = nn.shape[1]
    wts = np.ascontiguousarray(weights, np.float64)
    if len(wts) != k:
        raise ValueError("one weight per near-null column")
    mi = int(max_interp)
    m = max(mi, 1)
    count = np.zeros((max(n, 1), m), np.int32)
    cols = np.zeros((max(n, 1), m, m), np.int64)
    w = np.zeros((max(n, 1), m, m), np.float64)
    err = np.zeros((max(n, 1), m), np.float64)
    info = np.zeros(4, np.int64)
    tmp = HostCsr(_host_csr_from_scipy(lists))
    where = SA_SETUP[where] if isinstance(where, str) else int(where)
    _ck(_lib.amg_ls_search(None if ctx is None else ctx.h, tmp.h, nn.ctypes.data_as(vp), nn.shape[0], k,
                           wts.ctypes.data_as(vp), mi, where, int(max_list), count.ctypes.data_as(vp),
                           cols.ctypes.data_as(vp), w.ctypes.data_as(vp), err.ctypes.data_as(vp),
                           info.ctypes.data_as(vp)))
    return count[:n], cols[:n], w[:n], err[:n], {"device_rows": int(info[0]), "host_rows": int(info[1]),
                                                 "longest_list": int(info[2]), "subsets": int(info[3])}


def ls_accept(near_null, weights, count, err, tau=1.2):
    """amg_ls_accept: the accepted size per row (0: an empty row) from ls_search's count
    and err by the reference's rule err_r < pow(accepted err, tau * (r - accepted size))."""
    count = np.ascontiguousarray(count, np.int32)
    err = np.ascontiguousarray(err, np.float64)
    n, mi = count.shape
    nn = _colmajor_host(near_null, n)
    wts = np.ascontiguousarray(weights, np.float64)
    chosen = np.zeros(max(n, 1), np.int32)
    _ck(_lib.amg_ls_accept(n, nn.ctypes.data_as(vp), nn.shape[0], nn.shape[1], wts.ctypes.data_as(vp), mi,
                           float(tau), count.ctypes.data_as(vp), err.ctypes.data_as(vp), chosen.ctypes.data_as(vp)))
    return chosen[:n]


def ls_interpolation(A, point_type, near_null, weights, **config):
    """amg_ls_interpolation: classical interpolation for a given C/F split (point_type: 0
    F, 1 C, 2 N): (P, coarse near-null (n_coarse x k), row_err).  config: ClassicalConfig
    fields (depth_ls, search_depth, max_interp, tau_threshold, where).  P.ls_info: device_rows,
    host_rows, longest_list, subsets, empty_rows of the search."""
    cfg = ClassicalConfig(**config)
    pt = np.ascontiguousarray(point_type, np.int8)
    if pt.shape != (A.nrows,):
        raise ValueError("one point type per row")
    nn = _colmajor_host(near_null, A.nrows)
    k = nn.shape[1]
    wts = np.ascontiguousarray(weights, np.float64)
    if len(wts) != k:
        raise ValueError("one weight per near-null column")
    nc = int((pt == 1).sum())
    cnn = np.zeros((max(nc, 1), k), order="F")
    rerr = np.zeros(max(A.nrows, 1))
    h = vp()
    info = np.zeros(5, np.int64)
    _ck(_lib.amg_ls_interpolation(A.h, pt.ctypes.data_as(vp), nn.ctypes.data_as(vp), nn.shape[0], k,
                                  wts.ctypes.data_as(vp), C.byref(cfg), C.byref(h), cnn.ctypes.data_as(vp),
                                  rerr.ctypes.data_as(vp), info.ctypes.data_as(vp)))
    P_ = SparseMatOp(h, A.ctx)
    P_.ls_info = dict(zip(("device_rows", "host_rows", "longest_list", "subsets", "empty_rows"), (int(v) for v in info)))
    return P_, cnn[:nc], rerr[:A.nrows]


def _host_csr_from_scipy(G):
    G = G.tocsr()
    rp = np.ascontiguousarray(G.indptr, np.int64)
    ci = np.ascontiguousarray(G.indices, np.int64)
    va = np.ascontiguousarray(G.data, np.float64)
    h = vp()
    _ck(_lib.amg_host_csr_create(G.shape[0], G.shape[1], rp.ctypes.data_as(vp), ci.ctypes.data_as(vp),
                                 va.ctypes.data_as(vp), C.byref(h)))
    return h


def sa_tentative_block(ctx, agg_of, naggs, near_null, block_size=1, candidate_dimension=None):
    """Tentative SA interpolation for k candidates (interpolation/mod.rs:754-805):
    returns (P, coarse near-null (naggs*cd) x k)."""
    agg = np.ascontiguousarray(agg_of, np.int64)
    nn = _colmajor_host(near_null, len(agg) * block_size)
    k = nn.shape[1]
    cd = k if candidate_dimension is None else candidate_dimension
    cnn = np.zeros((naggs * cd, k), order="F")
    h = vp()
    _ck(_lib.amg_sa_tentative_block(ctx.h, len(agg), block_size, agg.ctypes.data_as(vp), naggs,
                                    nn.ctypes.data_as(vp), nn.shape[0], k, cd, C.byref(h),
                                    cnn.ctypes.data_as(vp)))
    return SparseMatOp(h, ctx), cnn


def block_jacobi(A, P_, block_size, omega=0.66):
    """block_jacobi P smoothing (interpolation/mod.rs:963-1028)."""
    h = vp()
    _ck(_lib.amg_block_jacobi_smooth(A.h, P_.h, block_size, omega, C.byref(h)))
    return SparseMatOp(h, A.ctx)


def nn_postprocess(A, x, iters=3):
    """Coarse near-null post-processing for k columns (hierarchy.rs:219-228)."""
    x = np.array(_colmajor_host(x, A.nrows), copy=True, order="F")
    _ck(_lib.amg_nn_postprocess(A.h, iters, x.ctypes.data_as(vp), x.shape[0], x.shape[1]))
    return x


def elasticity_q1(elements, contrast=1.0, nu=0.3, seed=42, permute=True):
    """Host CSR of the C5 stand-in: Q1 hex elasticity, block size 3 (gen.cpp).
    permute: False none, True over all nodes, an int W >= 2 within windows of W nodes."""
    ex, ey, ez = elements
    mode = 0 if permute is False else 1 if permute is True else int(permute)
    h = vp()
    _ck(_lib.amg_gen_elasticity_q1(ex, ey, ez, contrast, nu, seed, mode, C.byref(h)))
    return HostCsr(h)


def constant_candidates(n, block_size):
    """block_size constant-per-component near-null vectors, orthonormal (n x bs)."""
    nn = np.zeros((n, block_size), order="F")
    for c in range(block_size):
        nn[c::block_size, c] = 1.0
    return nn / np.sqrt(n // block_size)


def _block_copy(X):
    """A writable column-major copy of an n x k block (numpy or torch), same kind."""
    try:
        import torch
        if isinstance(X, torch.Tensor):
            if X.dim() == 1:
                X = X[:, None]
            return X.t().clone(memory_format=torch.contiguous_format).t()
    except ImportError:
        pass
    X = np.asarray(X, np.float64)
    if X.ndim == 1:
        X = X[:, None]
    return np.array(X, order="F", copy=True)


def thin_qr(ctx, X, in_place=False):
    """Thin QR of a column-major n x k block, k <= 64 (amg_thin_qr; the search's
    x.qr().compute_thin_Q(), adaptivity.rs:329): returns (Q, R), R a k x k numpy
    array with a positive diagonal.  in_place: X itself is overwritten by Q."""
    Q = X if in_place else _block_copy(X)
    p, m, n, k, ld = _dptr(Q)
    R = np.zeros((k, k), order="F")
    with _ordered(ctx, m):
        _ck(_lib.amg_thin_qr(ctx.h, p, ld, n, k, R.ctypes.data_as(vp), m))
    return Q, R


def smooth_vectors(A, pc, k=None, iters=50, seed=None, X0=None):
    """smooth_vector (adaptivity.rs:307-390): `iters` error-propagation steps
    X <- thinQ(X - pc(A X)) from the start block X0 (n x k, numpy or torch; left
    unchanged), or from default_rng(seed).standard_normal((n, k)).  Returns
    (X, cfs): the basis and the A-norm convergence factor of each column."""
    if X0 is None:
        if k is None:
            raise ValueError("give k or a start block X0")
        X = np.asfortranarray(np.random.default_rng(seed).standard_normal((A.nrows, k)))
    else:
        X = _block_copy(X0)
    p, m, n, kk, ld = _dptr(X)
    if n != A.nrows or (k is not None and k != kk):
        raise ValueError("the start block must be nrows x k")
    cfs = np.zeros(kk)
    with _ordered(A.ctx, m):
        _ck(_lib.amg_smooth_vectors(A.h, pc.h, p, ld, kk, iters, cfs.ctypes.data_as(vp), m))
    return X, cfs


def create_weights(A, X):
    """create_weights (adaptivity.rs:434-443): 1 / (x_c^T A x_c) per column."""
    if isinstance(X, np.ndarray):
        X = _colmajor_host(X, A.nrows)
    p, m, n, k, ld = _dptr(X)
    if n != A.nrows:
        raise ValueError("the block must have one row per matrix row")
    w = np.zeros(k)
    with _ordered(A.ctx, m):
        _ck(_lib.amg_create_weights(A.h, p, ld, k, w.ctypes.data_as(vp), m))
    return w


def find_near_null(A, k, iters=50, seed=0, block_size=1, strength_depth=1, X0=None):
    """find_near_null (adaptivity.rs:264-305): the two-stage search (L1, then a
    BlockSmoother over the strength graph's aggregates) from the start block
    default_rng(seed).standard_normal((n, k)) (or X0).  Returns (X, cfs) of stage 2."""
    if X0 is None:
        X = np.asfortranarray(np.random.default_rng(seed).standard_normal((A.nrows, k)))
    else:
        X = _block_copy(X0)
    p, m, n, kk, ld = _dptr(X)
    if n != A.nrows or kk != k:
        raise ValueError("the start block must be nrows x k")
    cfs = np.zeros(k)
    with _ordered(A.ctx, m):
        _ck(_lib.amg_find_near_null(A.h, p, ld, k, iters, block_size, strength_depth,
                                    cfs.ctypes.data_as(vp), m))
    return X, cfs


class AdaptiveConfig(C.Structure):
    """amg_adaptive_config: AdaptiveConfig (adaptivity.rs) -- the SaConfig fields of
    every hierarchy plus max_components and test_iters."""
    _fields_ = [("sa", SaConfig), ("max_components", i64), ("test_iters", i64)]

    def __init__(self, **kw):
        super().__init__()
        _ck(_lib.amg_adaptive_config_default(C.byref(self)))
        sa_fields = {name for name, _ in SaConfig._fields_}
        for k, v in kw.items():
            if k in ("max_components", "test_iters"):
                setattr(self, k, v)
            elif k in sa_fields:
                if k == "smoother" and isinstance(v, str):
                    v = SMOOTHERS[v]
                setattr(self.sa, k, v)
            else:
                raise TypeError(f"AdaptiveConfig has no option {k!r}")


def adaptive_build(A, dim=32, seed=0, X0=None, **config):
    """AdaptiveConfig::build (adaptivity.rs:55-165, amg_adaptive_build): near-null
    search, a first SA hierarchy, then max_components - 1 rounds of smoothing the
    start block with the composite built so far and building a hierarchy from what
    survives.  The start block is default_rng(seed).standard_normal((n, dim)) or X0
    (host, n x dim).  config: AdaptiveConfig fields (max_components, test_iters and
    the SaConfig ones).  Returns (Composite, cfs) with cfs (max_components - 1) x dim."""
    cfg = AdaptiveConfig(**config)
    n = A.nrows
    if X0 is None:
        X = np.asfortranarray(np.random.default_rng(seed).standard_normal((n, dim)))
    else:
        X = _colmajor_host(X0, n)
    if X.shape[1] != dim:
        raise ValueError("the start block must be nrows x dim")
    cfs = np.zeros((max(cfg.max_components - 1, 0), dim))
    h = vp()
    _ck(_lib.amg_adaptive_build(A.h, X.ctypes.data_as(vp), X.shape[0], dim, C.byref(cfg),
                                cfs.ctypes.data_as(vp), C.byref(h)))
    comp = Composite.__new__(Composite)
    LinOp.__init__(comp, h, A.ctx, refs=(A,))
    return comp, cfs


def stationary_solve(A, M, b, x, max_iter=100, rel_tol=1e-8):
    """examples/simple_geometric.rs:117-158 on device vectors; returns (iters, hist)."""
    hist = np.zeros(max_iter)
    it = i64()
    with _ordered(A.ctx, AMG_MEM_DEVICE):
        _ck(_lib.amg_stationary_solve(A.h, M.h, vp(b.data_ptr()), vp(x.data_ptr()), max_iter,
                                      rel_tol, hist.ctypes.data_as(vp), C.byref(it)))
    return it.value, hist[:it.value]


def pcg_solve(A, M, b, x, max_iter=1000, rel_tol=1e-8, abs_tol=0.0):
    hist = np.zeros(max(max_iter, 1))
    it = i64()
    with _ordered(A.ctx, AMG_MEM_DEVICE):
        _ck(_lib.amg_pcg_solve(A.h, None if M is None else M.h, vp(b.data_ptr()),
                               vp(x.data_ptr()), max_iter, rel_tol, abs_tol,
                               hist.ctypes.data_as(vp), C.byref(it)))
    return it.value, hist[:min(it.value, max_iter)]


def _solve_blocks(B, X):
    """Pointers, k and leading dimensions of the column-major device blocks B, X."""
    pb, memb, nb, kb, ldb = _dptr(B)
    px, memx, nx, kx, ldx = _dptr(X)
    if (nb, kb) != (nx, kx):
        raise ValueError("B and X must have equal shapes")
    if memb != AMG_MEM_DEVICE or memx != AMG_MEM_DEVICE:
        raise ValueError("B and X must be device tensors")
    return pb, ldb, px, ldx, kb


def pcg_solve_block(A, M, B, X, max_iter=1000, rel_tol=1e-8, abs_tol=0.0):
    """amg_pcg_solve_block: the k columns of B (column-major n x k device tensor,
    stride(0) == 1) through pcg_solve's loop at once, X in/out.  Every column is
    bitwise pcg_solve of that column (independent recurrences; the matrix and the
    hierarchy are streamed once per 8 columns).  Returns (iters[k], [hist per column])."""
    pb, ldb, px, ldx, k = _solve_blocks(B, X)
    ldh = max(max_iter, 1)
    hist = np.zeros((ldh, max(k, 1)), order="F")
    iters = np.zeros(max(k, 1), np.int64)
    with _ordered(A.ctx, AMG_MEM_DEVICE):
        _ck(_lib.amg_pcg_solve_block(A.h, None if M is None else M.h, pb, ldb, px, ldx, k, max_iter, rel_tol,
                                     abs_tol, hist.ctypes.data_as(vp), ldh, iters.ctypes.data_as(vp)))
    return iters[:k], [hist[:min(int(iters[c]), max_iter), c].copy() for c in range(k)]


def stationary_solve_block(A, M, B, X, max_iter=100, rel_tol=1e-8):
    """amg_stationary_solve_block: stationary_solve on the k columns of B at once,
    every column bitwise that call.  Returns (iters[k], [hist per column])."""
    pb, ldb, px, ldx, k = _solve_blocks(B, X)
    ldh = max(max_iter, 1)
    hist = np.zeros((ldh, max(k, 1)), order="F")
    iters = np.zeros(max(k, 1), np.int64)
    with _ordered(A.ctx, AMG_MEM_DEVICE):
        _ck(_lib.amg_stationary_solve_block(A.h, M.h, pb, ldb, px, ldx, k, max_iter, rel_tol,
                                            hist.ctypes.data_as(vp), ldh, iters.ctypes.data_as(vp)))
    return iters[:k], [hist[:int(iters[c]), c].copy() for c in range(k)]


def block_cg_solve(A, M, B, X, max_iter=1000, rel_tol=1e-8, abs_tol=0.0, rank_tol=0.0):
    """amg_block_cg_solve: the coupled block CG on the k <= 32 columns of B
    (column-major n x k device tensors, X in/out) -- what faer's conjugate_gradient
    does with an n x k rhs: one k x k system for the step and one for the new
    directions per iteration, fewer iterations than the slowest column alone.
    Returns (iters, hist[:m], ranks[:m]) with m = min(iters, max_iter): one count
    for the block, hist m x k relative residuals, ranks the directions kept."""
    pb, ldb, px, ldx, k = _solve_blocks(B, X)
    ldh = max(max_iter, 1)
    hist = np.zeros((ldh, max(k, 1)), order="F")
    ranks = np.zeros(ldh, np.int64)
    it = i64()
    with _ordered(A.ctx, AMG_MEM_DEVICE):
        _ck(_lib.amg_block_cg_solve(A.h, None if M is None else M.h, pb, ldb, px, ldx, k, max_iter, rel_tol, abs_tol,
                                    rank_tol, hist.ctypes.data_as(vp), ldh, ranks.ctypes.data_as(vp), C.byref(it)))
    m = min(it.value, max_iter)
    return it.value, hist[:m, :k].copy(), ranks[:m].copy()


def _device_block(X):
    p, mem, n, k, ld = _dptr(X)
    if mem != AMG_MEM_DEVICE:
        raise ValueError("blocks must be device tensors")
    return p, n, k, ld


def block_gram(ctx, X, Y1, Y2=None):
    """amg_block_gram: X^T [Y1 | Y2] of column-major device blocks (at most 32
    columns each) as a w x (m1 + m2) numpy array; fp64 matrix cores, fixed order."""
    px, n, w, ldx = _device_block(X)
    p1, n1, m1, ld1 = _device_block(Y1)
    p2, n2, m2, ld2 = _device_block(Y2) if Y2 is not None else (None, n, 0, n)
    if n1 != n or n2 != n:
        raise ValueError("the blocks must have equal row counts")
    out = np.zeros((w, m1 + m2), order="F")
    with _ordered(ctx, AMG_MEM_DEVICE):
        _ck(_lib.amg_block_gram(ctx.h, px, ldx, w, p1, ld1, m1, p2, ld2, m2, n, out.ctypes.data_as(vp)))
    return out


def block_gemm_update(ctx, Y, X, Cm, sign=1):
    """amg_block_gemm_update: Y <- Y + sign * X Cm in place (X n x w, Y n x m
    column-major device blocks, Cm a host w x m array; sign +1 or -1)."""
    py, n, m, ldy = _device_block(Y)
    px, nx, w, ldx = _device_block(X)
    Cm = np.asfortranarray(Cm, dtype=np.float64)
    if nx != n or Cm.shape != (w, m):
        raise ValueError("need X n x w, Cm w x m and Y n x m")
    with _ordered(ctx, AMG_MEM_DEVICE):
        _ck(_lib.amg_block_gemm_update(ctx.h, py, ldy, px, ldx, Cm.ctypes.data_as(vp), w, m, n, sign))


class BlockSmoother(LinOp):
    """BlockSmoother (block_smoothers.rs:80-291): block Jacobi over a node
    partition, diagonally compensated blocks solved exactly."""

    def __init__(self, A, node_partition, naggregates=None, block_size=1):
        part = np.ascontiguousarray(node_partition, np.int64)
        nagg = int(part.max()) + 1 if naggregates is None else int(naggregates)
        h = vp()
        _ck(_lib.amg_block_smoother_create(A.h, part.ctypes.data_as(vp), nagg, int(block_size),
                                           C.byref(h)))
        super().__init__(h, A.ctx, refs=(A,))

    def to_sparse(self):
        """BlockSmoother::into_sparse_mat: the block-diagonal inverse as a SparseMatOp."""
        h = vp()
        _ck(_lib.amg_block_smoother_to_csr(self.h, C.byref(h)))
        return SparseMatOp(h, self.ctx)

    def info(self):
        """amg_block_smoother_info: blocks, chunks, inverse bytes and the chunks per
        column width of the k-wide apply (flag block_smoother_cols)."""
        out = (i64 * 8)()
        _ck(_lib.amg_block_smoother_info(self.h, out))
        return {"nblocks": out[0], "max_block": out[1], "nchunks": out[2], "inverse_bytes": out[3],
                "chunks_by_width": {8: out[4], 4: out[5], 2: out[6], 1: out[7]}}


class Composite(LinOp):
    """Composite (preconditioners/composite.rs): components c_0..c_{m-1} applied
    c_{m-1}..c_1, c_0, c_1..c_{m-1}, each step out += c(r); r = rhs - A out."""

    def __init__(self, A, components):
        comps = list(components)
        arr = (vp * len(comps))(*[c.h for c in comps])
        h = vp()
        _ck(_lib.amg_composite_create(A.h, arr, len(comps), C.byref(h)))
        super().__init__(h, A.ctx, refs=(A, *comps))

    def push(self, component):
        _ck(_lib.amg_composite_push(self.h, component.h))
        self._refs = tuple(self._refs) + (component,)
        return self

    def ncomponents(self):
        v = i64()
        _ck(_lib.amg_composite_ncomponents(self.h, C.byref(v)))
        return v.value


# ------------------------------------------------------------------ multi-GPU

def rccl_library():
    """Path of the librccl the library bound to ('' if none could be loaded)."""
    return _lib.amg_rccl_library().decode()


def unique_id():
    """ncclUniqueId bytes (create on rank 0, broadcast out of band)."""
    n = _lib.amg_comm_unique_id_size()
    buf = (C.c_char * n)()
    _ck(_lib.amg_comm_get_unique_id(buf))
    return bytes(buf)


class LoopbackHub:
    """In-process transport hub: `nranks` virtual ranks driven by host threads."""

    def __init__(self, nranks):
        h = vp()
        _ck(_lib.amg_loopback_hub_create(nranks, C.byref(h)))
        self.h = h
        self.nranks = nranks

    def __del__(self, _destroy=_lib.amg_loopback_hub_destroy):
        if getattr(self, "h", None):
            _destroy(self.h)
            self.h = None


class Comm:
    """Per-process communicator: RCCL (`uid` from unique_id()) or loopback (`hub`)."""

    def __init__(self, ctx, nranks=None, rank=0, uid=None, hub=None):
        h = vp()
        if hub is not None:
            _ck(_lib.amg_comm_create_loopback(ctx.h, hub.h, rank, C.byref(h)))
            self._hub = hub
        else:
            buf = (C.c_char * len(uid)).from_buffer_copy(uid)
            _ck(_lib.amg_comm_create(ctx.h, nranks, rank, buf, C.byref(h)))
        self.h = h
        self.ctx = ctx
        r, n = i32(), i32()
        _ck(_lib.amg_comm_rank(h, C.byref(r), C.byref(n)))
        self.rank, self.nranks = r.value, n.value

    def barrier(self):
        _ck(_lib.amg_comm_barrier(self.h))

    def allreduce_max(self, v):
        d = dbl(v)
        _ck(_lib.amg_comm_allreduce_max(self.h, C.byref(d)))
        return d.value

    def allreduce_sum(self, v):
        d = dbl(v)
        _ck(_lib.amg_comm_allreduce_sum(self.h, C.byref(d)))
        return d.value

    def __del__(self, _destroy=_lib.amg_comm_destroy):
        if getattr(self, "h", None):
            _destroy(self.h)
            self.h = None


class DistMultigrid(LinOp):
    """Row-block distributed V-cycle built from a global multigrid on this rank.

    level_splits: list (one per level) of nranks+1 row splits."""

    def __init__(self, comm, mg_global, level_splits, agglomerate_rows=1 << 16):
        s = np.ascontiguousarray(np.concatenate([np.asarray(x, np.int64) for x in level_splits]))
        h = vp()
        _ck(_lib.amg_dist_multigrid_create(comm.h, mg_global.h, s.ctypes.data_as(vp),
                                           int(agglomerate_rows), C.byref(h)))
        super().__init__(h, comm.ctx)
        self.comm = comm
        self.nlevels = len(level_splits)

    def local_rows(self):
        b, e = i64(), i64()
        _ck(_lib.amg_dist_local_rows(self.h, C.byref(b), C.byref(e)))
        return b.value, e.value

    def level_info(self, l):
        info = np.zeros(6, np.int64)
        _ck(_lib.amg_dist_level_info(self.h, l, info.ctypes.data_as(vp)))
        keys = ("n_own", "n_ghost", "n_neighbors", "redundant", "halo_recv", "n_global")
        return dict(zip(keys, (int(v) for v in info)))

    def level_operator(self, l):
        h = vp()
        _ck(_lib.amg_dist_level_operator(self.h, l, C.byref(h)))
        return LinOp(h, self.ctx, refs=(self,))

    def level_matrix(self, l, which="A"):
        """This rank's local CSR of level l (owned rows, [owned | ghost] columns)."""
        h = vp()
        _ck(_lib.amg_dist_level_matrix(self.h, l, {"A": 0, "R": 1, "P": 2}[which], C.byref(h)))
        return SparseMatOp(h, self.ctx, refs=(self,))

    def set_overlap(self, on=True):
        """Overlap halo exchanges with the interior rows of their SpMV (default on)."""
        _ck(_lib.amg_dist_set_option(self.h, 0, 1 if on else 0))
        return self

    def cycle_plan(self, cap=4096):
        """The launches of one distributed V-cycle on this rank (amg_dist_cycle_plan;
        collective: every rank calls it), as Multigrid.cycle_plan."""
        n = i64()
        recs = (LaunchRec * cap)()
        _ck(_lib.amg_dist_cycle_plan(self.h, recs, cap, C.byref(n)))
        return [{"level": r.level, "role": ROLES.get(r.role, "?"), "kernel": r.kernel,
                 "mode": MODES.get(r.mode, "?"), "name": r.name.decode(), "rows": r.rows,
                 "bytes": r.bytes, "csr_bytes": r.csr_bytes} for r in recs[:min(cap, n.value)]]

    def set_graph(self, on=True):
        """hipGraph replay of the distributed cycle (RCCL communicators only; default off)."""
        _ck(_lib.amg_dist_set_option(self.h, 1, 1 if on else 0))
        return self

    def set_per_colour_halo(self, on=True):
        """SGS levels: exchange only the colour swept last before each colour (default on)."""
        _ck(_lib.amg_dist_set_option(self.h, 2, 1 if on else 0))
        return self

    def pcg_solve(self, b, x, max_iter=1000, rel_tol=1e-8, abs_tol=0.0, precondition=True):
        """Distributed PCG (dots all-reduced), one distributed V-cycle per iteration."""
        hist = np.zeros(max(max_iter, 1))
        it = i64()
        with _ordered(self.ctx, AMG_MEM_DEVICE):
            _ck(_lib.amg_dist_pcg_solve(self.h, 1 if precondition else 0, vp(b.data_ptr()),
                                        vp(x.data_ptr()), max_iter, rel_tol, abs_tol,
                                        hist.ctypes.data_as(vp), C.byref(it)))
        return it.value, hist[:min(it.value, max_iter)]

    def stationary_solve(self, b, x, max_iter=100, rel_tol=1e-8):
        hist = np.zeros(max_iter)
        it = i64()
        with _ordered(self.ctx, AMG_MEM_DEVICE):
            _ck(_lib.amg_dist_stationary_solve(self.h, vp(b.data_ptr()), vp(x.data_ptr()),
                                               max_iter, rel_tol, hist.ctypes.data_as(vp),
                                               C.byref(it)))
        return it.value, hist[:it.value]


def _i64(a):
    return np.ascontiguousarray(a, np.int64)


class HaloPlan:
    """Host-side halo plan of one level on one rank (amg_halo_plan_*; no device):
    the library's own planner, driven step by step so any process layout (a gloo
    test, a custom launcher) can exchange the requests itself."""

    def __init__(self, nranks, rank, splits):
        sp_ = _i64(splits)
        if len(sp_) != nranks + 1:
            raise ValueError("splits must have nranks + 1 entries")
        h = vp()
        _ck(_lib.amg_halo_plan_create(nranks, rank, sp_.ctypes.data_as(vp), C.byref(h)))
        self.h, self.nranks, self.rank = h, nranks, rank

    def __del__(self, _destroy=_lib.amg_halo_plan_destroy):
        if getattr(self, "h", None):
            _destroy(self.h)
            self.h = None

    def add_columns(self, cols):
        c = _i64(cols)
        _ck(_lib.amg_halo_plan_add_columns(self.h, len(c), c.ctypes.data_as(vp)))

    def requests(self):
        """(ghost ids sorted, ids to request from each rank as a list of arrays)."""
        cnt = np.zeros(self.nranks, np.int64)
        ng = i64()
        _ck(_lib.amg_halo_plan_requests(self.h, cnt.ctypes.data_as(vp), C.byref(ng)))
        ids = np.zeros(max(1, ng.value), np.int64)
        _ck(_lib.amg_halo_plan_ghost_ids(self.h, ids.ctypes.data_as(vp)))
        ids = ids[:ng.value]
        off = np.concatenate([[0], np.cumsum(cnt)])
        return ids, [ids[off[q]:off[q + 1]] for q in range(self.nranks)]

    def set_incoming(self, per_rank_ids):
        cnt = _i64([len(x) for x in per_rank_ids])
        ids = _i64(np.concatenate([np.asarray(x, np.int64) for x in per_rank_ids] + [np.zeros(0, np.int64)]))
        _ck(_lib.amg_halo_plan_set_incoming(self.h, cnt.ctypes.data_as(vp),
                                            ids.ctypes.data_as(vp) if len(ids) else None))

    def info(self):
        v = np.zeros(6, np.int64)
        _ck(_lib.amg_halo_plan_info(self.h, v.ctypes.data_as(vp)))
        return dict(zip(("n_own", "n_ghost", "neighbors", "nsend", "nrecv", "r0"), (int(x) for x in v)))

    def neighbors(self):
        k = self.info()["neighbors"]
        nbr = np.zeros(max(1, k), np.int32)
        arrs = [np.zeros(max(1, k), np.int64) for _ in range(4)]
        _ck(_lib.amg_halo_plan_neighbors(self.h, nbr.ctypes.data_as(vp), *[a.ctypes.data_as(vp) for a in arrs]))
        return {"nbr": nbr[:k], "soff": arrs[0][:k], "scnt": arrs[1][:k], "roff": arrs[2][:k], "rcnt": arrs[3][:k]}

    def send_indices(self):
        n = self.info()["nsend"]
        idx = np.zeros(max(1, n), np.int32)
        _ck(_lib.amg_halo_plan_send_indices(self.h, idx.ctypes.data_as(vp)))
        return idx[:n]

    def remap(self, M):
        """scipy CSR with global columns -> (CSR with [owned | ghost] columns, lo, hi)."""
        import scipy.sparse as sps
        M = M.tocsr()
        rp, ci = _i64(M.indptr), _i64(M.indices)
        out = np.zeros(max(1, len(ci)), np.int32)
        lo, hi = i64(), i64()
        _ck(_lib.amg_halo_plan_remap(self.h, M.shape[0], rp.ctypes.data_as(vp), ci.ctypes.data_as(vp),
                                     out.ctypes.data_as(vp), C.byref(lo), C.byref(hi)))
        inf = self.info()
        L = sps.csr_matrix((M.data.copy(), out[:len(ci)].astype(np.int64), rp.copy()),
                           shape=(M.shape[0], inf["n_own"] + inf["n_ghost"]))
        return L, lo.value, hi.value


def first_redundant_level(level_rows, agglomerate_rows):
    """The first level the distributed multigrid gathers and cycles redundantly."""
    r = _i64(level_rows)
    v = i64()
    _ck(_lib.amg_dist_first_redundant_level(len(r), r.ctypes.data_as(vp), agglomerate_rows, C.byref(v)))
    return v.value


def slab_splits(level_dims, nranks):
    """Row splits per level for a z-slab partition of box-coarsened grids:
    rank p owns planes [floor(p*nz/P), floor((p+1)*nz/P)) of every level."""
    out = []
    for (nx, ny, nz) in level_dims:
        planes = [(p * nz) // nranks for p in range(nranks + 1)]
        out.append([z * nx * ny for z in planes])
    return out


def box_level_dims(dims, box, nlevels):
    d = [tuple(dims)]
    for _ in range(nlevels - 1):
        d.append(tuple(-(-a // b) for a, b in zip(d[-1], box)))
    return d


# ------------------------------------------------------------------ loaders

class HostCsr:
    """Host CSR from a loader (int64 row pointers / columns, f64 values)."""

    def __init__(self, h, owner=None):
        self.h = h
        self._owner = owner  # borrowed from an MfemSystem when set

    def __del__(self, _destroy=_lib.amg_host_csr_destroy):
        if getattr(self, "h", None) and self._owner is None:
            _destroy(self.h)
            self.h = None

    def dims(self):
        m, n, z = i64(), i64(), i64()
        _ck(_lib.amg_host_csr_dims(self.h, C.byref(m), C.byref(n), C.byref(z)))
        return m.value, n.value, z.value

    def arrays(self):
        m, _, z = self.dims()
        rp = np.zeros(m + 1, np.int64)
        ci = np.zeros(z, np.int64)
        va = np.zeros(z, np.float64)
        _ck(_lib.amg_host_csr_arrays(self.h, rp.ctypes.data_as(vp), ci.ctypes.data_as(vp),
                                     va.ctypes.data_as(vp)))
        return rp, ci, va

    def to_scipy(self):
        import scipy.sparse as sps
        m, n, _ = self.dims()
        rp, ci, va = self.arrays()
        return sps.csr_matrix((va, ci, rp), shape=(m, n))

    def upload(self, ctx):
        h = vp()
        _ck(_lib.amg_host_csr_upload(ctx.h, self.h, C.byref(h)))
        return SparseMatOp(h, ctx)


def read_mtx(path):
    """Matrix Market coordinate file -> HostCsr (utils.rs:508-534 semantics)."""
    h = vp()
    _ck(_lib.amg_mtx_read(os.fsencode(path), C.byref(h)))
    return HostCsr(h)


class MfemSystem:
    """dir/name.{mtx,bdy,coords,rhs} (load_mfem_linear_system, utils.rs:269-350)."""

    def __init__(self, directory, name, delete_boundary=True):
        h = vp()
        _ck(_lib.amg_mfem_load(os.fsencode(directory), os.fsencode(name),
                               1 if delete_boundary else 0, C.byref(h)))
        self.h = h
        info = np.zeros(5, np.int64)
        _ck(_lib.amg_mfem_info(self.h, info.ctypes.data_as(vp)))
        self.n, self.rhs_cols, self.coord_dim, self.original_dim, nb = (int(v) for v in info)
        mh = vp()
        _ck(_lib.amg_mfem_matrix(self.h, C.byref(mh)))
        self.matrix = HostCsr(mh, owner=self)
        self.rhs = np.zeros((self.n, self.rhs_cols), order="F")
        self.coords = np.zeros((self.n, self.coord_dim), order="F")
        self.boundary = np.zeros(nb, np.int64)
        self.solution_to_mesh = np.zeros(self.n, np.int64)
        self.mesh_to_solution = np.zeros(self.original_dim, np.int64)
        _ck(_lib.amg_mfem_rhs(self.h, self.rhs.ctypes.data_as(vp), max(1, self.n)))
        _ck(_lib.amg_mfem_coords(self.h, self.coords.ctypes.data_as(vp), max(1, self.n)))
        _ck(_lib.amg_mfem_boundary(self.h, self.boundary.ctypes.data_as(vp)))
        _ck(_lib.amg_mfem_index_maps(self.h, self.solution_to_mesh.ctypes.data_as(vp),
                                     self.mesh_to_solution.ctypes.data_as(vp)))

    def __del__(self, _destroy=_lib.amg_mfem_destroy):
        if getattr(self, "h", None):
            _destroy(self.h)
            self.h = None
