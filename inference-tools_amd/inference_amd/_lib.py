"""
ctypes binding of libgpmi.so (C-ABI declared in include/gpmi.h).

The library is built in-tree by `__graft_entry__.build()` / `make -C
inference-tools_amd/csrc` into `inference_amd/lib/libgpmi.so`.  Nothing here
falls back to a CPU implementation: a missing library or device raises
`GpmiUnavailable`.
"""
import atexit
import ctypes as C
import os
import sys
import weakref

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# GPMI_LIB: another build of the same library (A/B timing of kernel variants: tools/ab_lib.sh); never a fallback
LIB_PATH = os.environ.get("GPMI_LIB") or os.path.join(_HERE, "lib", "libgpmi.so")

KERNEL_SE = 0
KERNEL_RQ = 1
KERNEL_SUM = 2  # GPMI_KERNEL_SUM: a sum of stationary kernels declared by gpmi_set_sum
KERNEL_M32 = 3  # GPMI_KERNEL_M32 / _M52: Matern 3/2 and 5/2, theta laid out as for SE
KERNEL_M52 = 4
KERNEL_PER = 5  # GPMI_KERNEL_PER: periodic in the dimensions declared by gpmi_set_periodic, SE in the others
MAX_PERIODIC = 8  # GPMI_MAX_PERIODIC
PROF_KBUILD, PROF_SYRK, PROF_PANEL, PROF_SOLVE, PROF_SYRK_REST, PROF_TRSM, PROF_SYRK_SLICE, PROF_FLOW = 0, 1, 2, 3, 4, 5, 6, 7
PROF_COV = 8  # GPMI_PROF_COV: the kernels of gpmi_cov_columns without the copies
OPT_LOCKSTEP_ALWAYS, OPT_RESERVE_POINTS, OPT_NO_FLOW = 1, 2, 3
PREDICT_PANEL = 256  # GPMI_PREDICT_PANEL: query points per panel of gpmi_predict_batch
_TRACE_MS = float(os.environ["GPMI_TRACE_CALLS"]) if os.environ.get("GPMI_TRACE_CALLS") else None
ERR_INTERNAL = -5  # GPMI_ERR_INTERNAL
COV_CHUNK_ROWS = 2048  # GPMI_COV_CHUNK_ROWS: rows per chunk of gpmi_cov_columns
COV_MAX_COLUMNS = 512  # the most columns gpmi_cov_columns takes
PROF_DRAWS_SIGMA, PROF_DRAWS_FACTOR, PROF_DRAWS_NORMALS, PROF_DRAWS_PRODUCT = 9, 10, 11, 12  # GPMI_PROF_DRAWS_*
DRAWS_MAX_M = 16384  # GPMI_DRAWS_MAX_M: the most points gpmi_posterior_draws / gpmi_mvn_draws take
DRAWS_PANEL = 4096  # GPMI_DRAWS_PANEL: draws per panel of those two
PROF_SGP_BUILD, PROF_SGP_GRAM, PROF_SGP_FACTOR, PROF_SGP_GRAD = 13, 14, 15, 16  # GPMI_PROF_SGP_*
PROF_HESS_BUILD, PROF_HESS_GEMM, PROF_HESS_TRACE, PROF_HESS_CONTRACT = 13, 14, 15, 16  # GPMI_PROF_HESS_*: the same ids
SGP_MAX_M = 4096  # GPMI_SGP_MAX_M: the most inducing points a gpmi_sgp object takes
MT_MAX_T = 4096  # GPMI_MT_MAX_T: the most targets gpmi_mt_set_targets takes
GGP_LOGISTIC, GGP_POISSON, GGP_BINOMIAL = 0, 1, 2  # GPMI_GGP_*: the likelihoods of the gpmi_ggp_* entry points
PROF_GGP_TERMS, PROF_GGP_KV, PROF_GGP_BFORM, PROF_GGP_GRAD = 13, 14, 15, 16  # GPMI_PROF_GGP_*: the same ids


class GpmiUnavailable(RuntimeError):
    """libgpmi.so (the HIP extension) or an MI355X device is missing."""


class GpmiError(RuntimeError):
    """A gpmi_* call returned a non-zero status."""


_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int)
_vp = C.c_void_p
_i64 = C.c_int64

# name -> (restype, argtypes); mirrors include/gpmi.h one to one
SIGNATURES = {
    "gpmi_version": (C.c_int, []),
    "gpmi_device_count": (C.c_int, [_ip]),
    "gpmi_device_pci_bus_id": (C.c_int, [C.c_int, C.c_char_p, C.c_int]),
    "gpmi_create": (C.c_int, [C.c_int, C.POINTER(_vp)]),
    "gpmi_destroy": (C.c_int, [_vp]),
    "gpmi_last_error": (C.c_char_p, [_vp]),
    "gpmi_sync": (C.c_int, [_vp]),
    "gpmi_live_bytes": (C.c_int, [C.POINTER(_i64)]),
    "gpmi_set_data": (C.c_int, [_vp, _dp, _dp, _dp, _dp, _i64, _i64]),
    "gpmi_fit": (C.c_int, [_vp, C.c_int, _dp, C.c_int, C.c_double, _dp, _dp, _dp, _ip]),
    "gpmi_lml": (C.c_int, [_vp, C.c_int, _dp, C.c_int, C.c_double, _dp, _dp, _ip]),
    "gpmi_lml_batch": (C.c_int, [_vp, C.c_int, _i64, _dp, C.c_int, _dp, _dp, _dp, _dp, _ip]),
    "gpmi_lml_batch_submit": (C.c_int, [_vp, C.c_int, _i64, _dp, C.c_int, _dp, _dp, _dp, C.c_int]),
    "gpmi_lml_batch_wait": (C.c_int, [_vp, C.c_int, _dp, _ip]),
    "gpmi_set_streams": (C.c_int, [_vp, C.c_int]),
    "gpmi_set_option": (C.c_int, [_vp, C.c_int, C.c_int]),
    "gpmi_lml_grad": (C.c_int, [_vp, C.c_int, _dp, C.c_int, C.c_double, _dp, _dp, _dp, _dp, _dp, _ip]),
    "gpmi_lml_hessian": (C.c_int, [_vp, C.c_int, _dp, C.c_int, C.c_double, _dp, _dp, C.c_int, _dp, _dp, _dp, _ip]),
    "gpmi_lml_hessian_alpha": (C.c_int, [_vp, _dp]),
    "gpmi_flow_task_lists": (C.c_int, [C.c_int, C.c_int, C.c_int64, C.POINTER(C.c_int32), C.POINTER(C.c_int64)]),
    "gpmi_lml_grad_batch": (C.c_int, [_vp, C.c_int, C.c_int64, _dp, C.c_int, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _ip]),
    "gpmi_lml_grad_batch_noise": (C.c_int, [_vp, C.c_int, C.c_int64, _dp, C.c_int, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _ip]),
    "gpmi_predict": (C.c_int, [_vp, _dp, _i64, _dp, _dp]),
    "gpmi_predict_batch": (C.c_int, [_vp, C.c_int, _i64, _dp, C.c_int, _dp, _dp, _dp, _dp, _i64, _dp, _dp, _dp, _dp, _dp, _dp,
                                     _ip]),
    "gpmi_posterior": (C.c_int, [_vp, _dp, _i64, _dp, _dp]),
    "gpmi_spatial_derivatives": (C.c_int, [_vp, _dp, _i64, _dp, _dp]),
    "gpmi_gradient": (C.c_int, [_vp, _dp, _i64, _dp, _dp]),
    "gpmi_covariance": (C.c_int, [_vp, C.c_int, _dp, C.c_int, C.c_double, C.c_int, _dp]),
    "gpmi_cross_covariance": (C.c_int, [_vp, C.c_int, _dp, C.c_int, _dp, _i64, _dp]),
    "gpmi_get_K": (C.c_int, [_vp, _dp]),
    "gpmi_get_L": (C.c_int, [_vp, _dp]),
    "gpmi_loo_diag": (C.c_int, [_vp, _dp]),
    "gpmi_loo_terms": (C.c_int, [_vp, C.c_int, _dp, C.c_int, C.c_double, _dp, _dp, _dp, _ip]),
    "gpmi_loo_grad": (C.c_int, [_vp, C.c_int, _dp, C.c_int, C.c_double, _dp, _dp, _dp, _dp, _dp, _dp, _ip]),
    "gpmi_loo_grad_batch": (C.c_int, [_vp, C.c_int, C.c_int64, _dp, C.c_int, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _ip]),
    "gpmi_loo_grad_batch_noise": (C.c_int, [_vp, C.c_int, C.c_int64, _dp, C.c_int, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _ip]),
    "gpmi_fit_mix": (C.c_int, [_vp, C.c_int, _ip, _dp, _ip, _dp, C.c_double, _dp, _dp, _dp, _ip]),
    "gpmi_lml_mix": (C.c_int, [_vp, C.c_int, _ip, _dp, _ip, _dp, C.c_double, _dp, _dp, _ip]),
    "gpmi_lml_grad_mix": (C.c_int, [_vp, C.c_int, _ip, _dp, _ip, _dp, _dp, C.c_double, _dp, _dp, _dp, _dp, _dp, _ip]),
    "gpmi_lml_grad_batch_mix": (C.c_int, [_vp, C.c_int, _ip, _i64, _dp, _ip, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _ip]),
    "gpmi_loo_grad_batch_mix": (C.c_int, [_vp, C.c_int, _ip, _i64, _dp, _ip, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _ip]),
    "gpmi_loo_terms_mix": (C.c_int, [_vp, C.c_int, _ip, _dp, _ip, _dp, C.c_double, _dp, _dp, _dp, _ip]),
    "gpmi_predict_mix": (C.c_int, [_vp, _dp, _i64, _dp, _dp, _dp]),
    "gpmi_posterior_mix": (C.c_int, [_vp, _dp, _i64, _dp, _dp, _dp]),
    "gpmi_set_noise": (C.c_int, [_vp, _dp]),
    "gpmi_set_sum": (C.c_int, [_vp, C.c_int, _ip]),
    "gpmi_set_periodic": (C.c_int, [_vp, C.c_int, _ip]),
    "gpmi_lml_grad_qdiag": (C.c_int, [_vp, _dp]),
    "gpmi_linv_set": (C.c_int, [_vp, _dp, _i64, _dp, _dp]),
    "gpmi_linv_lml": (C.c_int, [_vp, C.c_int, _dp, C.c_int, C.c_double, _dp, _dp, _ip]),
    "gpmi_linv_lml_grad": (C.c_int, [_vp, C.c_int, _dp, C.c_int, C.c_double, _dp, _dp, _dp, _dp, _dp, _ip]),
    "gpmi_linv_posterior": (C.c_int, [_vp, C.c_int, _dp, C.c_int, C.c_double, _dp, _dp, _dp, _ip]),
    "gpmi_linv_lml_dense": (C.c_int, [_vp, _dp, _dp, _dp, _ip]),
    "gpmi_linv_lml_grad_dense": (C.c_int, [_vp, _dp, _dp, _dp, _dp, _dp, _ip]),
    "gpmi_linv_posterior_dense": (C.c_int, [_vp, _dp, _dp, _dp, _dp, _ip]),
    "gpmi_append_point": (C.c_int, [_vp, _dp, C.c_double, C.c_double, _dp, _dp, _dp, _ip]),
    "gpmi_capacity": (C.c_int, [_vp, C.POINTER(_i64)]),
    "gpmi_fit_dense": (C.c_int, [_vp, _dp, _dp, _dp, _dp, _ip]),
    "gpmi_lml_dense": (C.c_int, [_vp, _dp, _dp, _dp, _dp, _dp, _ip]),
    "gpmi_loo_dense": (C.c_int, [_vp, _dp, _dp, _dp, _dp, _dp, _dp, _ip]),
    "gpmi_predict_dense": (C.c_int, [_vp, _dp, _i64, _dp, _dp]),
    "gpmi_solve_rows": (C.c_int, [_vp, _dp, _i64, _dp, _dp]),
    "gpmi_solve_rows_kinv": (C.c_int, [_vp, _dp, _i64, _dp]),
    "gpmi_prepare_gradient": (C.c_int, [_vp, C.c_int]),
    "gpmi_comm_unique_id": (C.c_int, [C.c_char_p]),
    "gpmi_comm_init": (C.c_int, [_vp, C.c_int, C.c_int, C.c_char_p]),
    "gpmi_comm_allgather": (C.c_int, [_vp, _dp, _dp, _i64]),
    "gpmi_comm_broadcast": (C.c_int, [_vp, _dp, _i64, C.c_int]),
    "gpmi_comm_count": (C.c_int, [_vp, C.POINTER(C.c_int)]),
    "gpmi_comm_destroy": (C.c_int, [_vp]),
    "gpmi_kde_create": (C.c_int, [_vp, _i64, _dp, _i64, C.POINTER(_i64), C.POINTER(_i64), C.POINTER(_vp)]),
    "gpmi_kde_destroy": (C.c_int, [_vp]),
    "gpmi_kde_eval": (C.c_int, [_vp, _i64, _dp, C.POINTER(_i64), C.c_double, _dp, _dp]),
    "gpmi_kde_cv_logprob": (C.c_int, [_vp, _i64, _dp, C.c_int, _dp, C.c_double, _dp]),
    "gpmi_kde2d_create": (C.c_int, [_vp, _i64, _dp, _dp, C.POINTER(_vp)]),
    "gpmi_kde2d_destroy": (C.c_int, [_vp, _vp]),
    "gpmi_kde2d_eval": (C.c_int, [_vp, _vp, _i64, _dp, _dp, C.c_double, C.c_double, _dp]),
    "gpmi_kde2d_self": (C.c_int, [_vp, _vp, C.c_double, C.c_double, _dp, C.POINTER(_i64)]),
    "gpmi_kde2d_grid": (C.c_int, [_vp, _vp, _i64, _dp, _i64, _dp, C.c_double, C.c_double, _dp]),
    "gpmi_unimodal_create": (C.c_int, [_vp, _i64, _dp, C.POINTER(_vp)]),
    "gpmi_unimodal_destroy": (C.c_int, [_vp, _vp]),
    "gpmi_unimodal_logpdf_sums": (C.c_int, [_vp, _vp, _i64, C.c_int, _dp, _dp]),
    "gpmi_hdi_columns": (C.c_int, [_vp, _i64, _i64, _i64, _i64, _dp, C.c_int, C.POINTER(_i64), _i64, _dp,
                                   C.POINTER(C.c_int32)]),
    "gpmi_acf_columns": (C.c_int, [_vp, _i64, _i64, _i64, _i64, _dp, _i64, _dp, _dp, C.POINTER(_i64),
                                   C.POINTER(C.c_int32)]),
    "gpmi_cov_columns": (C.c_int, [_vp, _i64, _i64, _i64, _i64, _dp, _i64, _dp, _dp, C.POINTER(C.c_int32)]),
    "gpmi_acf_lag_blocks": (C.c_int, [_i64, _i64, C.POINTER(_i64), C.POINTER(_i64)]),
    "gpmi_posterior_draws": (C.c_int, [_vp, _dp, _i64, C.c_double, _i64, _dp, _i64, _i64, _dp, _dp, _dp, _ip]),
    "gpmi_mvn_draws": (C.c_int, [_vp, _i64, _dp, _dp, C.c_double, _i64, _dp, _i64, _i64, _dp, _dp, _ip]),
    "gpmi_draws_normals": (C.c_int, [_i64, _i64, _i64, _i64, _dp]),
    "gpmi_sgp_create": (C.c_int, [_vp, _i64, _i64, _dp, _i64, _dp, C.POINTER(_vp)]),
    "gpmi_sgp_destroy": (C.c_int, [_vp]),
    "gpmi_sgp_set_targets": (C.c_int, [_vp, _dp, _dp]),
    "gpmi_sgp_bound": (C.c_int, [_vp, C.c_int, _dp, C.c_int, C.c_double, C.c_double, _i64, _dp, _dp, _dp, _ip]),
    "gpmi_sgp_bound_zgrad": (C.c_int, [_vp, C.c_int, _dp, C.c_int, C.c_double, C.c_double, _i64, _dp, _dp, _dp, _dp, _ip]),
    "gpmi_sgp_set_inducing": (C.c_int, [_vp, _dp]),
    "gpmi_sgp_fit": (C.c_int, [_vp, C.c_int, _dp, C.c_int, C.c_double, C.c_double, _i64, _dp, _ip]),
    "gpmi_sgp_predict": (C.c_int, [_vp, _dp, _i64, _dp, _dp]),
    "gpmi_sgp_posterior": (C.c_int, [_vp, _dp, _i64, _dp, _dp]),
    "gpmi_sgp_posterior_draws": (C.c_int, [_vp, _dp, _i64, C.c_double, _i64, _dp, _i64, _i64, _dp, _dp, _dp, _ip]),
    "gpmi_sgp_spatial_derivatives": (C.c_int, [_vp, _dp, _i64, _dp, _dp]),
    "gpmi_sgp_schedule": (C.c_int, [_i64, _i64, _i64, C.POINTER(_i64)]),
    "gpmi_sgp_set_observations": (C.c_int, [_vp, _dp, _dp]),
    "gpmi_sgp_bound_batch": (C.c_int, [_vp, C.c_int, _i64, _dp, C.c_int, _dp, _dp, _dp, C.c_double, _i64, _i64, _dp, _dp, _dp, _dp,
                                       _ip]),
    "gpmi_sgp_batch_schedule": (C.c_int, [_i64, _i64, _i64, _i64, _i64, C.c_int, _i64, _i64, C.POINTER(_i64)]),
    "gpmi_select_schedule": (C.c_int, [_i64, C.POINTER(_i64)]),
    "gpmi_select_points": (C.c_int, [_vp, _i64, _i64, _dp, _dp, C.c_int, _dp, C.c_int, _i64, C.c_double, C.c_double,
                                     C.POINTER(_i64), _dp, _dp, C.POINTER(_i64)]),
    "gpmi_mt_set_targets": (C.c_int, [_vp, _dp, _i64]),
    "gpmi_mt_fit": (C.c_int, [_vp, C.c_int, _dp, C.c_int, C.c_double, _dp, _dp, _ip]),
    "gpmi_mt_lml": (C.c_int, [_vp, C.c_int, _dp, C.c_int, C.c_double, _dp, _dp, _ip]),
    "gpmi_mt_lml_grad": (C.c_int, [_vp, C.c_int, _dp, C.c_int, C.c_double, _dp, _dp, _ip]),
    "gpmi_mt_loo_terms": (C.c_int, [_vp, C.c_int, _dp, C.c_int, C.c_double, _dp, _dp, _ip]),
    "gpmi_mt_alpha": (C.c_int, [_vp, _dp]),
    "gpmi_mt_predict": (C.c_int, [_vp, _dp, _i64, _dp, _dp]),
    "gpmi_mt_loo": (C.c_int, [_vp, _dp, _dp]),
    "gpmi_ggp_set_observations": (C.c_int, [_vp, C.c_int, _dp, _dp, C.c_double]),
    "gpmi_ggp_fit": (C.c_int, [_vp, C.c_int, _dp, C.c_int, C.c_double, C.c_int, _dp, _ip, _ip]),
    "gpmi_ggp_logq": (C.c_int, [_vp, C.c_int, _dp, C.c_int, C.c_double, C.c_int, _dp, _ip, _ip]),
    "gpmi_ggp_logq_grad": (C.c_int, [_vp, C.c_int, _dp, C.c_int, C.c_double, C.c_int, _dp, _dp, _ip, _ip]),
    "gpmi_ggp_mode": (C.c_int, [_vp, _dp, _dp]),
    "gpmi_ggp_predict": (C.c_int, [_vp, _dp, _i64, _dp, _dp]),
    "gpmi_ggp_kv": (C.c_int, [_vp, C.c_int, _dp, C.c_int, _dp, C.c_int, _dp, C.c_int, C.POINTER(C.c_float)]),
    "gpmi_timer_start": (C.c_int, [_vp]),
    "gpmi_timer_stop": (C.c_int, [_vp, C.POINTER(C.c_float)]),
    "gpmi_profile_enable": (C.c_int, [_vp, C.c_int]),
    "gpmi_profile_read": (C.c_int, [_vp, C.c_int, C.POINTER(_i64), _dp, _dp, _dp]),
    "gpmi_profile_reset": (C.c_int, [_vp]),
    "gpmi_profile_clock": (C.c_int, [_vp, _dp]),
    "gpmi_dev_alloc": (C.c_int, [_vp, _i64, C.POINTER(_vp)]),
    "gpmi_dev_free": (C.c_int, [_vp, _vp]),
    "gpmi_dev_upload": (C.c_int, [_vp, _vp, _vp, _i64]),
    "gpmi_dev_download": (C.c_int, [_vp, _vp, _vp, _i64]),
    "gpmi_dev_potrf": (C.c_int, [_vp, _vp, _i64, _i64, _ip]),
    "gpmi_dev_gemm_nt": (C.c_int, [_vp, _vp, _i64, _vp, _i64, _vp, _i64, _i64, _i64, _i64, C.c_int]),
}

_lib = None


def load():
    """Load libgpmi.so and declare every prototype.  Raises GpmiUnavailable if it is not built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise GpmiUnavailable(
                f"{LIB_PATH} not found - build the HIP extension first "
                "(python -c 'import __graft_entry__ as g; g.build()' or make -C inference-tools_amd/csrc)"
            )
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)  # AttributeError here = header / library mismatch
            fn.restype = res
            fn.argtypes = args
        _lib = lib
        atexit.register(_close_all_handles)
    return _lib


def device_count() -> int:
    """Number of HIP devices visible to this process (0 without a GPU)."""
    cnt = C.c_int(0)
    load().gpmi_device_count(C.byref(cnt))
    return cnt.value


def device_identity(device: int) -> str:
    """Physical identity of visible device `device`: its PCI bus id, which - unlike the index - does not depend on the
    HIP_VISIBLE_DEVICES / ROCR_VISIBLE_DEVICES mask of the process ("" if the runtime cannot tell)."""
    buf = C.create_string_buffer(64)
    rc = load().gpmi_device_pci_bus_id(int(device), buf, 64)
    return buf.value.decode() if rc == 0 else ""


def default_device() -> int:
    """The device `Handle(None)` binds: GPMI_DEVICE, else LOCAL_RANK, else 0, modulo the number of visible devices."""
    device = int(os.environ.get("GPMI_DEVICE", os.environ.get("LOCAL_RANK", "0")))
    cnt = C.c_int(0)
    load().gpmi_device_count(C.byref(cnt))
    return device % cnt.value if cnt.value > 0 else device


def dptr(a):
    """double* view of a C-contiguous float64 array (None -> NULL)."""
    if a is None:
        return None
    assert a.dtype == np.float64 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(_dp)


def as_f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


_live_handles = weakref.WeakSet()


def _close_all_handles():
    """Destroy every live context while the HIP runtime is still up.  Registered with atexit after the library is
    loaded, so it runs BEFORE the runtime's own exit handlers: a context that is only collected during interpreter
    shutdown (e.g. one kept alive by the traceback of a failed test) would otherwise synchronise streams of a
    runtime that is already gone and hang the process."""
    for h in list(_live_handles):
        try:
            h.close()
        except Exception:
            pass


class Handle:
    """Owns one gpmi_ctx (one device, one set of streams / workspaces)."""

    def __init__(self, device=None):
        lib = load()
        if device is None:
            device = default_device()
        self.lib = lib
        self.device = device
        self.ctx = _vp()
        rc = lib.gpmi_create(device, C.byref(self.ctx))
        if rc != 0:
            msg = lib.gpmi_last_error(None).decode()
            raise GpmiUnavailable(f"gpmi_create(device={device}) failed with status {rc}: {msg}")
        _live_handles.add(self)

    # entry points that factorise a matrix from their own inputs: safe to repeat after a failed attempt
    _REPEATABLE = frozenset(("gpmi_fit", "gpmi_fit_mix", "gpmi_fit_dense", "gpmi_lml", "gpmi_lml_batch", "gpmi_lml_grad", "gpmi_lml_hessian",
                             "gpmi_lml_grad_batch", "gpmi_lml_mix", "gpmi_lml_grad_mix", "gpmi_lml_dense", "gpmi_loo_dense",
                             "gpmi_linv_lml", "gpmi_linv_lml_grad", "gpmi_linv_posterior", "gpmi_linv_lml_dense",
                             "gpmi_linv_lml_grad_dense", "gpmi_linv_posterior_dense", "gpmi_loo_terms", "gpmi_loo_grad",
                             "gpmi_loo_terms_mix", "gpmi_dev_potrf", "gpmi_loo_grad_batch", "gpmi_loo_grad_batch_noise", "gpmi_lml_grad_batch_noise",
                             "gpmi_lml_grad_batch_mix", "gpmi_loo_grad_batch_mix", "gpmi_predict_batch", "gpmi_posterior_draws",
                             "gpmi_mvn_draws", "gpmi_mt_fit", "gpmi_mt_lml", "gpmi_mt_lml_grad", "gpmi_mt_loo_terms",
                             "gpmi_ggp_fit", "gpmi_ggp_logq", "gpmi_ggp_logq_grad"))

    def call(self, name, *args):
        if _TRACE_MS is not None:  # GPMI_TRACE_CALLS=<ms>: report every entry-point call that takes longer (debugging aid)
            import time

            t0 = time.perf_counter()
            rc = getattr(self.lib, name)(self.ctx, *args)
            dt = (time.perf_counter() - t0) * 1e3
            if dt > _TRACE_MS:
                print(f"[gpmi trace] {name}: {dt:.2f} ms", file=sys.stderr, flush=True)
        else:
            rc = getattr(self.lib, name)(self.ctx, *args)
        if (rc == ERR_INTERNAL and name in self._REPEATABLE and not getattr(self, "_no_flow", False)
                and b"[flow-tail]" in self.lib.gpmi_last_error(self.ctx)):
            # a flag-ordered launch did not get its kernels side by side within its time limit (gpmi.h: GPMI_OPT_NO_FLOW):
            # once, with the stream-ordered schedule - the same factor, bit for bit, only slower.  (Only that time-out:
            # a triangular sweep that timed out is not cured by the option and must not cost the handle its fast path.)
            import warnings

            warnings.warn(f"{name}: {self.lib.gpmi_last_error(self.ctx).decode()} - repeating the call with the "
                          "stream-ordered schedule (GPMI_OPT_NO_FLOW) for the rest of this handle's life", RuntimeWarning)
            self._no_flow = True
            self.lib.gpmi_set_option(self.ctx, OPT_NO_FLOW, 1)
            rc = getattr(self.lib, name)(self.ctx, *args)
        if rc != 0:
            raise GpmiError(f"{name} failed with status {rc}: {self.lib.gpmi_last_error(self.ctx).decode()}")

    def close(self):
        if self.ctx:
            self.lib.gpmi_destroy(self.ctx)
            self.ctx = _vp()

    def __del__(self):
        if sys.is_finalizing():
            return  # the atexit hook has already closed what was alive; never touch the runtime from here
        try:
            self.close()
        except Exception:
            pass
