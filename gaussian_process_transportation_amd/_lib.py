"""ctypes binding of libgpt_hip.so (include/gpt_hip.h).  No CPU fallback: if the library or a
GPU is missing, every compute entry point raises."""
from __future__ import annotations

import ctypes as C
import importlib.util
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("GPT_HIP_LIB") or os.path.join(_HERE, "libgpt_hip.so")   # override: A/B of two builds

GPT_OK, GPT_E_HIP, GPT_E_NOT_PD, GPT_E_ARG, GPT_E_STATE = 0, -1, -2, -3, -4
GPT_F64, GPT_F32 = 0, 1
INV_CONVERGED, INV_MAX_PASSES, INV_SINGULAR, INV_STALLED = 0, 1, 2, 3      # GPT_INV_*: per-query status of inverse_map
INV_STATUS_NAMES = ("CONVERGED", "MAX_PASSES", "SINGULAR", "STALLED")
# outputs of gpt_transport_policy, in the order of its arguments
TRANSPORT_OUTPUTS = ("pos_rot", "pos_out", "var", "vel_out", "vel_var", "det_vel", "ori_out", "det_ori", "ori_gap",
                     "post_mean", "post_J", "post_Jvar", "post_J_ori")
# outputs of gpt_pullback_policy, in the order of its arguments (passes and status are int32, the rest float64)
PULLBACK_OUTPUTS = ("x", "vel", "f", "det", "residual", "passes", "status", "var_dyn", "map_var", "vel_var_map", "vel_var_dyn",
                    "post_z", "post_A", "post_Jvar")
# outputs of gpt_pullback_chain, in the order of its arguments (status, stage_status and stage_passes are int32, the rest float64);
# the stage_* arrays are stage-major: (K, M, ...)
CHAIN_OUTPUTS = ("x", "vel", "f", "status", "var_dyn", "vel_var_map", "vel_var_dyn", "stage_x", "stage_z", "stage_A", "stage_Jvar",
                 "stage_map_var", "stage_status", "stage_passes", "stage_residual", "stage_det")
CHAIN_INT_OUTPUTS = ("status", "stage_status", "stage_passes")
CHAIN_MAX = 4      # GPT_CHAIN_MAX: stages of one gpt_pullback_chain call
# outputs of gpt_rollout_policy, in the order of its arguments (steps_done and status are int32, the rest float64)
ROLLOUT_OUTPUTS = ("path", "vel", "x", "steps_done", "status")
ROLLOUT_INT_OUTPUTS = ("steps_done", "status")
# outputs of gpt_rollout_stabilised, in the order of its arguments
ROLLOUT_STAB_OUTPUTS = ("path", "vel", "x", "f", "var", "dvar", "steps_done", "status")
ROLLOUT_STAB_MAX_N = 1024   # training points of the dynamics of a stabilised or sampled rollout, at most (gpt_rollout_stab.h)
# outputs of gpt_rollout_sampled, in the order of its arguments
ROLLOUT_SAMPLED_OUTPUTS = ("path", "vel", "x", "f", "pvar", "cvar", "chol", "steps_done", "status")
ROLLOUT_SAMPLED_MAX_T = 256   # GPT_ROLLOUT_SAMPLED_MAX_T: steps of a sampled rollout, at most
ROLLOUT_DEGENERATE = 4        # GPT_ROLLOUT_DEGENERATE: status of a sampled path whose conditional variance fell to rounding level
ROLLOUT_SAMPLED_STATUS_NAMES = INV_STATUS_NAMES + ("DEGENERATE",)      # the status of a sampled path, by value
# outputs of gpt_rollout_pathwise, in the order of its arguments
ROLLOUT_PATHWISE_OUTPUTS = ("path", "vel", "x", "f", "steps_done", "status")
ROLLOUT_NO_FUNCTION = -1      # GPT_ROLLOUT_NO_FUNCTION: status of a path of rollout_pathwise_dev whose func entry names no function
PATHWISE_MAX_FREQ = 8192      # GPT_PATHWISE_MAX_FREQ: frequencies of the drawn functions of a pathwise rollout, at most
MAX_D = 15         # input dimensions the library accepts (gpt_common.h MAX_DIMS: D <= 3 tuned layout, 4 .. 8 rows of 8, 9 .. 15 rows of 16)
_NP_DTYPE = {GPT_F64: np.float64, GPT_F32: np.float32}

_dp = C.POINTER(C.c_double)
_vp = C.c_void_p
_i64 = C.c_int64
_ip = C.POINTER(C.c_int)


class ChainStage(C.Structure):
    """gpt_chain_stage: one transport of a gpt_pullback_chain call (the pointers: host or device memory, as the entry's)."""
    _fields_ = [("h", _vp), ("R", _vp), ("c_src", _vp), ("c_dst", _vp), ("R_jac", _vp), ("scale", C.c_double)]



# name -> (restype, argtypes); mirrors include/gpt_hip.h one to one
SIGNATURES = {
    "gpt_device_count": (C.c_int, []),
    "gpt_last_error": (C.c_char_p, []),
    "gpt_version": (C.c_char_p, []),
    "gpt_create": (C.c_int, [C.POINTER(_vp), C.c_int]),
    "gpt_destroy": (None, [_vp]),
    "gpt_set_stream": (C.c_int, [_vp, _vp]),
    "gpt_synchronize": (C.c_int, [_vp]),
    "gpt_set_dtype": (C.c_int, [_vp, C.c_int]),
    "gpt_set_matern_derivatives": (C.c_int, [_vp, C.c_int]),
    "gpt_fit": (C.c_int, [_vp, _dp, _dp, _i64, C.c_int, C.c_int, _dp, C.c_int, C.c_double, C.c_double, C.c_double]),
    "gpt_fit_kernel": (C.c_int, [_vp, _dp, _dp, _i64, C.c_int, C.c_int, _dp, C.c_int, C.c_double, C.c_double, C.c_double, C.c_int]),
    "gpt_fit_noise_matrix": (C.c_int, [_vp, _dp, _dp, _i64, C.c_int, C.c_int, _dp, C.c_int, C.c_double, _dp, C.c_double, C.c_int]),
    "gpt_fit_svgp": (C.c_int, [_vp, _dp, _dp, _dp, _i64, C.c_int, C.c_int, _dp, C.c_int, _dp, C.c_double, C.c_int]),
    "gpt_predict": (C.c_int, [_vp, _vp, _i64, _vp, _vp]),
    "gpt_derivative": (C.c_int, [_vp, _vp, _i64, _vp, _vp]),
    "gpt_dvariance": (C.c_int, [_vp, _vp, _i64, _vp]),
    "gpt_predict_all": (C.c_int, [_vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp]),
    "gpt_predict_all_dev": (C.c_int, [_vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp]),
    "gpt_inverse_map_dev": (C.c_int, [_vp, _vp, _vp, _i64, C.c_double, C.c_int, _vp, _vp, _vp, _vp, _vp]),
    "gpt_inverse_map": (C.c_int, [_vp, _dp, _dp, _i64, C.c_double, C.c_int, _dp, _dp, _dp, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "gpt_transport_policy_dev": (C.c_int, [_vp, _vp, _i64, _vp, _vp, _vp, C.c_double] + [_vp] * 16),
    "gpt_transport_policy": (C.c_int, [_vp, _dp, _i64, _dp, _dp, _dp, C.c_double] + [_dp] * 16),
    "gpt_pullback_policy_dev": (C.c_int, [_vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp, C.c_double, _vp, C.c_double, C.c_int, C.c_double]
                                + [_vp] * 14),
    "gpt_pullback_policy": (C.c_int, [_vp, _vp, _dp, _dp, _i64, _dp, _dp, _dp, C.c_double, _dp, C.c_double, C.c_int, C.c_double]
                            + [_dp] * 5 + [C.POINTER(C.c_int)] * 2 + [_dp] * 7),
    "gpt_pullback_chain_dev": (C.c_int, [C.POINTER(ChainStage), C.c_int, _vp, _vp, _vp, _i64, C.c_double, C.c_int, C.c_double] + [_vp] * 16),
    "gpt_pullback_chain": (C.c_int, [C.POINTER(ChainStage), C.c_int, _vp, _dp, _dp, _i64, C.c_double, C.c_int, C.c_double]
                           + [_dp] * 3 + [_ip] + [_dp] * 8 + [_ip] * 2 + [_dp] * 2),
    "gpt_rollout_policy_dev": (C.c_int, [C.POINTER(ChainStage), C.c_int, _vp, _vp, _vp, _i64, _i64, C.c_double, C.c_double, C.c_int] + [_vp] * 5),
    "gpt_rollout_policy": (C.c_int, [C.POINTER(ChainStage), C.c_int, _vp, _dp, _dp, _i64, _i64, C.c_double, C.c_double, C.c_int]
                           + [_dp] * 3 + [_ip] * 2),
    "gpt_rollout_stabilised_dev": (C.c_int, [C.POINTER(ChainStage), C.c_int, _vp, _vp, _vp, _i64, _i64, C.c_double, C.c_double, C.c_int,
                                              C.c_double, C.c_double] + [_vp] * 8),
    "gpt_rollout_stabilised": (C.c_int, [C.POINTER(ChainStage), C.c_int, _vp, _dp, _dp, _i64, _i64, C.c_double, C.c_double, C.c_int,
                                          C.c_double, C.c_double] + [_dp] * 6 + [_ip] * 2),
    "gpt_rollout_sampled_dev": (C.c_int, [C.POINTER(ChainStage), C.c_int, _vp, _vp, _vp, _vp, _i64, _i64, C.c_double, C.c_double, C.c_int,
                                           C.c_double] + [_vp] * 9),
    "gpt_rollout_sampled": (C.c_int, [C.POINTER(ChainStage), C.c_int, _vp, _dp, _dp, _dp, _i64, _i64, C.c_double, C.c_double, C.c_int,
                                       C.c_double] + [_dp] * 7 + [_ip] * 2),
    "gpt_rollout_pathwise_dev": (C.c_int, [C.POINTER(ChainStage), C.c_int, _vp, _vp, _vp, _vp, _i64, _i64, C.c_double, C.c_double, C.c_int,
                                            _i64, _vp, _i64, _vp, _vp] + [_vp] * 6),
    "gpt_rollout_pathwise": (C.c_int, [C.POINTER(ChainStage), C.c_int, _vp, _dp, _dp, _ip, _i64, _i64, C.c_double, C.c_double, C.c_int,
                                        _i64, _dp, _i64, _dp, _dp] + [_dp] * 4 + [_ip] * 2),
    "gpt_predict_cov": (C.c_int, [_vp, _dp, _i64, _dp, _dp]),
    "gpt_export": (C.c_int, [_vp, _dp, _dp]),
    "gpt_export_inverse_factor": (C.c_int, [_vp, _dp]),
    "gpt_apply_inverse": (C.c_int, [_vp, _dp, _i64, _dp]),
    "gpt_lml": (C.c_int, [_vp, _dp]),
    "gpt_lml_gradient": (C.c_int, [_vp, _dp, _dp]),
    "gpt_lml_objective": (C.c_int, [_vp, _dp, _dp, _i64, C.c_int, C.c_int, _dp, C.c_int, C.c_double, C.c_double, C.c_double, C.c_int,
                                    _dp, _dp]),
    "gpt_factor_blob": (C.c_int, [_vp, C.POINTER(_vp), C.POINTER(C.c_size_t)]),
    "gpt_factor_alloc": (C.c_int, [_vp, _i64, C.c_int, C.c_int, C.POINTER(_vp), C.POINTER(C.c_size_t)]),
    "gpt_factor_alloc_model": (C.c_int, [_vp, _i64, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(_vp), C.POINTER(C.c_size_t)]),
    "gpt_factor_commit": (C.c_int, [_vp]),
    "gpt_factor_copy": (C.c_int, [_vp, _vp]),
    "gpt_model_info": (C.c_int, [_vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "gpt_debug_var_plan": (C.c_int, [_i64, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(_i64), C.POINTER(C.c_int),
                                     C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "gpt_debug_fit_plan": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(_i64), C.POINTER(_i64)]),
    "gpt_debug_dgemm": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, _dp, _i64, _dp, _i64, _dp, _i64,
                                  C.c_int, C.POINTER(C.c_int)]),
    "gpt_debug_set_inverse_factor": (C.c_int, [_vp, _dp, _i64]),
    "gpt_debug_set_task_inverse_factor": (C.c_int, [_vp, C.c_int, _dp, _i64]),
    "gpt_info": (C.c_int, [_vp, C.POINTER(_i64), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(_i64)]),
    "gpt_fit_timings": (C.c_int, [_vp, _dp, C.c_int]),
    "gpt_set_profiling": (C.c_int, [_vp, C.c_int]),
    "gpt_reserve": (C.c_int, [_vp, C.c_int64, C.c_int]),
    "gpt_predict_timings": (C.c_int, [_vp, _dp]),
    "gpt_debug_var_path": (C.c_int, [_vp]),
    "gpt_svgp_train": (C.c_int, [C.c_int, _dp, _dp, _i64, C.c_int, C.c_int, C.c_int, _dp, _dp, _dp, _dp, _dp, _dp,
                                 C.POINTER(_i64), _i64, C.POINTER(_i64), _i64, C.c_double, _dp]),
    "gpt_svgp_elbo_grad": (C.c_int, [C.c_int, _dp, _dp, _i64, _i64, C.c_int, C.c_int, C.c_int, _dp, _dp, _dp, _dp, _dp, _dp,
                                     _dp, _dp, _dp, _dp, _dp, _dp, _dp]),
    "gpt_svgp_surface_train": (C.c_int, [C.c_int, _dp, _dp, _i64, C.c_int, C.c_int, C.c_int, _dp, _dp, _dp, _dp, _dp, _dp,
                                         C.POINTER(_i64), _i64, C.POINTER(_i64), _i64, C.c_double, _dp]),
    "gpt_svgp_surface_elbo_grad": (C.c_int, [C.c_int, _dp, _dp, _i64, _i64, C.c_int, C.c_int, C.c_int, _dp, _dp, _dp, _dp, _dp,
                                             _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp]),
    "gpt_svgp_surface_predict": (C.c_int, [C.c_int, _dp, _dp, _dp, _dp, _dp, C.c_int, C.c_int, C.c_int, _dp, _i64, _dp, _dp, _dp]),
    "gpt_select_greedy": (C.c_int, [C.c_int, _dp, _i64, C.c_int, _dp, C.c_double, C.c_double, C.c_double, C.c_int, C.POINTER(_i64),
                                    C.c_int, C.c_int, C.POINTER(_i64), _dp, _dp]),
    "gpt_batch_lml_objective": (C.c_int, [C.c_int, _dp, _dp, C.POINTER(_i64), _i64, C.c_int, C.c_int, _dp, C.c_int, _dp, _dp, C.c_double,
                                          C.c_int, _dp, _dp, C.POINTER(C.c_int)]),
    "gpt_batch_fit": (C.c_int, [C.c_int, _dp, _dp, C.POINTER(_i64), _i64, C.c_int, C.c_int, _dp, C.c_int, _dp, _dp, C.c_double, C.c_int,
                                _dp, _dp, _dp, C.POINTER(C.c_int)]),
    "gpt_batch_predict": (C.c_int, [C.c_int, _dp, _dp, C.POINTER(_i64), _i64, C.c_int, C.c_int, _dp, C.c_int, _dp, _dp, C.c_double,
                                    C.c_int, _dp, C.POINTER(_i64), _dp, _dp, _dp, _dp, _dp, C.POINTER(C.c_int)]),
    "gpt_batch_optimize": (C.c_int, [C.c_int, _dp, _dp, C.POINTER(_i64), _i64, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), _dp, _i64,
                                     _dp, C.c_double, C.c_int, C.c_double, C.c_double, C.c_int, C.c_int, C.c_int, _dp, _dp,
                                     C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "gpt_batch_optimize_bounded": (C.c_int, [C.c_int, _dp, _dp, C.POINTER(_i64), _i64, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), _dp,
                                             _i64, _dp, C.c_double, C.c_int, C.c_double, C.c_double, C.c_int, C.c_int, C.c_int, _dp, _dp,
                                             C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "gpt_batch_fold_scan": (C.c_int, [C.c_int, _dp, _dp, C.POINTER(_i64), _i64, C.c_int, _dp, C.c_int, _dp, _dp, C.c_double, C.c_int, _dp,
                                      C.POINTER(_i64), _i64, C.c_int, _dp, C.POINTER(_i64), C.POINTER(_i64), _dp, _dp, _dp, _dp, _dp,
                                      C.POINTER(C.c_int), C.POINTER(C.c_int)]),
}

_lib = None


class GptError(RuntimeError):
    pass


def _preload_hip_runtime():
    """PyTorch-ROCm wheels bundle their own libamdhip64.so with the same SONAME as /opt/rocm's.  The
    first copy loaded serves the whole process, and torch cannot initialise on a foreign copy
    ("No HIP GPUs are available").  When torch is installed but not yet imported, load ITS runtime
    first so that libgpt_hip.so and a later `import torch` share one HIP runtime in either order."""
    if "torch" in sys.modules:
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.submodule_search_locations:
        return
    cand = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
    if os.path.exists(cand):
        try:
            C.CDLL(cand, mode=C.RTLD_GLOBAL)
        except OSError:
            pass


def load():
    """Load libgpt_hip.so (built by `__graft_entry__.build()` / csrc/Makefile).  Fails loudly."""
    global _lib
    if _lib is not None:
        return _lib
    _preload_hip_runtime()
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build the HIP extension first (python -c 'import __graft_entry__ as g; g.build()' "
            "or make -C gaussian_process_transportation_amd/csrc).  There is no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError if the ABI drifted
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def last_error() -> str:
    return load().gpt_last_error().decode("utf-8", "replace")


def check(rc: int, what: str = ""):
    if rc == GPT_OK:
        return
    msg = last_error()
    if rc == GPT_E_NOT_PD:
        raise np.linalg.LinAlgError(msg)          # what sklearn raises (_gpr.py:348-358)
    if rc == GPT_E_ARG:
        raise ValueError(msg)
    raise GptError(f"{what or 'libgpt_hip'} failed ({rc}): {msg}")


def require_gpu() -> int:
    n = load().gpt_device_count()
    if n < 1:
        raise GptError("no HIP device visible: this package only runs on an MI355X (gfx950); there is no CPU path")
    return n


def as_f64(a, ndim=None, what="Input", dtype=np.float64) -> np.ndarray:
    """C-contiguous array of `dtype`, finite.  scikit-learn's check_array refuses NaN / infinity in fit and predict
    inputs with a ValueError (sklearn/utils/validation.py, reached from _gpr.py:262 and :415); the kernels would
    otherwise turn a NaN query into a prior-looking prediction (the table exp clamps its argument).  The
    device-pointer API (`predict_all_dev`) leaves this check to the caller."""
    a = np.ascontiguousarray(a, dtype=dtype)
    if ndim is not None and a.ndim != ndim:
        raise ValueError(f"expected a {ndim}-D array, got shape {a.shape}")
    if not np.isfinite(a).all():
        raise ValueError(f"{what} contains NaN or infinity.")
    return a


def dptr(a):
    return None if a is None else a.ctypes.data_as(_dp)


def vptr(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def debug_var_plan(n_columns, n_iblocks, n_tasks, n_workgroups, order=-1):
    """The work decomposition of the variance kernel (csrc/gpt_plan.h) as numpy arrays; host code, no GPU."""
    lib = load()
    counts = (_i64 * 12)()
    ip = C.POINTER(C.c_int)
    check(lib.gpt_debug_var_plan(n_columns, n_iblocks, n_tasks, n_workgroups, order, counts, None, None, None, None))
    item_begin = np.zeros(n_workgroups + 1, dtype=np.int32)
    items = np.zeros((max(counts[0], 1), 8), dtype=np.int32)
    fin = np.zeros((max(counts[6], 1), 2), dtype=np.int32)
    splits = np.zeros((max(counts[1], 1), 3), dtype=np.int32)
    check(lib.gpt_debug_var_plan(n_columns, n_iblocks, n_tasks, n_workgroups, order, counts, item_begin.ctypes.data_as(ip),
                                 items.ctypes.data_as(ip), fin.ctypes.data_as(ip), splits.ctypes.data_as(ip)))
    return {"n_items": counts[0], "n_splits": counts[1], "n_slots": counts[2], "n_vslots": counts[3], "ncb": counts[4],
            "nfull": counts[5], "order": counts[7], "cohorts": bool(counts[8]), "cohort_s": counts[9], "cohort_f": counts[10], "cut_diag": bool(counts[11]),
            "item_begin": item_begin, "items": items[:counts[0]],
            "fin": fin[:counts[6]], "splits": splits[:counts[1]]}


FIT_OP_KINDS = ("POTRF", "FINISH", "TRINV", "UPDATE", "TRSM", "COPY_L21", "T", "WFIN", "FACTORED")
FIT_OP_FIELDS = ("kind", "stream", "off", "n1", "n2", "k0", "kw", "row_end", "grp", "r0", "r0_size", "r1", "r1_size", "wait0", "wait1",
                 "wait2", "record")


def debug_fit_plan(n_padded, form=-1, panel=-1, streams=-1):
    """The plan of the factor + inverse (csrc/gpt_fit_plan.h) for a padded size; host code, no GPU.
    ops: one row per operation, columns FIT_OP_FIELDS (regions in doubles inside the arena; events by id, -1 = none)."""
    lib = load()
    counts = (_i64 * 6)()
    check(lib.gpt_debug_fit_plan(n_padded, form, panel, streams, counts, None))
    ops = np.zeros((max(counts[0], 1), 18), dtype=np.int64)
    check(lib.gpt_debug_fit_plan(n_padded, form, panel, streams, counts, ops.ctypes.data_as(C.POINTER(_i64))))
    return {"arena": counts[1], "form": counts[2], "n_events": counts[3], "allocated": counts[4], "side_eighths": counts[5],
            "ops": ops[:counts[0], :17]}


def debug_dgemm(A, B, out, M, N, K, alpha=1.0, at=False, bt=False, lower_only=False, device=0):
    """One call of the library's fp64 GEMM (gpt_debug_dgemm; tests only): out[:M, :N] = alpha op(A) op(B) in place, where A,
    B and out are C-contiguous float64 2-D arrays whose row length is the leading dimension (the operands sit in their
    first rows and columns: A (M, K), or (K, M) with at; B (K, N), or (N, K) with bt).  Returns the tile edge the launcher
    chose (32, 64 or 128)."""
    rows = {"A": K if at else M, "B": N if bt else K, "out": M}
    for name, a in (("A", A), ("B", B), ("out", out)):
        if not (isinstance(a, np.ndarray) and a.dtype == np.float64 and a.ndim == 2 and a.flags.c_contiguous):
            raise ValueError(f"debug_dgemm: {name} must be a C-contiguous float64 2-D array")
        if a.shape[0] < rows[name]:
            raise ValueError(f"debug_dgemm: {name} has {a.shape[0]} rows, the product uses {rows[name]}")
    if not out.flags.writeable:
        raise ValueError("debug_dgemm: out is read-only")
    edge = C.c_int(0)
    check(load().gpt_debug_dgemm(device, int(at), int(bt), M, N, K, float(alpha), dptr(A), A.shape[1], dptr(B), B.shape[1], dptr(out),
                                 out.shape[1], int(lower_only), C.byref(edge)), "gpt_debug_dgemm")
    return edge.value


SVGP_PARAMS = ("Z", "m", "C", "raw_ls", "raw_os", "raw_noise")
SURFACE_MAX_INDUCING = 4096     # gpt_svgp_surface_* limits (include/gpt_hip.h)
SURFACE_MAX_TASKS = 32
SURFACE_MAX_BATCH = 1024
# entry-point prefix -> (name in messages, a length-scale vector per task, limits (inducing points, tasks, rows per batch))
_SVGP_MODELS = {"gpt_svgp": ("SVGP", False, (1024, 32, 1024)),
                "gpt_svgp_surface": ("surface SVGP", True, (SURFACE_MAX_INDUCING, SURFACE_MAX_TASKS, SURFACE_MAX_BATCH))}


def _svgp_params(params, D, T, who, per_task_ls, limits):
    """Validated C-contiguous float64 copies of the SVGP training parameters (gpt_svgp_train; per_task_ls: raw_ls (T,D)), within `limits`."""
    p = {k: np.ascontiguousarray(params[k], dtype=np.float64).copy() for k in SVGP_PARAMS}
    Zn = p["Z"].shape[0] if p["Z"].ndim == 2 else -1
    shapes = {"Z": (Zn, D), "m": (T, Zn), "C": (T, Zn, Zn), "raw_ls": (T, D) if per_task_ls else (D,), "raw_os": (T,),
              "raw_noise": (T + 1,)}
    for k, shp in shapes.items():
        if p[k].shape != shp:
            raise ValueError(f"{who} parameter {k} has shape {p[k].shape}, expected {shp}")
    for what, n, most in (("inducing points", Zn, limits[0]), ("T (tasks)", T, limits[1]), ("D", D, MAX_D)):
        if not 1 <= n <= most:
            raise ValueError(f"{who}: {what} must be 1 .. {most}, got {n}")
    return p, Zn


def svgp_train(X, Y, params, idx, batch_begin, lr=0.01, device=0, model="gpt_svgp"):
    """Adam on the SVGP's negative ELBO over the schedule (gpt_svgp_train).  `params` (dict of SVGP_PARAMS) is updated in
    place; returns the per-step loss (n_steps,).  Every refusal that needs no device comes before the library is loaded."""
    who, per_task_ls, limits = _SVGP_MODELS[model]
    X = as_f64(X, 2, "X")
    Y = as_f64(Y, 2, "y")
    (N, D), T = X.shape, Y.shape[1]
    if Y.shape[0] != N:
        raise ValueError("X and Y have different numbers of rows")
    p, Zn = _svgp_params(params, D, T, who, per_task_ls, limits)
    idx = np.ascontiguousarray(idx, dtype=np.int64)
    bb = np.ascontiguousarray(batch_begin, dtype=np.int64)
    n_steps = max(bb.size - 1, 0)
    if n_steps < 1:
        raise ValueError(f"{who}: empty schedule (no optimiser step)")
    sizes = np.diff(bb)
    if sizes.min() < 1 or sizes.max() > limits[2]:
        raise ValueError(f"{who}: every batch must have 1 .. {limits[2]} rows")
    if bb[0] < 0 or bb[-1] > idx.size or idx[bb[0]:bb[-1]].min() < 0 or idx[bb[0]:bb[-1]].max() >= N:
        raise ValueError(f"{who}: schedule indices must lie in [0, N)")
    lib = load()
    require_gpu()
    trace = np.zeros(n_steps)
    ip = C.POINTER(_i64)
    check(getattr(lib, model + "_train")(int(device), dptr(X), dptr(Y), N, D, T, Zn, *(dptr(p[k]) for k in SVGP_PARAMS),
                                         idx.ctypes.data_as(ip), idx.size, bb.ctypes.data_as(ip), n_steps, float(lr), dptr(trace)),
          model + "_train")
    for k in SVGP_PARAMS:
        params[k] = p[k]
    return trace


def svgp_elbo_grad(Xb, Yb, params, num_data, device=0, model="gpt_svgp"):
    """(loss, {name: gradient}) of one minibatch (gpt_svgp_elbo_grad)."""
    who, per_task_ls, limits = _SVGP_MODELS[model]
    Xb = as_f64(Xb, 2, "X")
    Yb = as_f64(Yb, 2, "y")
    (b, D), T = Xb.shape, Yb.shape[1]
    if Yb.shape[0] != b:
        raise ValueError("X and Y have different numbers of rows")
    if not 1 <= b <= limits[2]:
        raise ValueError(f"{who}: batch size must be 1 .. {limits[2]}, got {b}")
    p, Zn = _svgp_params(params, D, T, who, per_task_ls, limits)
    lib = load()
    require_gpu()
    g = {k: np.zeros_like(p[k]) for k in SVGP_PARAMS}
    loss = C.c_double()
    check(getattr(lib, model + "_elbo_grad")(int(device), dptr(Xb), dptr(Yb), b, int(num_data), D, T, Zn, *(dptr(p[k]) for k in SVGP_PARAMS),
                                             C.byref(loss), *(dptr(g[k]) for k in SVGP_PARAMS)), model + "_elbo_grad")
    return loss.value, g


def svgp_surface_train(X, Y, params, idx, batch_begin, lr=0.01, device=0):
    """Adam on the surface SVGP's negative ELBO over the schedule (gpt_svgp_surface_train).  `params` (dict of SVGP_PARAMS,
    raw_ls (T,D)) is updated in place; returns the per-step loss (n_steps,)."""
    return svgp_train(X, Y, params, idx, batch_begin, lr, device, model="gpt_svgp_surface")


def svgp_surface_elbo_grad(Xb, Yb, params, num_data, device=0):
    """(loss, {name: gradient}) of one minibatch of the surface SVGP (gpt_svgp_surface_elbo_grad)."""
    return svgp_elbo_grad(Xb, Yb, params, num_data, device, model="gpt_svgp_surface")


def svgp_surface_predict(params, Xq, var=False, J=False, device=0):
    """(mean (M,T), var (M,T) or None, J (M,T,D) or None) of the surface SVGP's variational predictive
    (gpt_svgp_surface_predict).  `params` needs Z, m, C, raw_ls, raw_os."""
    Z = as_f64(params["Z"], 2, "Z")
    Xq = as_f64(Xq, 2, "x")
    Zn, D = Z.shape
    T = np.asarray(params["m"]).shape[0]
    if Xq.shape[1] != D:
        raise ValueError(f"queries have {Xq.shape[1]} columns, the model {D}")
    p, _ = _svgp_params(dict(params, raw_noise=np.zeros(T + 1)), D, T, *_SVGP_MODELS["gpt_svgp_surface"])
    M = Xq.shape[0]
    if M < 1:
        raise ValueError("no query points")
    lib = load()
    require_gpu()
    mean = np.zeros((M, T))
    v = np.zeros((M, T)) if var else None
    j = np.zeros((M, T, D)) if J else None
    check(lib.gpt_svgp_surface_predict(int(device), dptr(p["Z"]), dptr(p["m"]), dptr(p["C"]), dptr(p["raw_ls"]), dptr(p["raw_os"]),
                                       Zn, D, T, dptr(Xq), M, dptr(mean), dptr(v) if var else None, dptr(j) if J else None),
          "gpt_svgp_surface_predict")
    return mean, v, j


def select_greedy(X, length_scale, constant_value, noise_level, alpha, n_total, initial=(), kernel_type=0, device=0,
                  residual=True):
    """Greedy maximum-variance selection of n_total pool points (gpt_select_greedy): the `initial` indices first, in their
    order, then the point of largest posterior variance each time (ties: lowest index).  Returns (selected (n_total,) int64,
    selection_variance (n_total - len(initial),), residual_variance (N,) or None)."""
    X = np.ascontiguousarray(X, dtype=np.float64)
    if X.ndim != 2:
        raise ValueError(f"expected a 2-D array, got shape {X.shape}")
    N, D = X.shape
    if not 1 <= D <= MAX_D:
        raise ValueError(f"the pool has {D} features: this GPU path supports input dimension D = 1 .. {MAX_D} only")
    ls = as_f64(np.atleast_1d(length_scale), 1, "length_scale")
    if ls.size == 1:
        ls = np.full(D, ls[0])
    if ls.size != D:
        raise ValueError(f"length_scale has {ls.size} entries, the pool {D} features")
    initial = np.ascontiguousarray(initial, dtype=np.int64).reshape(-1)
    n_total = int(n_total)
    if n_total > N:
        raise ValueError(f"cannot select {n_total} points from a pool of {N}")
    if n_total < 1 or initial.size > n_total:
        raise ValueError("need len(initial) <= n_total and n_total >= 1")
    lib = load()             # the entry point scans the pool for NaN / infinity itself (ValueError)
    require_gpu()
    selected = np.zeros(n_total, dtype=np.int64)
    selvar = np.zeros(max(n_total - initial.size, 1))
    resid = np.zeros(N) if residual else None
    ip = C.POINTER(_i64)
    check(lib.gpt_select_greedy(int(device), dptr(X), N, D, dptr(ls), float(constant_value), float(noise_level), float(alpha),
                                int(kernel_type), initial.ctypes.data_as(ip) if initial.size else None, initial.size, n_total,
                                selected.ctypes.data_as(ip), dptr(selvar), dptr(resid)), "gpt_select_greedy")
    return selected, selvar[:n_total - initial.size], resid


BATCH_MAX_N = 128          # gpt_batch_* limits (include/gpt_hip.h)
BATCH_MAX_O = 16
BATCH_MAX_B = 1 << 20


def batch_pack(Xs, Ys, who="batch"):
    """The ragged layout of the gpt_batch_* entry points from sequences of (n_b, D) / (n_b, O) arrays: (X (sum n, D),
    Y (sum n, O), n_begin (B + 1) int64).  Every refusal that needs no device is made here, before the library is loaded."""
    Xs = [as_f64(x, 2, "X") for x in Xs]
    Ys = [as_f64(y, 2, "y") for y in Ys]
    B = len(Xs)
    if len(Ys) != B:
        raise ValueError(f"{who}: {B} inputs but {len(Ys)} targets")
    if not 1 <= B <= BATCH_MAX_B:
        raise ValueError(f"{who}: a batch holds 1 .. 2^20 models, got {B}")
    D, O = Xs[0].shape[1], Ys[0].shape[1]
    for b, (x, y) in enumerate(zip(Xs, Ys)):
        if x.shape[1] != D or y.shape[1] != O:
            raise ValueError(f"{who}: every model of a batch must share D and O; model {b} has D = {x.shape[1]}, O = {y.shape[1]}, "
                             f"model 0 has D = {D}, O = {O}")
        if y.shape[0] != x.shape[0]:
            raise ValueError(f"{who}: model {b}: X and Y have different numbers of rows")
        if not 1 <= x.shape[0] <= BATCH_MAX_N:
            raise ValueError(f"{who}: model {b} has {x.shape[0]} rows; a batch member holds 1 .. {BATCH_MAX_N} points "
                             "(larger models: GaussianProcess)")
    if not 1 <= D <= MAX_D:
        raise ValueError(f"{who}: X has {D} features: this GPU path supports input dimension D = 1 .. {MAX_D} only")
    if not 1 <= O <= BATCH_MAX_O:
        raise ValueError(f"{who}: y has {O} outputs: a batch supports O = 1 .. {BATCH_MAX_O}")
    n_begin = np.zeros(B + 1, dtype=np.int64)
    np.cumsum([x.shape[0] for x in Xs], out=n_begin[1:])
    return np.concatenate(Xs), np.concatenate(Ys), n_begin


def _batch_hyper(B, D, length_scale, constant_value, noise_level, who):
    ls = as_f64(length_scale, None, "length_scale")
    if ls.ndim == 1:
        ls = ls[:, None]
    if ls.ndim != 2 or ls.shape[0] != B or ls.shape[1] not in (1, D):
        raise ValueError(f"{who}: length_scale must be (B, 1) or (B, D), got {ls.shape}")
    c = as_f64(constant_value, 1, "constant_value")
    noise = as_f64(noise_level, 1, "noise_level")
    if c.shape != (B,) or noise.shape != (B,):
        raise ValueError(f"{who}: constant_value and noise_level must have one entry per model")
    return np.ascontiguousarray(ls), c, noise


def _split(a, begin):
    return [a[begin[b]:begin[b + 1]] for b in range(len(begin) - 1)]


def batch_lml_objective_packed(X, Y, n_begin, length_scale, constant_value, noise_level, alpha, kernel_type=0, device=0):
    """gpt_batch_lml_objective on arrays already in the ragged layout (batch_pack): (lml (B,), grad (B, 2 + n_ls), status (B,)).
    A model whose status is GPT_E_NOT_PD has NaN in its lml and gradient."""
    B, D = n_begin.size - 1, X.shape[1]
    ls, c, noise = _batch_hyper(B, D, length_scale, constant_value, noise_level, "batch_lml_objective")
    lib = load()
    require_gpu()
    lml = np.full(B, np.nan)
    grad = np.full((B, 2 + ls.shape[1]), np.nan)
    status = np.zeros(B, dtype=np.int32)
    check(lib.gpt_batch_lml_objective(int(device), dptr(X), dptr(Y), n_begin.ctypes.data_as(C.POINTER(_i64)), B, D, Y.shape[1], dptr(ls),
                                      ls.shape[1], dptr(c), dptr(noise), float(alpha), int(kernel_type), dptr(lml), dptr(grad),
                                      status.ctypes.data_as(C.POINTER(C.c_int))), "gpt_batch_lml_objective")
    return lml, grad, status


GPT_OPT_PGTOL, GPT_OPT_FTOL, GPT_OPT_MAX_ITER, GPT_OPT_MAX_EVALS, GPT_OPT_LINESEARCH, GPT_OPT_NOT_PD_START = range(6)   # gpt_hip.h
BATCH_MAX_R = 1 << 20


def batch_opt_evals_per_launch():
    """Objective evaluations a run may spend in one launch of the device search (GPT_BATCH_OPT_EVALS_PER_LAUNCH, default 64):
    it bounds how long one launch can last."""
    return int(os.environ.get("GPT_BATCH_OPT_EVALS_PER_LAUNCH", "64"))


def batch_optimize_packed(X, Y, n_begin, n_ls, run_model, theta0, bounds, alpha, kernel_type=0, device=0, pgtol=1e-5, ftol=2.22e-9,
                          max_iter=15000, max_evals=15000, evals_per_launch=None):
    """gpt_batch_optimize on arrays in the ragged layout (batch_pack): R runs, run r minimising -LML of model run_model[r]
    from theta0[r] (R, 2 + n_ls) = log [c, l.., noise] inside bounds (2 + n_ls, 2) (log space; lo == hi: fixed).  The defaults
    are what sklearn passes to scipy's L-BFGS-B.  Returns (theta (R, 2 + n_ls), lml (R,), iterations (R,), evaluations (R,),
    status (R,) GPT_OPT_*, launches)."""
    who = "batch_optimize"
    B, D = n_begin.size - 1, X.shape[1]
    P = 2 + int(n_ls)
    run_model = np.ascontiguousarray(run_model, dtype=np.int32)
    theta0 = as_f64(theta0, 2, "theta0")
    bounds = as_f64(bounds, 2, "bounds")
    R = run_model.size
    if not 1 <= R <= BATCH_MAX_R:
        raise ValueError(f"{who}: a call holds 1 .. 2^20 runs, got {R}")
    if theta0.shape != (R, P) or bounds.shape != (P, 2):
        raise ValueError(f"{who}: theta0 must be (R, 2 + n_ls) = ({R}, {P}) and bounds (2 + n_ls, 2), got {theta0.shape} and {bounds.shape}")
    if evals_per_launch is None:
        evals_per_launch = batch_opt_evals_per_launch()
    lib = load()
    require_gpu()
    theta = np.full((R, P), np.nan)
    lml = np.full(R, np.nan)
    iters, evals, status = (np.zeros(R, dtype=np.int32) for _ in range(3))
    ip = C.POINTER(C.c_int)
    check(lib.gpt_batch_optimize(int(device), dptr(X), dptr(Y), n_begin.ctypes.data_as(C.POINTER(_i64)), B, D, Y.shape[1], int(n_ls),
                                 run_model.ctypes.data_as(ip), dptr(theta0), R, dptr(bounds), float(alpha), int(kernel_type), float(pgtol),
                                 float(ftol), int(max_iter), int(max_evals), int(evals_per_launch), dptr(theta), dptr(lml),
                                 iters.ctypes.data_as(ip), evals.ctypes.data_as(ip), status.ctypes.data_as(ip)), "gpt_batch_optimize")
    # per round one launch for every size class that still has a live run; a run with E evaluations is live for ceil(E / epl) rounds
    large = np.diff(n_begin)[run_model] > 32
    launches = sum(int(-(-int(evals[large == cls].max()) // int(evals_per_launch))) for cls in (False, True) if (large == cls).any())
    return theta, lml, iters, evals, status, launches


def batch_optimize_bounded_packed(X, Y, n_begin, n_ls, run_model, theta0, run_bounds, alpha, kernel_type=0, device=0, pgtol=1e-5,
                                  ftol=2.22e-9, max_iter=15000, max_evals=15000, evals_per_launch=None):
    """gpt_batch_optimize_bounded: batch_optimize_packed with bounds of its own for every run, run_bounds (R, 2 + n_ls, 2).  A run's
    results are, bit for bit, those of batch_optimize_packed with that run's bounds shared.  Returns the same tuple."""
    who = "batch_optimize_bounded"
    B, D = n_begin.size - 1, X.shape[1]
    P = 2 + int(n_ls)
    run_model = np.ascontiguousarray(run_model, dtype=np.int32)
    theta0 = as_f64(theta0, 2, "theta0")
    run_bounds = as_f64(run_bounds, 3, "run_bounds")
    R = run_model.size
    if not 1 <= R <= BATCH_MAX_R:
        raise ValueError(f"{who}: a call holds 1 .. 2^20 runs, got {R}")
    if theta0.shape != (R, P) or run_bounds.shape != (R, P, 2):
        raise ValueError(f"{who}: theta0 must be (R, 2 + n_ls) = ({R}, {P}) and run_bounds (R, 2 + n_ls, 2), got {theta0.shape} and "
                         f"{run_bounds.shape}")
    if evals_per_launch is None:
        evals_per_launch = batch_opt_evals_per_launch()
    lib = load()
    require_gpu()
    theta = np.full((R, P), np.nan)
    lml = np.full(R, np.nan)
    iters, evals, status = (np.zeros(R, dtype=np.int32) for _ in range(3))
    ip = C.POINTER(C.c_int)
    check(lib.gpt_batch_optimize_bounded(int(device), dptr(X), dptr(Y), n_begin.ctypes.data_as(C.POINTER(_i64)), B, D, Y.shape[1], int(n_ls),
                                         run_model.ctypes.data_as(ip), dptr(theta0), R, dptr(run_bounds), float(alpha), int(kernel_type),
                                         float(pgtol), float(ftol), int(max_iter), int(max_evals), int(evals_per_launch), dptr(theta),
                                         dptr(lml), iters.ctypes.data_as(ip), evals.ctypes.data_as(ip), status.ctypes.data_as(ip)),
          "gpt_batch_optimize_bounded")
    large = np.diff(n_begin)[run_model] > 32
    launches = sum(int(-(-int(evals[large == cls].max()) // int(evals_per_launch))) for cls in (False, True) if (large == cls).any())
    return theta, lml, iters, evals, status, launches


FOLD_SCAN_MAX_D = 3


def batch_fold_scan_packed(X, Y, n_begin, length_scale, constant_value, noise_level, alpha, Xq, q_begin=None, surrogate=True,
                           per_query=False, kernel_type=0, device=0):
    """gpt_batch_fold_scan on arrays in the ragged layout (batch_pack): does x -> x + psi_b(x) fold on its queries, psi_b the
    posterior mean of model b (Y (sum n_b, D): a displacement, D <= 3, RBF).  q_begin None: every model scans the same Xq (M, D);
    otherwise Xq (sum M_b, D) with q_begin (B + 1).  surrogate: also the error of the reference's inverse surrogate (the GP on
    X + Y -> -Y at the same hyper-parameters).  Returns a dict: min_det (B,), argmin (B,), n_fold (B,), err_sum (B,), err_max (B,),
    status (B,), surrogate_status (B,), and with per_query det, z, err (lists of per-model arrays).  NaN (-1 in argmin and n_fold)
    wherever the call left an output untouched: a model that is not PD, the err outputs without the surrogate or where the
    surrogate's matrix is not PD."""
    who = "batch_fold_scan"
    X = np.ascontiguousarray(X, dtype=np.float64)
    Y = np.ascontiguousarray(Y, dtype=np.float64)
    n_begin = np.ascontiguousarray(n_begin, dtype=np.int64)
    B, D = n_begin.size - 1, X.shape[1]
    if D > FOLD_SCAN_MAX_D:
        raise ValueError(f"{who}: D must be 1 .. {FOLD_SCAN_MAX_D} (the map x -> x + psi(x) is a displacement of the input space), got D = {D}")
    if Y.shape != X.shape:
        raise ValueError(f"{who}: Y must be of shape (n_b, D) = {X.shape}, a displacement per source point, got {Y.shape}")
    ls, c, noise = _batch_hyper(B, D, length_scale, constant_value, noise_level, who)
    Xq = np.ascontiguousarray(Xq, dtype=np.float64).reshape(-1, D)
    if q_begin is None:
        M, o_begin, qp = Xq.shape[0], np.arange(B + 1, dtype=np.int64) * Xq.shape[0], None
    else:
        o_begin = np.ascontiguousarray(q_begin, dtype=np.int64)
        if o_begin.shape != (B + 1,) or o_begin.max() > Xq.shape[0]:
            raise ValueError(f"{who}: q_begin must have B + 1 = {B + 1} entries ending within the {Xq.shape[0]} rows of Xq")
        M, qp = int(o_begin[-1]), o_begin.ctypes.data_as(C.POINTER(_i64))
    rows = max(int(o_begin.max()), 0)
    lib = load()
    require_gpu()
    out = dict(min_det=np.full(B, np.nan), argmin=np.full(B, -1, dtype=np.int64), n_fold=np.full(B, -1, dtype=np.int64),
               err_sum=np.full(B, np.nan), err_max=np.full(B, np.nan), status=np.zeros(B, dtype=np.int32),
               surrogate_status=np.zeros(B, dtype=np.int32))
    det, z, err = (np.full(shape, np.nan) if per_query else None for shape in ((rows,), (rows, D), (rows,)))
    ip, lp = C.POINTER(C.c_int), C.POINTER(_i64)
    check(lib.gpt_batch_fold_scan(int(device), dptr(X), dptr(Y), n_begin.ctypes.data_as(lp), B, D, dptr(ls), ls.shape[1], dptr(c), dptr(noise),
                                  float(alpha), int(kernel_type), dptr(Xq), qp, M, int(bool(surrogate)), dptr(out["min_det"]),
                                  out["argmin"].ctypes.data_as(lp), out["n_fold"].ctypes.data_as(lp), dptr(out["err_sum"]),
                                  dptr(out["err_max"]), dptr(det), dptr(z), dptr(err), out["status"].ctypes.data_as(ip),
                                  out["surrogate_status"].ctypes.data_as(ip)), "gpt_batch_fold_scan")
    if per_query:
        out.update(det=_split(det, o_begin), z=_split(z, o_begin), err=_split(err, o_begin))
    return out


def batch_fold_scan(Xs, Ys, length_scale, constant_value, noise_level, alpha, xq, surrogate=True, per_query=False, kernel_type=0, device=0):
    """batch_fold_scan_packed from sequences of (n_b, D) arrays.  xq: one (M, D) array that every model scans, or a sequence of B
    arrays (M_b, D), M_b >= 0."""
    X, Y, n_begin = batch_pack(Xs, Ys, "batch_fold_scan")
    if isinstance(xq, np.ndarray) and xq.ndim == 2:
        return batch_fold_scan_packed(X, Y, n_begin, length_scale, constant_value, noise_level, alpha, xq, None, surrogate, per_query,
                                      kernel_type, device)
    xqs = [np.asarray(x, dtype=np.float64).reshape(-1, X.shape[1]) for x in xq]
    if len(xqs) != n_begin.size - 1:
        raise ValueError(f"batch_fold_scan: {n_begin.size - 1} models but {len(xqs)} query arrays")
    q_begin = np.zeros(len(xqs) + 1, dtype=np.int64)
    np.cumsum([x.shape[0] for x in xqs], out=q_begin[1:])
    return batch_fold_scan_packed(X, Y, n_begin, length_scale, constant_value, noise_level, alpha, np.concatenate(xqs), q_begin, surrogate,
                                  per_query, kernel_type, device)


def batch_lml_objective(Xs, Ys, length_scale, constant_value, noise_level, alpha, kernel_type=0, device=0):
    """LML and its gradient with respect to log [c, l.., noise] of B independent small models in one launch
    (gpt_batch_lml_objective).  Xs, Ys: sequences of (n_b, D) / (n_b, O) arrays; length_scale (B, 1 or D), constant_value (B,),
    noise_level (B,).  Returns (lml (B,), grad (B, 2 + n_ls), status (B,))."""
    X, Y, n_begin = batch_pack(Xs, Ys, "batch_lml_objective")
    return batch_lml_objective_packed(X, Y, n_begin, length_scale, constant_value, noise_level, alpha, kernel_type, device)


def batch_fit(Xs, Ys, length_scale, constant_value, noise_level, alpha, kernel_type=0, device=0, want_L=True):
    """sklearn's fitted attributes of B independent small models (gpt_batch_fit): (L list of (n_b, n_b) or None, alpha list of
    (n_b, O), lml (B,), status (B,)); the arrays of a model that is not PD hold NaN."""
    X, Y, n_begin = batch_pack(Xs, Ys, "batch_fit")
    B, D = n_begin.size - 1, X.shape[1]
    ls, c, noise = _batch_hyper(B, D, length_scale, constant_value, noise_level, "batch_fit")
    lib = load()
    require_gpu()
    sizes = np.diff(n_begin)
    l_begin = np.concatenate([[0], np.cumsum(sizes * sizes)])
    L = np.full(l_begin[-1], np.nan) if want_L else None
    a = np.full(Y.shape, np.nan)
    lml = np.full(B, np.nan)
    status = np.zeros(B, dtype=np.int32)
    check(lib.gpt_batch_fit(int(device), dptr(X), dptr(Y), n_begin.ctypes.data_as(C.POINTER(_i64)), B, D, Y.shape[1], dptr(ls), ls.shape[1],
                            dptr(c), dptr(noise), float(alpha), int(kernel_type), dptr(L), dptr(a), dptr(lml),
                            status.ctypes.data_as(C.POINTER(C.c_int))), "gpt_batch_fit")
    Ls = [L[l_begin[b]:l_begin[b + 1]].reshape(sizes[b], sizes[b]) for b in range(B)] if want_L else None
    return Ls, _split(a, n_begin), lml, status


def batch_predict(Xs, Ys, length_scale, constant_value, noise_level, alpha, xqs, kernel_type=0, device=0, mean=False, var=False, J=False,
                  Jvar=False, dvar=False):
    """The fused posterior of B independent small models, each at its own queries xqs[b] (M_b, D), M_b >= 0
    (gpt_batch_predict).  Returns ({name: list of per-model arrays} for the outputs asked for — mean (M_b, O), var (M_b,),
    J (M_b, O, D), Jvar (M_b, D), dvar (M_b, D) — and status (B,)); a model that is not PD has NaN in its arrays."""
    X, Y, n_begin = batch_pack(Xs, Ys, "batch_predict")
    B, D, O = n_begin.size - 1, X.shape[1], Y.shape[1]
    ls, c, noise = _batch_hyper(B, D, length_scale, constant_value, noise_level, "batch_predict")
    xqs = [as_f64(x, 2, "X") for x in xqs]
    if len(xqs) != B:
        raise ValueError(f"batch_predict: {B} models but {len(xqs)} query arrays")
    for b, x in enumerate(xqs):
        if x.shape[1] != D:
            raise ValueError(f"batch_predict: the queries of model {b} have {x.shape[1]} features, the models {D}")
    q_begin = np.zeros(B + 1, dtype=np.int64)
    np.cumsum([x.shape[0] for x in xqs], out=q_begin[1:])
    M = int(q_begin[-1])
    if M >= 2 ** 31:
        raise ValueError("batch_predict: the queries of one call must number fewer than 2^31")
    Xq = np.concatenate(xqs) if M else np.zeros((0, D))
    lib = load()
    require_gpu()
    shapes = {"mean": (M, O), "var": (M,), "J": (M, O, D), "Jvar": (M, D), "dvar": (M, D)}
    want = {"mean": mean, "var": var, "J": J, "Jvar": Jvar, "dvar": dvar}
    out = {k: (np.full(shapes[k], np.nan) if want[k] else None) for k in shapes}
    status = np.zeros(B, dtype=np.int32)
    ip = C.POINTER(_i64)
    check(lib.gpt_batch_predict(int(device), dptr(X), dptr(Y), n_begin.ctypes.data_as(ip), B, D, O, dptr(ls), ls.shape[1], dptr(c),
                                dptr(noise), float(alpha), int(kernel_type), dptr(Xq), q_begin.ctypes.data_as(ip), dptr(out["mean"]),
                                dptr(out["var"]), dptr(out["J"]), dptr(out["Jvar"]), dptr(out["dvar"]),
                                status.ctypes.data_as(C.POINTER(C.c_int))), "gpt_batch_predict")
    return {k: _split(v, q_begin) for k, v in out.items() if v is not None}, status


class Handle:
    """Owns one gpt_handle (one fitted model on one GPU)."""

    def __init__(self, device: int = 0):
        self.lib = load()
        require_gpu()
        h = _vp()
        check(self.lib.gpt_create(C.byref(h), int(device)), "gpt_create")
        self._h = h
        self.device = int(device)

    def close(self):
        if getattr(self, "_h", None):
            self.lib.gpt_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- fit / export
    def set_dtype(self, dtype):
        """Element type of the models fitted from now on: GPT_F64 (default) or GPT_F32."""
        check(self.lib.gpt_set_dtype(self._h, int(dtype)), "gpt_set_dtype")

    def set_matern_derivatives(self, enable=True):
        """J / Jvar / dvar of Matern 3/2 and 5/2 models: the analytic derivatives of the posterior (default: refused)."""
        check(self.lib.gpt_set_matern_derivatives(self._h, int(bool(enable))), "gpt_set_matern_derivatives")

    def fit(self, X, Y, length_scale, constant_value, noise_level, alpha, kernel_type=0):
        """kernel_type: 0 RBF, 1/2/3 Matern nu = 0.5 / 1.5 / 2.5 (GPT_KERNEL_* of include/gpt_hip.h)."""
        X = as_f64(X, 2, "X")
        Y = as_f64(Y, 2, "y")
        ls = as_f64(np.atleast_1d(length_scale), 1, "length_scale")
        N, D = X.shape
        if Y.shape[0] != N:
            raise ValueError("X and Y have different numbers of rows")
        if not 1 <= D <= MAX_D:
            raise ValueError(f"X has {D} features: this GPU path supports input dimension D = 1 .. {MAX_D} only")
        check(self.lib.gpt_fit_kernel(self._h, dptr(X), dptr(Y), N, D, Y.shape[1], dptr(ls), ls.size,
                                      float(constant_value), float(noise_level), float(alpha), int(kernel_type)), "gpt_fit")

    def fit_noise_matrix(self, X, Y, length_scale, constant_value, Sigma, alpha=0.0, kernel_type=0):
        """K = c k(X,X) + Sigma (full SPD (N,N)) + alpha I — the SVGP exact-conversion model."""
        X = as_f64(X, 2, "X")
        Y = as_f64(Y, 2, "y")
        Sigma = as_f64(Sigma, 2, "Sigma")
        ls = as_f64(np.atleast_1d(length_scale), 1, "length_scale")
        N, D = X.shape
        if Y.shape[0] != N or Sigma.shape != (N, N):
            raise ValueError("X, Y and Sigma disagree on the number of points")
        check(self.lib.gpt_fit_noise_matrix(self._h, dptr(X), dptr(Y), N, D, Y.shape[1], dptr(ls), ls.size,
                                            float(constant_value), dptr(Sigma), float(alpha), int(kernel_type)),
              "gpt_fit_noise_matrix")

    def fit_svgp(self, Z, y, Sigma, length_scale, outputscale, jitter=0.0, dtype=GPT_F64):
        """The multi-task SVGP exact-conversion model in one handle (gpt_fit_svgp): Z (N,D), y (T,N), Sigma (T,N,N),
        outputscale (T,), length_scale (1 or D)."""
        Z = as_f64(Z, 2, "Z")
        y = as_f64(y, 2, "y")
        Sigma = as_f64(Sigma, 3, "Sigma")
        ls = as_f64(np.atleast_1d(length_scale), 1, "length_scale")
        osc = as_f64(np.atleast_1d(outputscale), 1, "outputscale")
        N, D = Z.shape
        T = y.shape[0]
        if y.shape != (T, N) or Sigma.shape != (T, N, N) or osc.shape != (T,):
            raise ValueError("expected y (T,N), Sigma (T,N,N), outputscale (T,)")
        check(self.lib.gpt_fit_svgp(self._h, dptr(Z), dptr(y), dptr(Sigma), N, D, T, dptr(ls), ls.size, dptr(osc),
                                    float(jitter), int(dtype)), "gpt_fit_svgp")

    def model_info(self):
        """(n_tasks, dtype) of the fitted model."""
        nt, dt = C.c_int(), C.c_int()
        check(self.lib.gpt_model_info(self._h, C.byref(nt), C.byref(dt)), "gpt_model_info")
        return nt.value, dt.value

    def info(self):
        N, NP, D, O = _i64(), _i64(), C.c_int(), C.c_int()
        check(self.lib.gpt_info(self._h, C.byref(N), C.byref(D), C.byref(O), C.byref(NP)), "gpt_info")
        return N.value, D.value, O.value, NP.value

    def export(self, want_L=True, want_alpha=True):
        N, D, O, _ = self.info()
        L = np.empty((N, N)) if want_L else None
        a = np.empty((N, O)) if want_alpha else None
        check(self.lib.gpt_export(self._h, dptr(L), dptr(a)), "gpt_export")
        return L, a

    def export_inverse_factor(self):
        N = self.info()[0]
        W = np.empty((N, N))
        check(self.lib.gpt_export_inverse_factor(self._h, dptr(W)), "gpt_export_inverse_factor")
        return W

    def apply_inverse(self, R):
        """(K + sigma^2 I)^-1 R for the columns of R (N,C) or one column (N,), with the inverse factor of this handle's own fit
        (gpt_apply_inverse: the launches that compute alpha in the fit, four columns per pass).  R = Y gives the alpha of
        export(), bit for bit; a column's result does not depend on the other columns.  float64, single-task, exact-GP models."""
        N = self.info()[0]
        R = np.ascontiguousarray(R, dtype=np.float64)
        one = R.ndim == 1
        R2 = R.reshape(N, -1) if one and R.shape == (N,) else R
        if R2.ndim != 2 or R2.shape[0] != N:
            raise ValueError(f"apply_inverse: R has shape {R.shape}, expected ({N}, C) or ({N},): one row per training point")
        out = np.empty_like(R2)
        check(self.lib.gpt_apply_inverse(self._h, dptr(R2), R2.shape[1], dptr(out)), "gpt_apply_inverse")
        return out[:, 0] if one else out

    def debug_set_inverse_factor(self, W):
        """Replace the inverse factor of this handle's own fit by the dense (N, N) float64 array W (gpt_debug_set_inverse_factor;
        tests only): the variance kernels then work on W's lower triangle, LML calls refuse until the next fit."""
        if not (isinstance(W, np.ndarray) and W.dtype == np.float64 and W.ndim == 2 and W.shape[0] == W.shape[1] and W.flags.c_contiguous):
            raise ValueError("debug_set_inverse_factor: W must be a square C-contiguous float64 array")
        check(self.lib.gpt_debug_set_inverse_factor(self._h, dptr(W), W.shape[0]), "gpt_debug_set_inverse_factor")

    def debug_set_task_inverse_factor(self, task, W):
        """The same for task `task` of a gpt_fit_svgp model (gpt_debug_set_task_inverse_factor; tests only): W is packed into the
        task's slot times the task's outputscale, as the fit packs it."""
        if not (isinstance(W, np.ndarray) and W.dtype == np.float64 and W.ndim == 2 and W.shape[0] == W.shape[1] and W.flags.c_contiguous):
            raise ValueError("debug_set_task_inverse_factor: W must be a square C-contiguous float64 array")
        check(self.lib.gpt_debug_set_task_inverse_factor(self._h, int(task), dptr(W), W.shape[0]), "gpt_debug_set_task_inverse_factor")

    def lml(self) -> float:
        v = C.c_double()
        check(self.lib.gpt_lml(self._h, C.byref(v)), "gpt_lml")
        return v.value

    def lml_gradient(self, n_ls):
        v = C.c_double()
        g = np.zeros(2 + int(n_ls))
        check(self.lib.gpt_lml_gradient(self._h, C.byref(v), dptr(g)), "gpt_lml_gradient")
        return v.value, g

    def lml_objective(self, X, Y, length_scale, constant_value, noise_level, alpha, kernel_type=0):
        """(lml, gradient w.r.t. theta = log [c, length_scale..., noise]) for these hyper-parameters in one call; the
        handle holds no model afterwards.  X, Y as for fit (validated by the caller once: the optimizer calls this
        hundreds of times on the same arrays)."""
        ls = np.ascontiguousarray(np.atleast_1d(length_scale), dtype=np.float64)
        v = C.c_double()
        g = np.zeros(2 + ls.size)
        N, D = X.shape
        check(self.lib.gpt_lml_objective(self._h, dptr(X), dptr(Y), N, D, Y.shape[1], dptr(ls), ls.size, float(constant_value),
                                         float(noise_level), float(alpha), int(kernel_type), C.byref(v), dptr(g)), "gpt_lml_objective")
        return v.value, g

    def fit_timings(self):
        t = np.zeros(6)
        check(self.lib.gpt_fit_timings(self._h, dptr(t), 6), "gpt_fit_timings")
        return dict(zip(["total", "gram", "cholesky", "inverse", "alpha", "pack"], t.tolist()))

    # ---- predict (host buffers)
    def predict_all(self, Xq, mean=False, var=False, J=False, Jvar=False, dvar=False):
        """Arrays come back in the model's element type (float64, or float32 for a GPT_F32 model); the multi-task
        model returns var (M,T) and Jvar (M,T,D)."""
        N, D, O, _ = self.info()
        nt, dt = self.model_info()
        ty = _NP_DTYPE[dt]
        Xq = as_f64(Xq, 2, "X", dtype=ty)
        if Xq.shape[1] != D:
            raise ValueError(f"query has {Xq.shape[1]} features, model was fitted with {D}")
        M = Xq.shape[0]
        vshape, jvshape = ((M,), (M, D)) if nt == 1 else ((M, nt), (M, nt, D))
        out = {
            "mean": np.empty((M, O), dtype=ty) if mean else None,
            "var": np.empty(vshape, dtype=ty) if var else None,
            "J": np.empty((M, O, D), dtype=ty) if J else None,
            "Jvar": np.empty(jvshape, dtype=ty) if Jvar else None,
            "dvar": np.empty((D, M), dtype=ty) if dvar else None,
        }
        check(self.lib.gpt_predict_all(self._h, vptr(Xq), M, vptr(out["mean"]), vptr(out["var"]), vptr(out["J"]),
                                       vptr(out["Jvar"]), vptr(out["dvar"])), "gpt_predict_all")
        return out

    def predict_cov(self, Xq):
        N, D, O, _ = self.info()
        Xq = as_f64(Xq, 2, "X")
        if Xq.shape[1] != D:
            raise ValueError(f"query has {Xq.shape[1]} features, model was fitted with {D}")
        M = Xq.shape[0]
        mean, cov = np.empty((M, O)), np.empty((M, M))
        check(self.lib.gpt_predict_cov(self._h, dptr(Xq), M, dptr(mean), dptr(cov)), "gpt_predict_cov")
        return mean, cov

    # ---- inverse of the displacement map
    def inverse_map(self, y, z0=None, rtol=1e-10, max_passes=64):
        """The z (M,D) with z + mean(z) = y for each row of y, by damped Newton on the device (gpt_inverse_map), started at
        z0 (default: y).  Returns (z, info): info["status"] (M,) int32 INV_*, info["passes"] (M,) int32, info["residual"] (M,)
        = |z + mean(z) - y| and info["det"] (M,) = det(I + J(z)) at the returned point."""
        N, D, O, _ = self.info()
        y = as_f64(y, 2, "y")
        if y.shape[1] != D:
            raise ValueError(f"y has {y.shape[1]} columns, model was fitted with {D} features")
        if z0 is not None:
            z0 = as_f64(z0, 2, "z0")
            if z0.shape != y.shape:
                raise ValueError(f"z0 has shape {z0.shape}, y {y.shape}")
        M = y.shape[0]
        z = np.empty((M, D))
        info = {"status": np.empty(M, dtype=np.int32), "passes": np.empty(M, dtype=np.int32), "residual": np.empty(M),
                "det": np.empty(M)}
        ip = C.POINTER(C.c_int)
        check(self.lib.gpt_inverse_map(self._h, dptr(y), dptr(z0), M, float(rtol), int(max_passes), dptr(z), dptr(info["residual"]),
                                       dptr(info["det"]), info["passes"].ctypes.data_as(ip), info["status"].ctypes.data_as(ip)),
              "gpt_inverse_map")
        return z, info

    def inverse_map_dev(self, y_ptr, M, z_ptr, status_ptr, z0_ptr=0, residual_ptr=0, det_ptr=0, passes_ptr=0, rtol=1e-10, max_passes=64):
        """The same on device pointers (float64 / int32), asynchronous on the handle's stream (gpt_inverse_map_dev)."""
        check(self.lib.gpt_inverse_map_dev(self._h, _vp(y_ptr), _vp(z0_ptr or None), int(M), float(rtol), int(max_passes), _vp(z_ptr),
                                           _vp(residual_ptr or None), _vp(det_ptr or None), _vp(passes_ptr or None), _vp(status_ptr)),
              "gpt_inverse_map_dev")

    # ---- transport: affine part, posterior and push-forward in one call
    def transport_policy(self, pos, R, c_src, c_dst, scale=1.0, R_jac=None, vel=None, ori=None, outputs=TRANSPORT_OUTPUTS):
        """gpt_transport_policy on host arrays: pos (M,D) through gamma(x) = scale R (x - c_src) + c_dst and the fitted
        displacement, velocities vel (M,D) and orientations ori (M,4; w,x,y,z) along.  R_jac: the Jacobian of gamma as the
        caller defines it (default R).  `outputs`: names out of TRANSPORT_OUTPUTS; pos_out always comes, vel_out / vel_var
        are left out without vel and ori_out without ori; ori_gap needs no ori (it is a property of the Jacobian at pos) and
        is left out only where there is no quaternion to speak of, D != 3 (orientations GIVEN to a model with D != 3:
        ValueError from the library).  Returns a dict."""
        N, D, O, _ = self.info()
        pos = as_f64(pos, 2, "pos")
        if pos.shape[1] != D:
            raise ValueError(f"pos has {pos.shape[1]} columns, model was fitted with {D} features")
        M = pos.shape[0]
        R = as_f64(R, 2, "R")
        R_jac = R if R_jac is None else as_f64(R_jac, 2, "R_jac")
        c_src, c_dst = as_f64(c_src, 1, "c_src"), as_f64(c_dst, 1, "c_dst")
        if R.shape != (D, D) or R_jac.shape != (D, D) or c_src.shape != (D,) or c_dst.shape != (D,):
            raise ValueError(f"the affine part of a {D}-dimensional model is R ({D},{D}), R_jac ({D},{D}), c_src ({D},), c_dst ({D},)")
        if vel is not None:
            vel = as_f64(vel, 2, "vel")
            if vel.shape != pos.shape:
                raise ValueError(f"vel has shape {vel.shape}, pos {pos.shape}")
        if ori is not None:
            ori = as_f64(ori, 2, "ori")
            if ori.shape != (M, 4):
                raise ValueError(f"ori has shape {ori.shape}, expected ({M}, 4)")
        unknown = set(outputs) - set(TRANSPORT_OUTPUTS)
        if unknown:
            raise ValueError(f"transport_policy: unknown outputs {sorted(unknown)}")
        shapes = {"pos_rot": (M, D), "pos_out": (M, D), "var": (M,), "vel_out": (M, D), "vel_var": (M,), "det_vel": (M,),
                  "ori_out": (M, 4), "det_ori": (M,), "ori_gap": (M,), "post_mean": (M, D), "post_J": (M, D, D),
                  "post_Jvar": (M, D), "post_J_ori": (M, D, D)}
        missing = set()
        if vel is None:
            missing |= {"vel_out", "vel_var"}
        if ori is None:
            missing |= {"ori_out"} | ({"ori_gap"} if D != 3 else set())
        want = [k for k in TRANSPORT_OUTPUTS if k == "pos_out" or (k in outputs and k not in missing)]
        out = {k: np.empty(shapes[k]) for k in want}
        check(self.lib.gpt_transport_policy(self._h, dptr(pos), M, dptr(R), dptr(c_src), dptr(c_dst), float(scale), dptr(R_jac),
                                            dptr(vel), dptr(ori), *(dptr(out.get(k)) for k in TRANSPORT_OUTPUTS)),
              "gpt_transport_policy")
        return out

    def transport_policy_dev(self, pos_ptr, M, R_ptr, c_src_ptr, c_dst_ptr, scale, R_jac_ptr, pos_out_ptr, vel_ptr=0, ori_ptr=0, **out_ptrs):
        """The same on device pointers (float64, the affine part included), asynchronous on the handle's stream
        (gpt_transport_policy_dev).  out_ptrs: <name>_ptr for the further names of TRANSPORT_OUTPUTS."""
        ptrs = dict(out_ptrs, pos_out_ptr=pos_out_ptr)
        unknown = set(ptrs) - {k + "_ptr" for k in TRANSPORT_OUTPUTS}
        if unknown:
            raise TypeError(f"transport_policy_dev: unknown arguments {sorted(unknown)}")
        check(self.lib.gpt_transport_policy_dev(self._h, _vp(pos_ptr or None), int(M), _vp(R_ptr or None), _vp(c_src_ptr or None),
                                                _vp(c_dst_ptr or None), float(scale), _vp(R_jac_ptr or None), _vp(vel_ptr or None),
                                                _vp(ori_ptr or None), *(_vp(ptrs.get(k + "_ptr") or None) for k in TRANSPORT_OUTPUTS)),
              "gpt_transport_policy_dev")

    # ---- the transported policy at target-space points: inverse, dynamics and push-forward in one call
    def pullback_policy(self, dyn, y, R, c_src, c_dst, scale=1.0, R_jac=None, x0=None, rtol=1e-10, max_passes=64, std_offset=0.0,
                        outputs=PULLBACK_OUTPUTS):
        """gpt_pullback_policy on host arrays, this handle the map: for each row of y (M,D) the preimage x under
        Phi = gamma + psi o gamma (gamma(x) = scale R (x - c_src) + c_dst, psi this handle's mean; damped Newton as inverse_map,
        started at gamma(x0) or y), the mean f of the handle `dyn` at x and vel = (I + J_psi) R_jac f.  R_jac: the Jacobian of
        gamma as the caller defines it (default R).  `outputs`: names out of PULLBACK_OUTPUTS; vel and status always come.
        Returns a dict."""
        N, D, O, _ = self.info()
        y = as_f64(y, 2, "y")
        if y.shape[1] != D:
            raise ValueError(f"y has {y.shape[1]} columns, model was fitted with {D} features")
        M = y.shape[0]
        if x0 is not None:
            x0 = as_f64(x0, 2, "x0")
            if x0.shape != y.shape:
                raise ValueError(f"x0 has shape {x0.shape}, y {y.shape}")
        R = as_f64(R, 2, "R")
        R_jac = R if R_jac is None else as_f64(R_jac, 2, "R_jac")
        c_src, c_dst = as_f64(c_src, 1, "c_src"), as_f64(c_dst, 1, "c_dst")
        if R.shape != (D, D) or R_jac.shape != (D, D) or c_src.shape != (D,) or c_dst.shape != (D,):
            raise ValueError(f"the affine part of a {D}-dimensional model is R ({D},{D}), R_jac ({D},{D}), c_src ({D},), c_dst ({D},)")
        unknown = set(outputs) - set(PULLBACK_OUTPUTS)
        if unknown:
            raise ValueError(f"pullback_policy: unknown outputs {sorted(unknown)}")
        shapes = {"x": (M, D), "vel": (M, D), "f": (M, D), "det": (M,), "residual": (M,), "passes": (M,), "status": (M,),
                  "var_dyn": (M,), "map_var": (M,), "vel_var_map": (M,), "vel_var_dyn": (M, D), "post_z": (M, D), "post_A": (M, D, D),
                  "post_Jvar": (M, D)}
        want = [k for k in PULLBACK_OUTPUTS if k in ("vel", "status") or k in outputs]
        out = {k: np.empty(shapes[k], dtype=np.int32 if k in ("passes", "status") else np.float64) for k in want}
        ip = C.POINTER(C.c_int)
        ptr = lambda k: (None if k not in out else out[k].ctypes.data_as(ip)) if k in ("passes", "status") else dptr(out.get(k))
        check(self.lib.gpt_pullback_policy(self._h, dyn._h, dptr(y), dptr(x0), M, dptr(R), dptr(c_src), dptr(c_dst), float(scale),
                                           dptr(R_jac), float(rtol), int(max_passes), float(std_offset),
                                           *(ptr(k) for k in PULLBACK_OUTPUTS)),
              "gpt_pullback_policy")
        return out

    def pullback_policy_dev(self, dyn, y_ptr, M, R_ptr, c_src_ptr, c_dst_ptr, scale, R_jac_ptr, vel_ptr, status_ptr, x0_ptr=0, rtol=1e-10,
                            max_passes=64, std_offset=0.0, **out_ptrs):
        """The same on device pointers (float64; passes / status int32; the affine part included), asynchronous on this handle's
        stream (gpt_pullback_policy_dev).  out_ptrs: <name>_ptr for the further names of PULLBACK_OUTPUTS."""
        ptrs = dict(out_ptrs, vel_ptr=vel_ptr, status_ptr=status_ptr)
        unknown = set(ptrs) - {k + "_ptr" for k in PULLBACK_OUTPUTS}
        if unknown:
            raise TypeError(f"pullback_policy_dev: unknown arguments {sorted(unknown)}")
        check(self.lib.gpt_pullback_policy_dev(self._h, dyn._h, _vp(y_ptr or None), _vp(x0_ptr or None), int(M), _vp(R_ptr or None),
                                               _vp(c_src_ptr or None), _vp(c_dst_ptr or None), float(scale), _vp(R_jac_ptr or None),
                                               float(rtol), int(max_passes), float(std_offset),
                                               *(_vp(ptrs.get(k + "_ptr") or None) for k in PULLBACK_OUTPUTS)),
              "gpt_pullback_policy_dev")

    # ---- the transported policy through a chain of transports: K inverses, dynamics and push-forward in one call
    def pullback_chain(self, inner, dyn, y, x0=None, rtol=1e-10, max_passes=64, std_offset=0.0, outputs=CHAIN_OUTPUTS):
        """gpt_pullback_chain on host arrays, this handle the LAST stage of the chain (it owns the call's scratch and stream).
        `inner`: the K stages in application order, stage 0 first, each a tuple (handle, R, c_src, c_dst, scale, R_jac) with
        R_jac None for R; the last tuple's handle is this one.  For each row of y (M,D): the preimage x under Phi_{K-1} o ... o
        Phi_0, the mean f of the handle `dyn` at x and vel = J_Phi(x) f; x0 (M,D): guesses of the source-space preimages.
        `outputs`: names out of CHAIN_OUTPUTS; vel and status always come.  Returns a dict; the stage_* arrays are (K, M, ...)."""
        stages = list(inner)
        K = len(stages)
        if not 1 <= K <= CHAIN_MAX:
            raise ValueError(f"pullback_chain: 1 .. {CHAIN_MAX} stages, got {K}")
        if stages[-1][0] is not self:
            raise ValueError("pullback_chain: the last stage's handle must be the handle the call is made on")
        N, D, O, _ = self.info()
        y = as_f64(y, 2, "y")
        if y.shape[1] != D:
            raise ValueError(f"y has {y.shape[1]} columns, model was fitted with {D} features")
        M = y.shape[0]
        if x0 is not None:
            x0 = as_f64(x0, 2, "x0")
            if x0.shape != y.shape:
                raise ValueError(f"x0 has shape {x0.shape}, y {y.shape}")
        unknown = set(outputs) - set(CHAIN_OUTPUTS)
        if unknown:
            raise ValueError(f"pullback_chain: unknown outputs {sorted(unknown)}")
        keep = []                                # the affine arrays live until the call returns
        arr = (ChainStage * K)()
        for k, (h, R, c_src, c_dst, scale, R_jac) in enumerate(stages):
            R = as_f64(R, 2, "R")
            R_jac = R if R_jac is None else as_f64(R_jac, 2, "R_jac")
            c_src, c_dst = as_f64(c_src, 1, "c_src"), as_f64(c_dst, 1, "c_dst")
            if R.shape != (D, D) or R_jac.shape != (D, D) or c_src.shape != (D,) or c_dst.shape != (D,):
                raise ValueError(f"stage {k}: the affine part of a {D}-dimensional model is R ({D},{D}), R_jac ({D},{D}), c_src ({D},), "
                                 f"c_dst ({D},)")
            keep += [R, R_jac, c_src, c_dst]
            arr[k] = ChainStage(h._h, R.ctypes.data, c_src.ctypes.data, c_dst.ctypes.data, R_jac.ctypes.data, float(scale))
        shapes = {"x": (M, D), "vel": (M, D), "f": (M, D), "status": (M,), "var_dyn": (M,), "vel_var_map": (M, D), "vel_var_dyn": (M, D),
                  "stage_x": (K, M, D), "stage_z": (K, M, D), "stage_A": (K, M, D, D), "stage_Jvar": (K, M, D), "stage_map_var": (K, M),
                  "stage_status": (K, M), "stage_passes": (K, M), "stage_residual": (K, M), "stage_det": (K, M)}
        want = [k for k in CHAIN_OUTPUTS if k in ("vel", "status") or k in outputs]
        out = {k: np.empty(shapes[k], dtype=np.int32 if k in CHAIN_INT_OUTPUTS else np.float64) for k in want}
        ptr = lambda k: (None if k not in out else out[k].ctypes.data_as(_ip)) if k in CHAIN_INT_OUTPUTS else dptr(out.get(k))
        check(self.lib.gpt_pullback_chain(arr, K, dyn._h, dptr(y), dptr(x0), M, float(rtol), int(max_passes), float(std_offset),
                                          *(ptr(k) for k in CHAIN_OUTPUTS)),
              "gpt_pullback_chain")
        del keep
        return out

    def pullback_chain_dev(self, inner, dyn, y_ptr, M, vel_ptr, status_ptr, x0_ptr=0, rtol=1e-10, max_passes=64, std_offset=0.0, **out_ptrs):
        """The same on device pointers (float64; status / stage_status / stage_passes int32), asynchronous on this handle's stream
        (gpt_pullback_chain_dev).  `inner`: tuples (handle, R_ptr, c_src_ptr, c_dst_ptr, scale, R_jac_ptr), device pointers, the
        last tuple's handle this one.  out_ptrs: <name>_ptr for the further names of CHAIN_OUTPUTS."""
        stages = list(inner)
        K = len(stages)
        if not 1 <= K <= CHAIN_MAX:
            raise ValueError(f"pullback_chain_dev: 1 .. {CHAIN_MAX} stages, got {K}")
        if stages[-1][0] is not self:
            raise ValueError("pullback_chain_dev: the last stage's handle must be the handle the call is made on")
        ptrs = dict(out_ptrs, vel_ptr=vel_ptr, status_ptr=status_ptr)
        unknown = set(ptrs) - {k + "_ptr" for k in CHAIN_OUTPUTS}
        if unknown:
            raise TypeError(f"pullback_chain_dev: unknown arguments {sorted(unknown)}")
        arr = (ChainStage * K)()
        for k, (h, R_ptr, c_src_ptr, c_dst_ptr, scale, R_jac_ptr) in enumerate(stages):
            arr[k] = ChainStage(h._h, R_ptr or None, c_src_ptr or None, c_dst_ptr or None, R_jac_ptr or None, float(scale))
        check(self.lib.gpt_pullback_chain_dev(arr, K, dyn._h, _vp(y_ptr or None), _vp(x0_ptr or None), int(M), float(rtol), int(max_passes),
                                              float(std_offset), *(_vp(ptrs.get(k + "_ptr") or None) for k in CHAIN_OUTPUTS)),
              "gpt_pullback_chain_dev")

    # ---- whole paths of the transported policy: the loop over the steps on the device
    def _rollout_host(self, what, names, optional, extra, inner, dyn, y0, n_steps, dt, x0, rtol, max_passes, outputs, inputs=()):
        """The host entry `gpt_<what>` of a rollout family: `names` its outputs in the order of its arguments, `optional` those the
        caller chooses among, `extra` the arguments between max_passes and the outputs, `inputs` the arrays it takes between
        x0 and M: float64 ones (or None) go as double pointers, int32 ones as int pointers."""
        stages = list(inner)
        K = len(stages)
        if K > CHAIN_MAX:
            raise ValueError(f"{what}: 0 .. {CHAIN_MAX} stages, got {K}")
        if (stages[-1][0] if K else dyn) is not self:
            raise ValueError(f"{what}: the last stage's handle (without stages: dyn) must be the handle the call is made on")
        N, D, O, _ = self.info()
        y0 = as_f64(y0, 2, "y0")
        if y0.shape[1] != D:
            raise ValueError(f"y0 has {y0.shape[1]} columns, model was fitted with {D} features")
        M, T = y0.shape[0], int(n_steps)
        if x0 is not None:
            x0 = as_f64(x0, 2, "x0")
            if x0.shape != y0.shape:
                raise ValueError(f"x0 has shape {x0.shape}, y0 {y0.shape}")
        unknown = set(outputs) - set(optional)
        if unknown:
            raise ValueError(f"{what}: unknown outputs {sorted(unknown)}")
        if T < 0:
            raise ValueError(f"{what}: n_steps must be >= 0")
        if M * (T + 1) >= 2 ** 31:
            raise ValueError(f"{what}: M (n_steps + 1), the rows of path, must be below 2^31")
        keep = []                                # the affine arrays live until the call returns
        arr = (ChainStage * max(K, 1))()
        for k, (h, R, c_src, c_dst, scale, R_jac) in enumerate(stages):
            R = as_f64(R, 2, "R")
            R_jac = R if R_jac is None else as_f64(R_jac, 2, "R_jac")
            c_src, c_dst = as_f64(c_src, 1, "c_src"), as_f64(c_dst, 1, "c_dst")
            if R.shape != (D, D) or R_jac.shape != (D, D) or c_src.shape != (D,) or c_dst.shape != (D,):
                raise ValueError(f"stage {k}: the affine part of a {D}-dimensional model is R ({D},{D}), R_jac ({D},{D}), c_src ({D},), "
                                 f"c_dst ({D},)")
            keep += [R, R_jac, c_src, c_dst]
            arr[k] = ChainStage(h._h, R.ctypes.data, c_src.ctypes.data, c_dst.ctypes.data, R_jac.ctypes.data, float(scale))
        shapes = {"path": (M, T + 1, D), "var": (M, T), "pvar": (M, T), "cvar": (M, T), "chol": (M, T, T), "steps_done": (M,), "status": (M,)}
        want = [k for k in names if k not in optional or k in outputs]
        out = {k: np.empty(shapes.get(k, (M, T, D)), dtype=np.int32 if k in ROLLOUT_INT_OUTPUTS else np.float64) for k in want}
        ptr = lambda k: (None if k not in out else out[k].ctypes.data_as(_ip)) if k in ROLLOUT_INT_OUTPUTS else dptr(out.get(k))
        check(getattr(self.lib, "gpt_" + what)(arr if K else None, K, dyn._h, dptr(y0), dptr(x0), *(a.ctypes.data_as(_ip) if a is not None and a.dtype == np.int32 else dptr(a) for a in inputs), M, T,
                                               float(dt),
                                               float(rtol), int(max_passes), *extra, *(ptr(k) for k in names)),
              "gpt_" + what)
        del keep
        return out

    def _rollout_dev(self, what, names, extra, inner, dyn, y0_ptr, x0_ptr, M, n_steps, dt, rtol, max_passes, ptrs, input_ptrs=()):
        """The device entry `gpt_<what>_dev` of a rollout family; ptrs: output name -> device pointer (0: not asked for);
        input_ptrs: the device pointers it takes between x0 and M."""
        stages = list(inner)
        K = len(stages)
        if K > CHAIN_MAX:
            raise ValueError(f"{what}_dev: 0 .. {CHAIN_MAX} stages, got {K}")
        if (stages[-1][0] if K else dyn) is not self:
            raise ValueError(f"{what}_dev: the last stage's handle (without stages: dyn) must be the handle the call is made on")
        arr = (ChainStage * max(K, 1))()
        for k, (h, R_ptr, c_src_ptr, c_dst_ptr, scale, R_jac_ptr) in enumerate(stages):
            arr[k] = ChainStage(h._h, R_ptr or None, c_src_ptr or None, c_dst_ptr or None, R_jac_ptr or None, float(scale))
        check(getattr(self.lib, f"gpt_{what}_dev")(arr if K else None, K, dyn._h, _vp(y0_ptr or None), _vp(x0_ptr or None),
                                                   *(_vp(q or None) for q in input_ptrs), int(M), int(n_steps),
                                                   float(dt), float(rtol), int(max_passes), *extra, *(_vp(ptrs.get(k) or None) for k in names)),
              f"gpt_{what}_dev")

    def rollout_policy(self, inner, dyn, y0, n_steps, dt=1.0, x0=None, rtol=1e-10, max_passes=64, outputs=("vel", "x")):
        """gpt_rollout_policy on host arrays: n_steps explicit Euler steps y += dt * vel from every row of y0 (M,D), vel the mean
        policy of pullback_chain at y with the x of the step before as its guess (x0 (M,D): guesses for the starts).  `inner`: the K
        stages as pullback_chain's, 0 <= K <= CHAIN_MAX; this handle is the last stage's, or — K = 0, the model `dyn` rolls out
        itself — dyn.  `outputs`: which of "vel" and "x" (M,n_steps,D) come back besides path (M,n_steps+1,D), steps_done and status
        (M,).  A trajectory ends at the first step that does not converge or leaves the finite numbers; every row after its end is
        NaN.  Returns a dict."""
        return self._rollout_host("rollout_policy", ROLLOUT_OUTPUTS, ("vel", "x"), (), inner, dyn, y0, n_steps, dt, x0, rtol, max_passes, outputs)

    def rollout_policy_dev(self, inner, dyn, y0_ptr, M, n_steps, path_ptr, steps_done_ptr, status_ptr, dt=1.0, x0_ptr=0, rtol=1e-10,
                           max_passes=64, vel_ptr=0, x_ptr=0):
        """The same on device pointers (float64; steps_done / status int32), asynchronous on this handle's stream
        (gpt_rollout_policy_dev).  `inner`: tuples (handle, R_ptr, c_src_ptr, c_dst_ptr, scale, R_jac_ptr), device pointers."""
        self._rollout_dev("rollout_policy", ROLLOUT_OUTPUTS, (), inner, dyn, y0_ptr, x0_ptr, M, n_steps, dt, rtol, max_passes,
                          dict(path=path_ptr, vel=vel_ptr, x=x_ptr, steps_done=steps_done_ptr, status=status_ptr))

    # ---- whole paths of the variance-stabilised policy
    def rollout_stabilised(self, inner, dyn, y0, n_steps, gain, std_offset=0.0, dt=1.0, x0=None, rtol=1e-10, max_passes=64,
                           outputs=("vel", "x", "f", "var", "dvar")):
        """gpt_rollout_stabilised on host arrays: rollout_policy with the reference's variance stabiliser inside every step,
        vel = push(f - gain * (sqrt(var) - std_offset) * dvar / |dvar|), var and dvar the posterior variance of `dyn` and its
        gradient at the source-space preimage x of the step's point.  Arguments as rollout_policy's; `outputs`: which of "vel",
        "x", "f", "dvar" (M,n_steps,D) and "var" (M,n_steps) come back besides path, steps_done and status.  gain = 0 gives
        rollout_policy's path, vel, x, steps_done and status bit for bit.  `dyn`: at most ROLLOUT_STAB_MAX_N training points, a
        kernel with derivatives.  Returns a dict."""
        return self._rollout_host("rollout_stabilised", ROLLOUT_STAB_OUTPUTS, ("vel", "x", "f", "var", "dvar"), (float(gain), float(std_offset)),
                                  inner, dyn, y0, n_steps, dt, x0, rtol, max_passes, outputs)

    def rollout_stabilised_dev(self, inner, dyn, y0_ptr, M, n_steps, gain, path_ptr, steps_done_ptr, status_ptr, std_offset=0.0, dt=1.0,
                               x0_ptr=0, rtol=1e-10, max_passes=64, vel_ptr=0, x_ptr=0, f_ptr=0, var_ptr=0, dvar_ptr=0):
        """The same on device pointers (float64; steps_done / status int32), asynchronous on this handle's stream
        (gpt_rollout_stabilised_dev).  `inner`: tuples (handle, R_ptr, c_src_ptr, c_dst_ptr, scale, R_jac_ptr), device pointers."""
        self._rollout_dev("rollout_stabilised", ROLLOUT_STAB_OUTPUTS, (float(gain), float(std_offset)), inner, dyn, y0_ptr, x0_ptr, M, n_steps,
                          dt, rtol, max_passes, dict(path=path_ptr, vel=vel_ptr, x=x_ptr, f=f_ptr, var=var_ptr, dvar=dvar_ptr,
                                                     steps_done=steps_done_ptr, status=status_ptr))

    # ---- whole paths of functions drawn from the dynamics posterior
    def rollout_sampled(self, inner, dyn, y0, normals, n_steps, nugget, dt=1.0, x0=None, rtol=1e-10, max_passes=64,
                        outputs=("vel", "x", "f", "pvar", "cvar")):
        """gpt_rollout_sampled on host arrays: rollout_policy with, in place of the mean of `dyn`, one function drawn from its
        posterior per path, the draw of a step conditioned on the path's own earlier draws (only `dyn` is sampled; the maps of
        `inner` act through their means).  y0 (P,D): one start per path; normals (P,n_steps,D): the caller's standard normal
        numbers, the only randomness; nugget >= 0: added to the diagonal of a path's covariance (the noise level of `dyn`: noisy
        values, predict(return_cov=True)'s convention).  `outputs`: which of "vel", "x", "f" (P,n_steps,D), "pvar", "cvar"
        (P,n_steps: the marginal and the conditional variance of a step's draw) and "chol" (P,n_steps,n_steps: the lower Cholesky
        factor of the path's covariance) come back besides path, steps_done and status; status takes the INV_* values and
        ROLLOUT_DEGENERATE (ROLLOUT_SAMPLED_STATUS_NAMES).  Zero normals give rollout_policy's path.  `dyn`: at most
        ROLLOUT_STAB_MAX_N training points, any kernel; n_steps at most ROLLOUT_SAMPLED_MAX_T.  Returns a dict."""
        y0 = as_f64(y0, 2, "y0")
        T = int(n_steps)
        if T > ROLLOUT_SAMPLED_MAX_T:
            raise ValueError(f"rollout_sampled: n_steps must be at most {ROLLOUT_SAMPLED_MAX_T} (ROLLOUT_SAMPLED_MAX_T), got {T}")
        if not np.isfinite(float(nugget)) or float(nugget) < 0.0:
            raise ValueError(f"rollout_sampled: nugget must be finite and >= 0, got {nugget!r}")
        normals = as_f64(normals, 3, "normals")
        if normals.shape != (y0.shape[0], max(T, 0), y0.shape[1]):
            raise ValueError(f"normals has shape {normals.shape}, expected (paths, n_steps, D) = {(y0.shape[0], T, y0.shape[1])}")
        return self._rollout_host("rollout_sampled", ROLLOUT_SAMPLED_OUTPUTS, ("vel", "x", "f", "pvar", "cvar", "chol"), (float(nugget),),
                                  inner, dyn, y0, T, dt, x0, rtol, max_passes, outputs, inputs=(normals,))

    def rollout_sampled_dev(self, inner, dyn, y0_ptr, normals_ptr, M, n_steps, nugget, path_ptr, steps_done_ptr, status_ptr, dt=1.0,
                            x0_ptr=0, rtol=1e-10, max_passes=64, vel_ptr=0, x_ptr=0, f_ptr=0, pvar_ptr=0, cvar_ptr=0, chol_ptr=0):
        """The same on device pointers (float64; steps_done / status int32), asynchronous on this handle's stream
        (gpt_rollout_sampled_dev).  `inner`: tuples (handle, R_ptr, c_src_ptr, c_dst_ptr, scale, R_jac_ptr), device pointers."""
        self._rollout_dev("rollout_sampled", ROLLOUT_SAMPLED_OUTPUTS, (float(nugget),), inner, dyn, y0_ptr, x0_ptr, M, n_steps, dt, rtol,
                          max_passes, dict(path=path_ptr, vel=vel_ptr, x=x_ptr, f=f_ptr, pvar=pvar_ptr, cvar=cvar_ptr, chol=chol_ptr,
                                           steps_done=steps_done_ptr, status=status_ptr), input_ptrs=(normals_ptr,))

    # ---- whole paths of whole functions drawn from the dynamics posterior (pathwise conditioning)
    def rollout_pathwise(self, inner, dyn, y0, func, weights, omega, amp, n_steps, dt=1.0, x0=None, rtol=1e-10, max_passes=64,
                         outputs=("vel", "x", "f")):
        """gpt_rollout_pathwise on host arrays: rollout_policy with, in place of the mean of `dyn`, the drawn function
        F_s(x) = k(x, X) weights[s] + sum_j amp[s, j, 0] cos(omega[j] . x) + amp[s, j, 1] sin(omega[j] . x), s = func[p] for path p
        (only `dyn` is sampled; the maps of `inner` act through their means).  y0 (P,D): one start per path; func (P,) ints in
        0 .. S - 1; weights (S,N,D); omega (J,D), J <= PATHWISE_MAX_FREQ (J = 0: the kernel part alone); amp (S,J,2,D).
        `outputs`: which of "vel", "x", "f" (P,n_steps,D; f = F_s at x) come back besides path, steps_done and status.  With J = 0
        and weights = alpha: rollout_policy's path.  Any kernel, any N, any n_steps.  Returns a dict."""
        N, D, O, _ = dyn.info()
        y0 = as_f64(y0, 2, "y0")
        func = np.ascontiguousarray(func, dtype=np.int32)
        if func.shape != (y0.shape[0],):
            raise ValueError(f"func has shape {func.shape}, expected (paths,) = {(y0.shape[0],)}")
        weights = as_f64(weights, 3, "weights")
        S = weights.shape[0]
        if S < 1 or weights.shape != (S, N, D):
            raise ValueError(f"weights has shape {weights.shape}, expected (functions >= 1, N, D) = (S, {N}, {D})")
        omega = as_f64(omega, 2, "omega")
        J = omega.shape[0]
        amp = as_f64(amp, 4, "amp")
        if omega.shape != (J, D) or amp.shape != (S, J, 2, D):
            raise ValueError(f"omega has shape {omega.shape} and amp {amp.shape}, expected (J, {D}) and ({S}, J, 2, {D})")
        if J > PATHWISE_MAX_FREQ:
            raise ValueError(f"rollout_pathwise: at most {PATHWISE_MAX_FREQ} (PATHWISE_MAX_FREQ) frequencies, got {J}")
        if func.size and (func.min() < 0 or func.max() >= S):
            raise ValueError(f"rollout_pathwise: func must hold indices 0 .. {S - 1}")
        return self._rollout_host("rollout_pathwise", ROLLOUT_PATHWISE_OUTPUTS, ("vel", "x", "f"),
                                  (S, dptr(weights), J, dptr(omega) if J else None, dptr(amp) if J else None), inner, dyn, y0, n_steps, dt,
                                  x0, rtol, max_passes, outputs, inputs=(func,))

    def rollout_pathwise_dev(self, inner, dyn, y0_ptr, func_ptr, M, n_steps, S, weights4_ptr, J, omega_ptr, amp_ptr, path_ptr, steps_done_ptr,
                             status_ptr, dt=1.0, x0_ptr=0, rtol=1e-10, max_passes=64, vel_ptr=0, x_ptr=0, f_ptr=0):
        """The same on device pointers (float64; func / steps_done / status int32), asynchronous on this handle's stream
        (gpt_rollout_pathwise_dev).  weights4_ptr: (S,NP,4), one image per function in the layout of the model's alpha rows.
        `inner`: tuples (handle, R_ptr, c_src_ptr, c_dst_ptr, scale, R_jac_ptr), device pointers."""
        self._rollout_dev("rollout_pathwise", ROLLOUT_PATHWISE_OUTPUTS, (int(S), _vp(weights4_ptr or None), int(J), _vp(omega_ptr or None),
                                                                         _vp(amp_ptr or None)), inner, dyn, y0_ptr, x0_ptr, M, n_steps, dt,
                          rtol, max_passes, dict(path=path_ptr, vel=vel_ptr, x=x_ptr, f=f_ptr, steps_done=steps_done_ptr, status=status_ptr),
                          input_ptrs=(func_ptr,))

    # ---- predict (device pointers, asynchronous)
    def predict_all_dev(self, xq_ptr, M, mean_ptr=0, var_ptr=0, J_ptr=0, Jvar_ptr=0, dvar_ptr=0):
        check(self.lib.gpt_predict_all_dev(self._h, _vp(xq_ptr), int(M), _vp(mean_ptr or None), _vp(var_ptr or None),
                                           _vp(J_ptr or None), _vp(Jvar_ptr or None), _vp(dvar_ptr or None)),
              "gpt_predict_all_dev")

    def reserve(self, M, jacobian_variance=False):
        """Allocate the scratch of a predict_all_dev call with M queries ahead of time."""
        check(self.lib.gpt_reserve(self._h, int(M), int(bool(jacobian_variance))), "gpt_reserve")

    def set_profiling(self, enable=True):
        check(self.lib.gpt_set_profiling(self._h, int(bool(enable))), "gpt_set_profiling")

    def predict_timings(self):
        t = np.zeros(2)
        check(self.lib.gpt_predict_timings(self._h, dptr(t)), "gpt_predict_timings")
        return {"mean_jac_ms": float(t[0]), "var_ms": float(t[1])}

    def var_path(self):
        """Kernel of the last variance launch: 0 fp64, 1 residue (int8), -1 none yet."""
        return int(self.lib.gpt_debug_var_path(self._h))

    def set_stream(self, stream_ptr):
        check(self.lib.gpt_set_stream(self._h, _vp(stream_ptr or None)), "gpt_set_stream")

    def synchronize(self):
        check(self.lib.gpt_synchronize(self._h), "gpt_synchronize")

    # ---- multi-GPU hand-off
    def factor_blob(self):
        p, n = _vp(), C.c_size_t()
        check(self.lib.gpt_factor_blob(self._h, C.byref(p), C.byref(n)), "gpt_factor_blob")
        return p.value, n.value

    def factor_alloc(self, N, D, O, n_tasks=1, dtype=GPT_F64):
        p, n = _vp(), C.c_size_t()
        check(self.lib.gpt_factor_alloc_model(self._h, int(N), int(D), int(O), int(n_tasks), int(dtype), C.byref(p),
                                              C.byref(n)), "gpt_factor_alloc_model")
        return p.value, n.value

    def factor_commit(self):
        check(self.lib.gpt_factor_commit(self._h), "gpt_factor_commit")

    def factor_copy_from(self, src: "Handle"):
        """This handle becomes a replica of `src`'s fitted model (same process, any device): gpt_factor_copy."""
        check(self.lib.gpt_factor_copy(self._h, src._h), "gpt_factor_copy")
