"""ctypes binding of libndq.so (C-ABI: include/ndq.h).  The product path has no CPU or torch fallback for these
entry points: if the library is missing or a launch fails, it raises."""
import ctypes
import os

from . import _build

NDQ_ACT_TANH, NDQ_ACT_SIN, NDQ_ACT_SIGMOID, NDQ_ACT_SWISH, NDQ_ACT_APTX = 0, 1, 2, 3, 4
NDQ_ACT_ELU, NDQ_ACT_SOFTPLUS, NDQ_ACT_GELU = 5, 6, 7


class MlpDesc(ctypes.Structure):
    _fields_ = [("d", ctypes.c_int), ("first", ctypes.c_int), ("mask2", ctypes.c_int), ("hidden", ctypes.c_int),
                ("layers", ctypes.c_int), ("act", ctypes.c_int), ("n_out", ctypes.c_int), ("lap", ctypes.c_int),
                ("skip", ctypes.c_int), ("mask3", ctypes.c_int), ("actp", ctypes.c_int), ("widths", ctypes.c_int), ("mono", ctypes.c_int),
                ("mask4", ctypes.c_int)]

    def key(self):
        return (self.d, self.first, self.mask2, self.hidden, self.layers, self.act, self.n_out, self.lap, self.skip,
                self.mask3, self.actp, self.widths, self.mono, self.mask4)


NDQ_SAMPLE_UNIFORM, NDQ_SAMPLE_GRID, NDQ_SAMPLE_SPHERICAL = 0, 1, 2


class SamplerDesc(ctypes.Structure):
    """ndq_sampler_desc of include/ndq.h"""
    _fields_ = [("kind", ctypes.c_int), ("d", ctypes.c_int), ("n", ctypes.c_int * 3), ("lo", ctypes.c_float * 3),
                ("hi", ctypes.c_float * 3), ("noise_std", ctypes.c_float * 3), ("radial", ctypes.c_int)]


NDQ_TABLE_MAX_AXES = 6
NDQ_AXIS_NORMAL, NDQ_AXIS_CHEB2_NOISY = 0, 1


class TableSamplerDesc(ctypes.Structure):
    """ndq_table_sampler_desc of include/ndq.h"""
    _fields_ = [("d", ctypes.c_int), ("n", ctypes.c_int * 6), ("law", ctypes.c_int * 6), ("abs_value", ctypes.c_int),
                ("mean", ctypes.c_void_p * 6), ("std", ctypes.c_void_p * 6), ("lo", ctypes.c_float * 6),
                ("hi", ctypes.c_float * 6)]


NDQ_PLAN_MAX_LEAVES = 8
NDQ_LEAF_SIMPLE, NDQ_LEAF_TABLE, NDQ_LEAF_DATA = 0, 1, 2
NDQ_SEG_LEAF, NDQ_SEG_ENSEMBLE, NDQ_SEG_MESH = 0, 1, 2
NDQ_INDEX_NONE, NDQ_INDEX_PERMUTE, NDQ_INDEX_REPLACE = 0, 1, 2


class _PlanLaw(ctypes.Union):
    _fields_ = [("simple", SamplerDesc), ("table", TableSamplerDesc), ("data", ctypes.c_void_p * 6)]


class PlanLeaf(ctypes.Structure):
    """ndq_plan_leaf of include/ndq.h"""
    _fields_ = [("kind", ctypes.c_int), ("row0", ctypes.c_int), ("rows", ctypes.c_int), ("n", ctypes.c_int), ("u", _PlanLaw)]


class PlanSegment(ctypes.Structure):
    """ndq_plan_segment of include/ndq.h"""
    _fields_ = [("mode", ctypes.c_int), ("first", ctypes.c_int), ("count", ctypes.c_int), ("offset", ctypes.c_int),
                ("size", ctypes.c_int)]


class PlanSamplerDesc(ctypes.Structure):
    """ndq_plan_sampler_desc of include/ndq.h"""
    _fields_ = [("d", ctypes.c_int), ("n_leaves", ctypes.c_int), ("n_segments", ctypes.c_int), ("reserved", ctypes.c_int),
                ("leaf", PlanLeaf * 8), ("seg", PlanSegment * 8)]


class PlanIndexDesc(ctypes.Structure):
    """ndq_plan_index_desc of include/ndq.h"""
    _fields_ = [("mode", ctypes.c_int), ("m", ctypes.c_int), ("batch", ctypes.c_int), ("reserved", ctypes.c_int)]


FUSED_LAUNCH_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                   ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
                                   ctypes.c_float, ctypes.c_int, ctypes.c_void_p)


class FusedStep(ctypes.Structure):
    """ndq_fused_step of include/ndq.h"""
    _fields_ = [("launch", ctypes.c_void_p),
                ("n", ctypes.c_int), ("ldc", ctypes.c_int), ("ldj", ctypes.c_int), ("blocks", ctypes.c_int),
                ("n_params", ctypes.c_int), ("seed", ctypes.c_float),
                ("params", ctypes.c_void_p), ("partials", ctypes.c_void_p), ("loss_partials", ctypes.c_void_p),
                ("grad", ctypes.c_void_p), ("loss_slot", ctypes.c_void_p), ("adam_m", ctypes.c_void_p),
                ("adam_v", ctypes.c_void_p),
                ("lr", ctypes.c_float), ("beta1", ctypes.c_float), ("beta2", ctypes.c_float), ("eps", ctypes.c_float),
                ("weight_decay", ctypes.c_float),
                ("loss_hist", ctypes.c_void_p), ("best_loss", ctypes.c_void_p), ("best_flat", ctypes.c_void_p),
                ("allreduce", ctypes.c_void_p), ("comm", ctypes.c_void_p),
                ("next_sampler", ctypes.c_void_p), ("next_seed", ctypes.c_ulonglong), ("next_draw", ctypes.c_ulonglong),
                ("next_stream", ctypes.c_uint), ("next_coords", ctypes.c_void_p), ("next_ldc", ctypes.c_int)]


NDQ_THETA_MAX = 32


class ThetaStep(ctypes.Structure):
    """ndq_theta_step of include/ndq.h"""
    _fields_ = [("n_theta", ctypes.c_int), ("frozen", ctypes.c_uint),
                ("theta", ctypes.c_void_p), ("partials", ctypes.c_void_p), ("gtheta", ctypes.c_void_p),
                ("adam_m", ctypes.c_void_p), ("adam_v", ctypes.c_void_p),
                ("lr", ctypes.c_float * 32), ("beta1", ctypes.c_float * 32), ("beta2", ctypes.c_float * 32),
                ("eps", ctypes.c_float * 32), ("weight_decay", ctypes.c_float * 32), ("step", ctypes.c_int * 32)]


class FusedStep64(ctypes.Structure):
    """ndq64_fused_step of include/ndq.h"""
    _fields_ = [("n", ctypes.c_int), ("ldc", ctypes.c_int), ("ldj", ctypes.c_int), ("blocks", ctypes.c_int),
                ("n_params", ctypes.c_int), ("seed", ctypes.c_double),
                ("params", ctypes.c_void_p), ("partials", ctypes.c_void_p), ("loss_partials", ctypes.c_void_p),
                ("grad", ctypes.c_void_p), ("loss_slot", ctypes.c_void_p), ("adam_m", ctypes.c_void_p),
                ("adam_v", ctypes.c_void_p),
                ("lr", ctypes.c_double), ("beta1", ctypes.c_double), ("beta2", ctypes.c_double), ("eps", ctypes.c_double),
                ("weight_decay", ctypes.c_double),
                ("loss_hist", ctypes.c_void_p), ("best_loss", ctypes.c_void_p), ("best_flat", ctypes.c_void_p)]


class FusedFit(ctypes.Structure):
    """ndq_fused_fit of include/ndq.h"""
    _fields_ = [("launch", ctypes.c_void_p), ("n_nets", ctypes.c_int), ("net", FusedStep * 4),
                ("valid_coords", ctypes.c_void_p), ("valid_n", ctypes.c_int), ("valid_ldc", ctypes.c_int),
                ("valid_blocks", ctypes.c_int), ("valid_scale", ctypes.c_float),
                ("valid_loss_partials", ctypes.c_void_p), ("valid_hist", ctypes.c_void_p), ("track_best", ctypes.c_int),
                ("pull_ok", ctypes.c_int), ("alt_params", ctypes.c_void_p * 4), ("alt_m", ctypes.c_void_p * 4),
                ("alt_v", ctypes.c_void_p * 4), ("alt_partials", ctypes.c_void_p * 4),
                ("alt_loss_partials", ctypes.c_void_p), ("alt_valid_loss_partials", ctypes.c_void_p),
                ("launch_loop", ctypes.c_void_p), ("loop_ok", ctypes.c_int)]


class NdqError(RuntimeError):
    pass


REAL = object()         # placeholder in SHARED_ARGTYPES: c_float in libndq.so, c_double in libndq64.so
_vp, _ci, _dp = ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(MlpDesc)
#: the entry points both libraries have (ndq_<suffix> / ndq64_<suffix>, csrc/ndq_api_common.h and the two sums): suffix -> argtypes
SHARED_ARGTYPES = {
    "mlp_supported": [_dp],
    "mlp_num_streams": [_dp],
    "mlp_num_params": [_dp],
    "mlp_bwd_blocks": [_dp, _ci],
    "mlp_jet_fwd": [_dp, _vp, _ci, _ci, _vp, _vp, _ci, _vp],
    "mlp_jet_bwd": [_dp, _vp, _ci, _ci, _vp, _vp, _ci, _vp, _vp],
    "mlp_register": [_vp],
    "reduce_partials": [_vp, _ci, _ci, _vp, _ci, REAL, _vp],
    "adam_step": [_vp, _vp, _vp, _vp, _ci, REAL, REAL, REAL, REAL, REAL, _ci, _vp],
    "epoch_tail": [_vp, _vp, _vp, _vp, _ci, REAL, REAL, REAL, REAL, REAL, _ci, _vp, _ci, _vp, _ci, _vp, _ci, _vp, _ci, _vp],
}


def _bind(L, prefix, real, own, exports):
    """argtypes of the shared entry points (REAL -> ``real``) and of the library's ``own`` ones; every export returns int."""
    for suffix, args in SHARED_ARGTYPES.items():
        getattr(L, prefix + suffix).argtypes = [real if a is REAL else a for a in args]
    for name, args in own.items():
        getattr(L, name).argtypes = args
    for name in exports:
        getattr(L, name).restype = _ci
    return L


_LIB = None


def lib():
    """Load libndq.so (building it first if hipcc is available and the sources are newer)."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = _build.LIB
    if _build.is_stale():
        try:
            _build.build_lib()
        except Exception as e:  # no hipcc / compile error
            if not os.path.exists(path):
                raise NdqError(f"libndq.so is missing and could not be built: {e}") from e
    vp, ci, cf, u64 = _vp, _ci, ctypes.c_float, ctypes.c_ulonglong
    _LIB = _bind(ctypes.CDLL(path), "ndq_", cf, {
        "ndq_reduce_grad_loss": [vp, ci, ci, vp, ci, vp, ci, vp, cf, vp],
        "ndq_fused_step_run": [ctypes.POINTER(FusedStep), vp, ci, ci, ci, vp],
        "ndq_fused_multi_step_run": [ctypes.POINTER(FusedStep), ci, vp, vp, ci, ci, ci, vp],
        "ndq_fused_fit_run": [ctypes.POINTER(FusedFit), ci, vp, ci, ci, ci, ci, vp],
        "ndq_theta_step_bytes": [],
        "ndq_theta_step_consts": [ctypes.POINTER(ThetaStep), ci, ctypes.POINTER(cf)],
        "ndq_fused_theta_step_run": [ctypes.POINTER(FusedStep), ctypes.POINTER(ThetaStep), vp, ci, ci, ci, vp],
        "ndq_fused_theta_multi_step_run": [ctypes.POINTER(FusedStep), ci, vp, ctypes.POINTER(ThetaStep), vp, ci, ci, ci, vp],
        "ndq_sample": [ctypes.POINTER(SamplerDesc), u64, u64, ctypes.c_uint, vp, ci, vp],
        "ndq_sample_table": [ctypes.POINTER(TableSamplerDesc), u64, u64, ctypes.c_uint, vp, ci, vp],
        "ndq_sample_plan": [ctypes.POINTER(PlanSamplerDesc), u64, u64, ctypes.c_uint, vp, ci, vp],
        "ndq_sample_plan_indexed": [ctypes.POINTER(PlanSamplerDesc), ctypes.POINTER(PlanIndexDesc), u64, u64, ctypes.c_uint, vp, ci,
                                    vp],
        "ndq_oneshot_create": [ci, ci, ci, ctypes.POINTER(vp), ctypes.c_char_p],
        "ndq_oneshot_connect": [vp, ctypes.c_char_p],
        "ndq_oneshot_allreduce": [vp, vp, ctypes.c_size_t, ci, ci, vp, vp],
        "ndq_oneshot_status": [vp],
        "ndq_oneshot_destroy": [vp],
    }, EXPORTS)
    return _LIB


_LIB64 = None


def lib64():
    """Load libndq64.so (the fp64 build of the stream kernels: ndq64_* of include/ndq.h), building it first if needed."""
    global _LIB64
    if _LIB64 is not None:
        return _LIB64
    if _build.is_stale64():
        try:
            _build.build_lib64()
        except Exception as e:  # no hipcc / compile error
            if not os.path.exists(_build.LIB64):
                raise NdqError(f"libndq64.so is missing and could not be built: {e}") from e
    vp, ci = _vp, _ci
    _LIB64 = _bind(ctypes.CDLL(_build.LIB64), "ndq64_", ctypes.c_double, {
        "ndq64_fused_step_bytes": [],
        "ndq64_reduce_tail": [ctypes.POINTER(FusedStep64), ci, ci, ci, ci, vp],
        "ndq64_fused_step_run": [ctypes.POINTER(FusedStep64), ci, vp, vp, ci, ci, ci, vp],
    }, EXPORTS64)
    return _LIB64


EXPORTS64 = ("ndq64_mlp_register", "ndq64_mlp_supported", "ndq64_mlp_num_streams", "ndq64_mlp_num_params",
             "ndq64_mlp_bwd_blocks", "ndq64_mlp_jet_fwd", "ndq64_mlp_jet_bwd", "ndq64_reduce_partials", "ndq64_adam_step",
             "ndq64_epoch_tail", "ndq64_fused_step_bytes", "ndq64_reduce_tail", "ndq64_fused_step_run")

EXPORTS = ("ndq_mlp_supported", "ndq_mlp_num_streams", "ndq_mlp_num_params", "ndq_mlp_bwd_blocks", "ndq_mlp_jet_fwd",
           "ndq_mlp_jet_bwd", "ndq_reduce_partials", "ndq_adam_step", "ndq_reduce_grad_loss", "ndq_epoch_tail",
           "ndq_fused_step_run", "ndq_sample", "ndq_sample_table", "ndq_sample_plan", "ndq_sample_plan_indexed", "ndq_mlp_register",
           "ndq_fused_multi_step_run", "ndq_fused_fit_run", "ndq_oneshot_create", "ndq_oneshot_connect", "ndq_oneshot_allreduce", "ndq_oneshot_status",
           "ndq_oneshot_destroy", "ndq_theta_step_bytes", "ndq_theta_step_consts", "ndq_fused_theta_step_run",
           "ndq_fused_theta_multi_step_run")


def check(rc, what):
    if rc != 0:
        raise NdqError(f"{what} failed with code {rc}" + (" (no kernel for this descriptor)" if rc == -1 else ""))
