"""The fp64 sums + tail launch (csrc/ndq_api64.hip: reduce_tail64_kernel behind ndq64_reduce_tail / ndq64_fused_step_run)
without a GPU: the ctypes mirror of its argument struct, the exported names, the argument checks that run before any HIP
call -- csrc/ndq_api_common.h, so the fp32 runner ndq_fused_multi_step_run is held to the same list -- and the switch that
routes a solver epoch to it."""
import ctypes
import os
import re

import pytest

from neurodiffeq_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ndq64_fused_step_bytes", "ndq64_reduce_tail", "ndq64_fused_step_run")
NDQ_EINVAL = -2


def test_struct_mirror_has_the_librarys_size():
    assert ctypes.sizeof(_lib.FusedStep64) == _lib.lib64().ndq64_fused_step_bytes()


def test_new_names_are_exported_and_declared():
    header = open(os.path.join(ROOT, "include", "ndq.h")).read()
    declared = set(re.findall(r"^\s*int\s+(ndq64_\w+)\s*\(", header, flags=re.M))
    L = _lib.lib64()
    for name in NEW:
        assert name in _lib.EXPORTS64 and name in declared
        assert getattr(L, name) is not None


FP32_ENTRY = "ndq_fused_multi_step_run"        # the same runner and rule set in float (csrc/ndq_api_common.h)


def _steps(entry):
    """Structs that pass every check: the pointers are never followed (each case below fails validation first).  Returns the
    array and the buffer the pointers aim at."""
    real, step = (ctypes.c_float, _lib.FusedStep) if entry == FP32_ENTRY else (ctypes.c_double, _lib.FusedStep64)
    buf = (real * 64)()
    p = ctypes.addressof(buf)
    arr = (step * 4)()
    for k in range(4):
        st = arr[k]
        st.n, st.ldc, st.ldj, st.blocks, st.n_params = 16, 64, 64, 1, 8
        st.seed = 1.0
        for f in ("params", "partials", "loss_partials", "grad", "loss_slot", "adam_m", "adam_v", "loss_hist", "best_loss"):
            setattr(st, f, p)
        st.lr, st.beta1, st.beta2, st.eps, st.weight_decay = 1e-3, 0.9, 0.999, 1e-8, 0.0
    return arr, buf


def _never(*_):        # pragma: no cover
    raise AssertionError("the launcher must not run: validation comes first")


_CB = ctypes.CFUNCTYPE(ctypes.c_int)(_never)
_CB_PTR = ctypes.cast(_CB, ctypes.c_void_p)


def _call(entry, arr, n_nets=1, adam_step=1, hist_index=0, parity=0, coords=True, launch=_CB_PTR):
    if entry == "ndq64_reduce_tail":
        return _lib.lib64().ndq64_reduce_tail(arr, n_nets, adam_step, hist_index, parity, None)
    buf = ((ctypes.c_float if entry == FP32_ENTRY else ctypes.c_double) * 8)()
    run = _lib.lib().ndq_fused_multi_step_run if entry == FP32_ENTRY else _lib.lib64().ndq64_fused_step_run
    return run(arr, n_nets, launch, ctypes.c_void_p(ctypes.addressof(buf)) if coords else None, adam_step, hist_index, parity, None)


@pytest.mark.parametrize("entry", ["ndq64_reduce_tail", "ndq64_fused_step_run", FP32_ENTRY])
def test_bad_arguments_are_refused_before_any_hip_call(entry):
    arr, keep = _steps(entry)
    assert _call(entry, None) == NDQ_EINVAL                                   # null steps
    for n_nets in (0, 5):
        assert _call(entry, arr, n_nets=n_nets) == NDQ_EINVAL
    assert _call(entry, arr, adam_step=0) == NDQ_EINVAL
    assert _call(entry, arr, hist_index=-1) == NDQ_EINVAL
    assert _call(entry, arr, parity=2) == NDQ_EINVAL
    for field in ("params", "grad", "adam_m", "loss_partials", "loss_slot"):
        arr, keep = _steps(entry)
        setattr(arr[0], field, None)
        assert _call(entry, arr) == NDQ_EINVAL, field
    for field in ("blocks", "n_params"):      # (sizes the fp32 entry did not check before it shared the fp64 rules)
        arr, keep = _steps(entry)
        setattr(arr[0], field, 0)
        assert _call(entry, arr) == NDQ_EINVAL, field
    # ... and of a later network of the system
    for field in ("params", "grad", "adam_m"):
        arr, keep = _steps(entry)
        setattr(arr[1], field, None)
        assert _call(entry, arr, n_nets=2) == NDQ_EINVAL, field
    if entry != "ndq64_reduce_tail":
        arr, keep = _steps(entry)
        assert _call(entry, arr, coords=False) == NDQ_EINVAL
        assert _call(entry, arr, launch=None) == NDQ_EINVAL


def test_switch_is_opt_in():
    from neurodiffeq_amd.engine import f64_fused_tail_switch
    assert f64_fused_tail_switch({}) is False
    assert f64_fused_tail_switch({"NDQ_F64_FUSED_TAIL": "1"}) is True
    assert f64_fused_tail_switch({"NDQ_F64_FUSED_TAIL": "0"}) is False
