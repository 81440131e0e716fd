"""Compile-time switches that were folded into the side that won stop the build (csrc/ndq_mlp.h, the #error block under the
table of surviving switches): a stale NDQ_JIT_FLAGS / NDQ_LIB_FLAGS would otherwise compile the same kernels twice under two
cache keys and time noise.  Preprocessor only: no kernel is compiled, no GPU needed."""
import os
import subprocess

import pytest

from neurodiffeq_amd import _hipcc

#: retired switch -> header a translation unit reaches it through (the deep-network switches lived in ndq_deep.h / ndq_launch.h)
RETIRED = {name: "ndq_mlp.h" for name in (
    "NDQ_FAST_TANH", "NDQ_BF16X3", "NDQ_WIDE_LOWREG", "NDQ_PIN_WEIGHT_READS", "NDQ_KEEP_H", "NDQ_REUSE_FWD", "NDQ_WIDE_LAUNDER",
    "NDQ_WG32", "NDQ_WG_SCHED_BARRIER", "NDQ_QUAD_SWAP", "NDQ_STAGE_INFLIGHT", "NDQ_GROUP_PREFETCH", "NDQ_WG_BF16",
    "NDQ_SPLIT_PAIRS", "NDQ_STAGGER", "NDQ_BF16_NPROD")}
RETIRED.update({name: "ndq_launch.h" for name in (
    "NDQ_DEEP_XCD_REMAP", "NDQ_DEEP_HEAD_FUSED", "NDQ_DEEP_HEAD_FWD_FUSED", "NDQ_DEEP_WGRAD_BF", "NDQ_DEEP_BF16X3")})


def preprocess(tmp_path, header, flags=()):
    src = tmp_path / f"unit_{header[:-2]}.hip"
    src.write_text(f'#include "{header}"\nint unit;\n')
    return subprocess.run([_hipcc.HIPCC, f"--offload-arch={_hipcc.ARCH}", "--cuda-device-only", "-E"] + _hipcc.BASE_FLAGS + list(flags)
                          + [str(src), "-o", os.devnull], capture_output=True, text=True)


@pytest.mark.parametrize("header", sorted(set(RETIRED.values())))
def test_unit_without_retired_flags_preprocesses(tmp_path, header):
    proc = preprocess(tmp_path, header)
    assert proc.returncode == 0, proc.stderr[-2000:]


@pytest.mark.parametrize("name", sorted(RETIRED))
def test_retired_switch_stops_the_build(tmp_path, name):
    for value in ("0", "1"):
        proc = preprocess(tmp_path, RETIRED[name], [f"-D{name}={value}"])
        assert proc.returncode != 0, f"-D{name}={value} still compiles"
        errors = [line for line in proc.stderr.splitlines() if "error:" in line]
        assert errors and all("retired" in line for line in errors) and any(name in line for line in errors), proc.stderr[-2000:]
