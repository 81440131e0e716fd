"""The multi-network closure kernel compiled in double, without a GPU: which fp64 systems codegen.can_fuse_multi_f64 admits,
what the generated source says, what the cross-compiled module answers when loaded (loading and asking touches no GPU), and
that nothing about the fp32 modules moved."""
import ctypes
import hashlib
import os
import re
import subprocess
import warnings

import pytest
import torch

from neurodiffeq_amd import _hipcc, _lib, codegen, diff, engine
from neurodiffeq_amd.conditions import IVP
from neurodiffeq_amd.networks import FCNN
from tests import configs
from tests import f64_multi_problems as FP
from tests import site_problems as SP
from tests import wide_multi_problems as WM
from tests.test_wide_multi import EXPORTS, _exports, _load

SWITCHES = ("NDQ_NO_MULTI_FUSE", "NDQ_F64_CLOSURE", "NDQ_FUSE_GROUP", "NDQ_NO_GROUP_FUSE", "NDQ_NO_LAP", "NDQ_NO_SITE_FUSE",
            "NDQ_NO_WIDE_MULTI_FUSE")
LDS_LIMIT = 160 * 1024
#: SHA-1 of the fp32 closure / pointwise sources of c1 and w8 as the commit before the fp64 multi-network closure generated
#: them (scripts/closure_source_digests.py on that commit)
FP32_DIGESTS = {"c1": ("multi", "fd5dcaa67c3921e6e9f005d021535787f2eae0b6", "1381cb98fa4fbbe7cea259dd0ba89c48ef21ea31"),
                "w8": ("sites", "4f01a024cec99c97bc91869d25ebb1462b40d7f1", "652da74aa0d5b5c89cb25ae857edae99c0bc925c")}


@pytest.fixture(autouse=True)
def _no_switches(monkeypatch):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)


def traced(name):
    torch.manual_seed(0)
    nets, conds, eqs, d, cfv = FP.make(name)
    return engine.trace_system(nets, conds, eqs, d, compute_func_val=cfv, f64=True)


def traced_config(name, f64):
    torch.manual_seed(0)
    cfg = configs.make(name, 8 if name.startswith("c") else None)
    if f64:
        for net in cfg["nets"]:
            net.double()
    return engine.trace_system(cfg["nets"], cfg["conds"], configs.fused_equations(cfg), configs.n_coords(cfg),
                               compute_func_val=configs.func_val(cfg), f64=f64)


@pytest.mark.parametrize("name,nets", [("c1", 2), ("lv_tanh", 2), ("mix32", 2), ("uvp16", 3)])
def test_fp64_systems_of_narrow_networks_take_the_multi_closure(name, nets):
    program, descs = traced(name)
    assert program.n_nets == program.n_sites == nets
    assert codegen.can_fuse_multi_f64(program, descs)
    assert not codegen.can_fuse_f64(program, descs)              # (keeps its meaning: the one-network closure)
    src = program.fused_source(descs[0], f64=True)
    assert src.startswith("#define NDQ_F64 1\n")
    assert not re.search(r"\bfloat\b", src)
    assert f"ndq::fused_multi_closure_kernel<CFG, {nets}, PW, true>" in src
    assert f"ndq::fused_multi_closure_tv_kernel<CFG, {nets}, PW>" in src
    assert "fused_multi_closure_loop_kernel" not in src and "static constexpr auto loop = nullptr;" in src
    so = codegen.build_fused(program, descs[0], f64=True)
    assert _exports(so) == EXPORTS
    lib = _load(so)
    assert lib.ndq_fused_num_nets() == nets and lib.ndq_fused_threads() == 64 * nets * (2 if nets == 2 else 1)
    assert lib.ndq_fused_num_params() == _lib.lib64().ndq64_mlp_num_params(ctypes.byref(descs[0]))
    assert lib.ndq_fused_lds_bytes() <= LDS_LIMIT
    assert lib.ndq_fused_pull_ok() == 0 and lib.ndq_fused_loop_ok() == 0
    assert lib.ndq_fused_blocks(1) == 1 and lib.ndq_fused_blocks(1 << 20) == 256


def test_w8_has_neumann_ends_and_stays_on_the_pipeline_in_double():
    """tests/configs.py ``w8`` -- two tanh 32 x 32 networks -- is DoubleEndedBVP1D with a Neumann end on either network: four
    evaluation sites of two networks.  Evaluation sites are outside the fp64 closures, so in double it keeps the pipeline;
    ``lv_tanh`` above is the two-network tanh 32 x 32 system the fp64 closure is run on."""
    program, descs = traced_config("w8", True)
    assert program.site_net == [0, 1, 0, 1]
    assert not codegen.can_fuse_multi_f64(program, descs) and not codegen.can_fuse_f64(program, descs)


def _host_lds_report(K, cfg_t, tmp_path):
    """A stand-alone host program (its own main) that evaluates the LDS-size constexprs of csrc/ndq_mlp.h in double for K
    networks of ``cfg_t`` and checks them against their parts; returns what it prints."""
    src = tmp_path / f"lds64_{K}.hip"
    src.write_text(f"""#define NDQ_F64 1
#define NDQ_WG_TR_K {K}
#include <cstdio>
#include "ndq_mlp.h"
using CFG = {cfg_t};
constexpr int K = {K};
constexpr size_t T = ndq::fused_multi_lds_bytes<CFG, K>(true), E = ndq::fused_multi_lds_bytes<CFG, K>(false);
static_assert(sizeof(ndq::real) == 8, "double build");
static_assert(!CFG::BF16 && !CFG::WG_TR && CFG::BWD_THREADS == 256, "no bf16 planes in double; one wave per SIMD");
static_assert(!ndq::pull_supported<CFG>(), "no pull mode in double");
static_assert(CFG::ldsWeightsEnd(true) % 4 == 0 && ndq::multi_group_floats<CFG, K>() % 4 == 0, "regions stay 32-byte aligned");
static_assert(T == 8 * ((size_t)K * CFG::ldsWeightsEnd(true) + (size_t)K * ndq::multi_group_floats<CFG, K>() +
                        ndq::multi_xchg_floats<CFG, K>() + 16), "training launch: images + staging / reduction + exchange");
constexpr size_t EP = (size_t)K * CFG::ldsWeightsEnd(false) + ndq::multi_xchg_floats<CFG, K>() + 16;
constexpr size_t EQ = (size_t)K * CFG::ldsWeightsEnd(false) + (size_t)K * ndq::pull_floats<CFG>() + 16;   // (sized for fp32's pull prologue too)
static_assert(E == 8 * (EP > EQ ? EP : EQ), "forward-only launch");
static_assert(ndq::multi_group_floats<CFG, K>() >= ndq::multi_regions<CFG, K>() * ((CFG::P + 3) & ~3), "reduction regions fit");
static_assert(ndq::multi_group_floats<CFG, K>() >= ndq::multi_group<K>() * CFG::stageFloatsPerWave, "staging tiles fit");
int main() {{
  std::printf("%zu %zu %d %d %d\\n", T, E, ndq::multi_threads<K>(), ndq::multi_group<K>(), CFG::P);
  return 0;
}}
""")
    exe = tmp_path / f"lds64_{K}"
    subprocess.run([_hipcc.HIPCC, "--offload-arch=gfx950", *_hipcc.BASE_FLAGS, str(src), "-o", str(exe)], check=True,
                   capture_output=True, text=True)
    return [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]


@pytest.mark.parametrize("name", ["c1", "uvp16", "four32"])
def test_lds_constexprs_in_double_from_a_stand_alone_host_program(name, tmp_path):
    program, descs = traced(name)
    K = program.n_nets
    train, ev, threads, group, n_params = _host_lds_report(K, codegen.mlp_cfg(descs[0], 1), tmp_path)
    lib = _load(codegen.build_fused(program, descs[0], f64=True))
    assert lib.ndq_fused_lds_bytes() == train > ev
    assert lib.ndq_fused_threads() == threads == 64 * K * group and lib.ndq_fused_num_params() == n_params
    if name == "c1":
        assert group == 2 and train == 110784          # two tile slots per workgroup fit in double


def test_four_networks_at_32x32_the_engine_gate_follows_the_lds_formula(tmp_path):
    """K = 4 at 32 x 32: the predicate admits it, the module is built, and what the engine's gate reads -- the module's
    ``ndq_fused_lds_bytes()`` against 160 KiB -- is the LDS formula of csrc/ndq_mlp.h evaluated by the host program.  (On the GPU
    tests/test_gpu_f64_multi_closure.py holds ``FusedSystem.fusedk`` to the same figure.)"""
    import inspect
    program, descs = traced("four32")
    assert program.n_nets == 4 and codegen.can_fuse_multi_f64(program, descs)
    lib = _load(codegen.build_fused(program, descs[0], f64=True))
    assert lib.ndq_fused_num_nets() == 4
    train = _host_lds_report(4, codegen.mlp_cfg(descs[0], 1), tmp_path)[0]
    assert lib.ndq_fused_lds_bytes() == train
    assert "if fk.lib.ndq_fused_lds_bytes() <= 160 * 1024:" in inspect.getsource(engine.FusedSystem.__init__)


def test_systems_outside_the_family_are_turned_down():
    no = lambda program, descs: not codegen.can_fuse_multi_f64(program, descs)
    # evaluation sites (Neumann ends)
    assert no(*traced_config("w6", True)) and no(*traced_config("w8", True))
    program, descs = SP.trace("heat-nd")
    assert program.n_sites > program.n_nets and no(program, descs)
    # one network; one network on the grouped kernel (several outputs)
    assert no(*traced_config("c2", True)) and no(*traced_config("c4", True))
    # wide one-layer networks
    torch.manual_seed(0)
    nets, conds, eqs, d = WM.make("lv", 80)
    assert no(*engine.trace_system([n.double() for n in nets], conds, eqs, d, f64=True))
    # one two-output network shared by two conditions
    lv = lambda u, v, t: [diff(u, t) - (u - u * v), diff(v, t) - (u * v - v)]
    shared = FCNN(1, 2, hidden_units=(32, 32)).double()
    sconds = [IVP(0.0, 1.5), IVP(0.0, 1.0)]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        sconds[0].set_impose_on(0)
        sconds[1].set_impose_on(1)
    assert no(*engine.trace_system([shared, shared], sconds, lv, 1, f64=True))
    # mixed shapes
    mixed = [FCNN(1, 1, hidden_units=(32, 32)).double(), FCNN(1, 1, hidden_units=(16, 16)).double()]
    assert no(*engine.trace_system(mixed, [IVP(0.0, 1.5), IVP(0.0, 1.0)], lv, 1, f64=True))
    # H = 64
    big = [FCNN(1, 1, hidden_units=(64, 64)).double() for _ in range(2)]
    assert no(*engine.trace_system(big, [IVP(0.0, 1.5), IVP(0.0, 1.0)], lv, 1, f64=True))
    # third- / fourth-order stream sets: a descriptor that carries one is turned down by the predicate itself
    program, descs = traced("c1")
    d0 = descs[0]
    for m3, m4 in ((1, 0), (0, 1)):
        odd = {k: _lib.MlpDesc(d0.d, d0.first, d0.mask2, d0.hidden, d0.layers, d0.act, 1, d0.lap, 0, m3, 0, 0, 0, m4) for k in range(2)}
        assert codegen.fuse_mode(program, odd) == "multi" and no(program, odd)
    # ... as is a two-output one
    two = {k: _lib.MlpDesc(d0.d, d0.first, d0.mask2, d0.hidden, d0.layers, d0.act, 2, d0.lap, 0, 0, 0, 0, 0) for k in range(2)}
    assert no(program, two)


def test_grouped_mode_and_both_off_switches(monkeypatch):
    program, descs = traced("c1")
    assert codegen.can_fuse_multi_f64(program, descs)
    # NDQ_NO_MULTI_FUSE: no multi mode, in either precision
    monkeypatch.setenv("NDQ_NO_MULTI_FUSE", "1")
    assert not codegen.can_fuse_multi_f64(program, descs) and codegen.fuse_mode(program, descs) is None
    program, descs = traced("c1")
    assert not codegen.can_fuse_multi_f64(program, descs)
    monkeypatch.delenv("NDQ_NO_MULTI_FUSE")
    # NDQ_FUSE_GROUP=1 sends one-network systems to the grouped kernel: not a multi system either way
    monkeypatch.setenv("NDQ_FUSE_GROUP", "1")
    assert not codegen.can_fuse_multi_f64(*traced_config("c2", True))
    monkeypatch.delenv("NDQ_FUSE_GROUP")
    # NDQ_F64_CLOSURE=0 is the engine's switch: every fp64 system on the three-kernel pipeline, fp32 systems untouched
    program, descs = traced("c1")
    one = traced_config("c2", True)
    assert engine.wants_closure(program, descs, True) and engine.wants_closure(*one, True)
    monkeypatch.setenv("NDQ_F64_CLOSURE", "0")
    assert not engine.wants_closure(program, descs, True) and not engine.wants_closure(*one, True)
    assert engine.wants_closure(*traced_config("c1", False), False)
    monkeypatch.delenv("NDQ_F64_CLOSURE")
    monkeypatch.setenv("NDQ_NO_MULTI_FUSE", "1")
    assert not engine.wants_closure(*traced("c1"), True) and engine.wants_closure(*one, True)


@pytest.mark.parametrize("name", ["c1", "w8"])
def test_fp32_sources_are_what_they_were(name):
    program, descs = traced_config(name, False)
    mode, closure, pointwise = FP32_DIGESTS[name]
    assert codegen.fuse_mode(program, descs) == mode
    assert hashlib.sha1(program.fused_source(descs[0]).encode()).hexdigest() == closure
    assert hashlib.sha1(program.source.encode()).hexdigest() == pointwise
