"""The "wide_sites" closure mode without a GPU: which systems codegen.fuse_mode sends to wide_multi_closure_kernel with site
traits (csrc/ndq_wide.h: 2 .. 4 evaluation sites of fewer one-hidden-layer networks of 65 .. 512 units behind one launch --
conditions with Neumann ends), what the generated module says, exports and answers when it is cross-compiled for gfx950 and
loaded (loading and asking touches no GPU)."""
import ctypes
import re

import pytest
import torch

from neurodiffeq_amd import _lib, codegen, diff, engine
from neurodiffeq_amd.conditions import IBVP1D, DoubleEndedBVP1D
from neurodiffeq_amd.networks import FCNN
from tests import configs
from tests import site_problems as SP
from tests import wide_multi_problems as WM
from tests import wide_site_problems as WS
from tests.test_wide_multi import EXPORTS, _exports, _load

SWITCHES = ("NDQ_NO_WIDE_SITE_FUSE", "NDQ_NO_SITE_FUSE", "NDQ_NO_WIDE_MULTI_FUSE", "NDQ_NO_MULTI_FUSE", "NDQ_FUSE_GROUP",
            "NDQ_NO_GROUP_FUSE", "NDQ_NO_LAP")


@pytest.fixture(autouse=True)
def _no_switches(monkeypatch):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)


def wide_site_lds_bytes(d, width, n_streams, sites, nets, n_theta=0, waves=4):
    """csrc/ndq_wide.h's WideMulti layout with sites restated: one unit image per NETWORK, then per wave the reduction rows of
    one pass and S output + S seed slices -- or the block reduction rows, if those are larger."""
    ul = 64 if width > 256 else (32 if width > 128 else 16)
    u, pl = -(-width // ul), 64 // ul
    nc = n_streams                      # one output
    ncp = (nc + 3) & ~3
    nx = max(n_streams - 1 - d, 1)
    rs, rp = ul + 4, 16
    while rp > pl and rp * nc * rs * 4 > 20 * 1024 * 4 // waves:
        rp >>= 1
    img = u * (d + 1 + nx + 1 + n_streams) * ul
    wave = (rp * nc * rs + 2 * sites * 16 * ncp + 3) & ~3
    p = width * d + width + width + 1
    red = ((p + 16 + 3) & ~3) + 32 + waves * max(n_theta, 1)
    return 4 * (nets * img + max(waves * wave, red))


def test_layout_restatement_at_the_sizes_worked_out_by_hand():
    assert wide_site_lds_bytes(1, 512, 3, 4, 2) == 4 * (2 * 3584 + 4 * 3776) == 89088            # pair-0101-512
    assert wide_site_lds_bytes(2, 128, 5, 3, 1) == 4 * (8 * 11 * 16 + 4 * (16 * 5 * 20 + 2 * 3 * 16 * 8)) == 43520      # heat-nn-128
    assert wide_site_lds_bytes(3, 512, 10, 4, 3) == 4 * (3 * 10752 + 4 * 4256) == 197120 > 160 * 1024   # the over-budget system
    # S slices, N images: one image less than the four-network module of the same shape and stream set
    from tests.test_wide_multi import wide_multi_lds_bytes
    assert wide_multi_lds_bytes(1, 512, 3, 4) - wide_site_lds_bytes(1, 512, 3, 4, 2) == 2 * 4 * 3584


@pytest.mark.parametrize("name", WS.NAMES + ["heat-nn-128"])
def test_wide_systems_with_neumann_ends_take_the_wide_site_closure(name):
    program, descs = WS.trace(name)
    sites = WS.sites(name)
    assert program.site_net == sites and program.n_nets == WS.n_nets(name) < program.n_sites == len(sites)
    assert len({descs[k].key() for k in range(len(sites))}) == 1          # after widen: ONE descriptor
    d = descs[0]
    assert (d.hidden, d.layers, d.n_out, d.mask3, d.lap) == (WS.width(name), 1, 1, 0, 0)
    assert _lib.lib().ndq_mlp_num_streams(ctypes.byref(d)) == WS.n_streams(name)
    assert program.n_theta == (1 if WS.base(name) == "heat-theta" else 0)
    assert codegen.fuse_mode(program, descs) == "wide_sites"
    assert codegen.can_fuse(program, descs) and not codegen.can_fuse_f64(program, descs)


def test_case_list_covers_every_lane_layout_and_both_sides_of_keep_all():
    """The kept-states decision is read from the modules' constants: WideMulti::KEEP_ALL = S * ROUNDS * U * 2 <= 128 with the
    generated CFG's W and the kernel's site count, both taken from the source text."""
    seen, keep = set(), {}
    for name in WS.NAMES:
        program, descs = WS.trace(name)
        src = program.fused_source(descs[0])
        w = int(re.search(r"using CFG = ndq::WideCfg<\d+, \d+, \d+u, \d+, \d+u, (\d+), \d+, \d+>;", src).group(1))
        s = int(re.search(r"ndq::wide_multi_closure_kernel<CFG, (\d+), PW, true, SITES>", src).group(1))
        ul = 64 if w > 256 else (32 if w > 128 else 16)
        u, rounds = -(-w // ul), 16 // (64 // ul)
        keep[name] = s * rounds * u * 2 <= 128
        assert keep[name] == WS.keep_all(name) and (w, s) == (WS.width(name), len(WS.sites(name)))
        seen.add((ul, w % ul != 0))
    assert {ul for ul, _ in seen} == {16, 32, 64} and all((ul, True) in seen for ul in (16, 32, 64))     # each with a ragged row
    assert any(keep.values()) and not all(keep.values())
    assert keep["heat-nd-65"] and keep["heat-dn-128"] and not keep["heat-nn-129"] and not keep["pair-0101-128"]


def _heat(hidden=(128,), n_out=1, third=False, f64=False):
    left, right = (lambda t: 1.0 + t), (lambda t: t * t)
    eq = (lambda u, x, t: [diff(u, t) - diff(u, x, order=3)]) if third else (lambda u, x, t: [diff(u, t) - diff(u, x, order=2)])
    cond = IBVP1D(SP.X0, SP.X1, SP.T0, lambda x: torch.cos(x), x_min_prime=left, x_max_val=right)
    torch.manual_seed(0)
    net = FCNN(2, n_out, hidden_units=hidden)
    return engine.trace_system([net.double() if f64 else net], [cond], eq, 2, f64=f64)


def test_systems_outside_the_family_stay_on_the_pipeline(monkeypatch):
    program, descs = _heat()
    assert program.site_net == [0, 0] and codegen.fuse_mode(program, descs) == "wide_sites"
    # two hidden layers
    program, descs = _heat(hidden=(128, 128))
    assert program.site_net == [0, 0] and codegen.fuse_mode(program, descs) is None
    # a third-order stream at the interior site
    program, descs = _heat(third=True)
    assert program.site_net == [0, 0] and program.streams[0].mask3 and codegen.fuse_mode(program, descs) is None
    # five sites: one network with two Neumann ends, one with one
    torch.manual_seed(0)
    nets = [FCNN(1, 1, hidden_units=(128,)) for _ in range(2)]
    conds = [DoubleEndedBVP1D(SP.X0, SP.X1, x_min_prime=0.5, x_max_prime=-0.5), DoubleEndedBVP1D(SP.X0, SP.X1, x_min_prime=0.5, x_max_val=1.0)]
    program, descs = engine.trace_system(nets, conds, SP.equations("pair-0101", diff), 1)
    assert program.site_net == [0, 1, 0, 0, 1] and codegen.fuse_mode(program, descs) is None
    # two outputs: the mode function turns a two-output descriptor down by itself
    program, descs = WS.trace("heat-nd-65")
    d = descs[0]
    two = {k: _lib.MlpDesc(d.d, d.first, d.mask2, d.hidden, d.layers, d.act, 2, d.lap, 0, 0, 0, 0, 0) for k in range(2)}
    assert codegen.fuse_mode(program, descs) == "wide_sites" and codegen.fuse_mode(program, two) is None
    # ... and trainable activation parameters, a skip connection, sites of different descriptors
    for bad in (dict(actp=1), dict(skip=1)):
        other = {k: _lib.MlpDesc(d.d, d.first, d.mask2, d.hidden, d.layers, d.act, 1, d.lap, bad.get("skip", 0), 0, bad.get("actp", 0), 0, 0)
                 for k in range(2)}
        assert codegen.fuse_mode(program, other) is None, bad
    mixed = {0: d, 1: _lib.MlpDesc(d.d, d.first, 1, d.hidden, d.layers, d.act, 1, d.lap, 0, 0, 0, 0, 0)}
    assert codegen.fuse_mode(program, mixed) is None
    # fp64: the sites keep their own stream sets, and nothing fuses
    program, descs = _heat(f64=True)
    assert len({descs[k].key() for k in range(2)}) == 2 and codegen.fuse_mode(program, descs) is None
    assert not codegen.can_fuse_f64(program, descs)


def test_off_switch_gives_no_mode_and_per_site_stream_sets(monkeypatch):
    program, descs = WS.trace("heat-nn-129")
    assert codegen.fuse_mode(program, descs) == "wide_sites"
    monkeypatch.setenv("NDQ_NO_WIDE_SITE_FUSE", "1")
    assert codegen.fuse_mode(program, descs) is None
    program, descs = WS.trace("heat-nn-129")
    assert codegen.fuse_mode(program, descs) is None
    assert [(st.first, st.mask2) for st in program.streams.values()] == [(1, 0b1), (1, 0b10), (1, 0b10)]
    assert len({descs[k].key() for k in range(3)}) == 2
    # the narrow mode's switch means the narrow mode only -- in both directions
    monkeypatch.delenv("NDQ_NO_WIDE_SITE_FUSE")
    monkeypatch.setenv("NDQ_NO_SITE_FUSE", "1")
    program, descs = WS.trace("heat-nn-129")
    assert codegen.fuse_mode(program, descs) == "wide_sites" and len({descs[k].key() for k in range(3)}) == 1
    monkeypatch.delenv("NDQ_NO_SITE_FUSE")
    monkeypatch.setenv("NDQ_NO_WIDE_SITE_FUSE", "1")
    program, descs = SP.trace("heat-nn")
    assert codegen.fuse_mode(program, descs) == "sites"


def test_unified_stream_set_is_the_union_of_the_sites(monkeypatch):
    for name in ("heat-nn-129", "pair-011-80", "bvp-nn-512"):
        monkeypatch.setenv("NDQ_NO_WIDE_SITE_FUSE", "1")
        own, _ = WS.trace(name)
        monkeypatch.delenv("NDQ_NO_WIDE_SITE_FUSE")
        program, descs = WS.trace(name)
        sets = [(st.first, st.mask2, st.lap) for st in own.streams.values()]
        assert len(set(sets)) > 1, name                     # (the sites do differ: a boundary site needs no second x-derivative)
        first, mask2 = max(s[0] for s in sets), 0
        for s in sets:
            mask2 |= s[1]
        assert all((st.first, st.mask2, st.lap) == (first, mask2, 0) for st in program.streams.values()), name
        assert all((descs[k].first, descs[k].mask2) == (first, mask2) for k in range(program.n_sites))


@pytest.mark.parametrize("name", ["pair-0101-128", "bvp-nn-512", "heat-nn-129", "pair-010-200"])
def test_traits_carry_the_site_map_and_the_boundary_values(name):
    program, descs = WS.trace(name)
    src = program.fused_source(descs[0])
    sites, lits = WS.sites(name), WS.boundary_literals(name)
    S, N = len(sites), WS.n_nets(name)
    assert f"NET[k] = {{{', '.join(map(str, sites))}}}" in src
    chain = lambda vals: " : ".join([f"k == {k} ? {v}" for k, v in enumerate(vals[:-1])] + [str(vals[-1])])
    assert f"static constexpr int net(int k) {{ return {chain(sites)}; }}" in src
    assert f"static constexpr unsigned vmask(int k) {{ return {chain([f'{sum(1 << d for d in lits[k])}u' for k in range(S)])}; }}" in src
    values = "".join(f"(k == {k} && d == {d}) ? {v!r}f : " for k in range(S) for d, v in sorted(lits[k].items())) + "0.0f"
    assert f"static constexpr float value(int k, int d) {{ return {values}; }}" in src
    if name == "pair-0101-128":
        assert "site 2 input 0 = -0.5f; site 3 input 0 = 1.5f" in src
    if name == "bvp-nn-512":        # one input, and it is a boundary value at both boundary sites
        assert program.n_coords == 1 and "vmask(int k) { return k == 0 ? 0u : k == 1 ? 1u : 1u; }" in src
    # N images and S slices: the kernel on S sites, its LDS on S slices and N images, the host side on N parameter sets
    assert '#include "ndq_wide.h"' in src and "static_assert(CFG::NS * CFG::NOUT ==" in src
    assert f"ndq::wide_multi_closure_kernel<CFG, {S}, PW, true, SITES>" in src
    assert f"ndq::wide_multi_closure_kernel<CFG, {S}, PW, false, SITES>" in src
    assert f"ndq::wide_multi_closure_tv_kernel<CFG, {S}, PW, SITES>" in src
    assert f"ndq::wide_multi_closure_lds_bytes<CFG, {S}, PW, {N}>()" in src
    assert f"static constexpr int K = {N}," in src and "static constexpr bool NO_PULL = true;" in src
    assert "using Args = ndq::FusedMultiArgs;" in src and "static constexpr auto loop = nullptr;" in src
    # every network input is the batch coordinate of its position; the rows are [site][stream]
    dep = " : ".join(f"d == {a} ? {a}" for a in range(program.n_coords)) + " : 0"
    assert f"static constexpr int dep(int d) {{ return {dep}; }}" in src
    assert f"grow[{S * WS.n_streams(name) - 1}] =" in src and f"grow[{S * WS.n_streams(name)}] =" not in src


@pytest.mark.parametrize("name", WS.NAMES)
def test_module_size_exports_and_launch_geometry(name):
    """The generated module cross-compiles for gfx950 (a cache hit after build()), exports the thirteen names of every closure
    module and answers: parameter sets, 256 threads, the LDS bytes of the layout -- inside one workgroup's 160 KiB --, no pull /
    loop mode, one workgroup per four tiles up to 256."""
    program, descs = WS.trace(name)
    so = codegen.build_fused(program, descs[0])
    assert _exports(so) == EXPORTS
    lib = _load(so)
    n_theta = 1 if WS.base(name) == "heat-theta" else 0
    want = wide_site_lds_bytes(WS.n_inputs(name), WS.width(name), WS.n_streams(name), len(WS.sites(name)), WS.n_nets(name), n_theta)
    assert lib.ndq_fused_lds_bytes() == want <= 160 * 1024
    assert lib.ndq_fused_num_nets() == WS.n_nets(name) and lib.ndq_fused_threads() == 256
    assert lib.ndq_fused_num_params() == sum(p.numel() for p in program.unique_nets[0].parameters())
    assert lib.ndq_fused_pull_ok() == 0 and lib.ndq_fused_loop_ok() == 0 and lib.ndq_fused_num_theta() == n_theta
    for n in (1, 16, 17, 64, 65, 1000, 4097, 16384, 16385, 16400):
        assert lib.ndq_fused_blocks(n) == min(256, -(-(-(-n // 16)) // 4)), n


def test_module_over_the_lds_budget_is_what_the_engine_drops():
    """engine.FusedSystem keeps a closure module only if ndq_fused_lds_bytes() <= 160 KiB: three 512-unit networks of three inputs
    at four sites answer 197 120 bytes -- the mode is "wide_sites", the module builds, and the engine's gate turns it down (the
    GPU test of the same system finds it on the pipeline, and right)."""
    import inspect
    torch.manual_seed(0)
    program, descs = engine.trace_system(*WS.make_over())
    assert program.site_net == WS.OVER_SITES and codegen.fuse_mode(program, descs) == "wide_sites"
    lib = _load(codegen.build_fused(program, descs[0]))
    assert lib.ndq_fused_lds_bytes() == wide_site_lds_bytes(3, WS.OVER_WIDTH, 10, 4, 3) == 197120 > 160 * 1024
    assert "if fk.lib.ndq_fused_lds_bytes() <= 160 * 1024:" in inspect.getsource(engine.FusedSystem.__init__)


def test_modes_of_the_other_systems_are_what_they_were():
    want = {"c1": "multi", "c2": "tile", "c3": "tile", "c4": "group", "c5": None}
    for name, mode in want.items():
        torch.manual_seed(0)
        cfg = configs.make(name, 8)
        program, descs = engine.trace_system(cfg["nets"], cfg["conds"], configs.fused_equations(cfg), configs.n_coords(cfg),
                                             compute_func_val=configs.func_val(cfg))
        assert codegen.fuse_mode(program, descs) == mode, name
    torch.manual_seed(0)
    program, descs = engine.trace_system(*WM.make("lv", 80))       # Lotka-Volterra on two wide networks
    assert codegen.fuse_mode(program, descs) == "wide_multi"
    src = program.fused_source(descs[0])
    assert "SITES" not in src and "NO_PULL" not in src and "ndq::wide_multi_closure_kernel<CFG, 2, PW, true>" in src
    assert "(ndq::wide_multi_closure_lds_bytes<CFG, 2, PW>())" in src
    for name in SP.NAMES:
        program, descs = SP.trace(name)
        assert codegen.fuse_mode(program, descs) == "sites", name


def test_goldens_are_reproduced_by_the_fp64_oracle(golden_dir):
    """ws1 / ws2 (tests/golden/make_wide_site_golden.py, from the unmodified reference) against the autograd oracle's restatement
    of the same systems in fp64, on the CPU: loss, gradient, function values and residuals of the recorded batch."""
    import os
    import numpy as np
    from oracle import autograd_ref as R
    for gname, case in WS.GOLDEN.items():
        gold = np.load(os.path.join(golden_dir, f"{gname}.npz"))
        nets, enf, eqs = WS.make_oracle(case)
        R.set_flat(nets, torch.from_numpy(gold["params0"]).double())
        out = R.closure(nets, enf, eqs, [torch.from_numpy(c).double() for c in gold["coords"]])
        grad = R.get_flat_grad(nets).numpy()
        rel = lambda a, b: float(np.linalg.norm(np.asarray(a, np.float64) - b) / np.linalg.norm(b))
        assert gold["coords"].shape[1] == WS.GOLDEN_POINTS
        assert abs(out["loss"].item() - float(gold["loss_f64"])) < 1e-12 * abs(float(gold["loss_f64"]))
        assert rel(grad, gold["grad_f64"]) < 1e-11
        assert rel(out["funcs"].numpy(), gold["funcs_f64"]) < 1e-12 and rel(out["residuals"].numpy(), gold["residuals_f64"]) < 1e-12
