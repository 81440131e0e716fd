"""The "sites" closure mode without a GPU: which systems codegen.fuse_mode sends to the multi-network closure kernel with site
traits (csrc/ndq_mlp.h: 2 .. 4 evaluation sites of fewer networks behind one launch -- conditions with Neumann ends), what the
traits of the generated module say, and what the module exports and answers when it is cross-compiled for gfx950 and loaded
(loading and asking touches no GPU)."""
import warnings

import pytest
import torch

from neurodiffeq_amd import _lib, codegen, diff, engine
from neurodiffeq_amd.conditions import IBVP1D, DoubleEndedBVP1D
from neurodiffeq_amd.networks import FCNN
from tests import configs
from tests import site_problems as SP
from tests import wide_multi_problems as WM
from tests.test_wide_multi import EXPORTS, _exports, _load

SWITCHES = ("NDQ_NO_SITE_FUSE", "NDQ_NO_MULTI_FUSE", "NDQ_FUSE_GROUP", "NDQ_NO_GROUP_FUSE", "NDQ_NO_LAP")


@pytest.fixture(autouse=True)
def _no_switches(monkeypatch):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)


@pytest.mark.parametrize("name", SP.NAMES)
def test_systems_with_neumann_ends_take_the_site_closure(name):
    program, descs = SP.trace(name)
    sites = SP.CASES[name][1]
    assert program.site_net == sites and program.n_nets == SP.n_nets(name) < program.n_sites == len(sites)
    assert len({descs[k].key() for k in range(len(sites))}) == 1
    assert program.n_theta == (1 if name == "heat-theta" else 0)
    assert codegen.fuse_mode(program, descs) == "sites"
    assert codegen.can_fuse(program, descs) and not codegen.can_fuse_f64(program, descs)


@pytest.mark.parametrize("name", ["w6", "w7", "w8"])
def test_reference_pinned_neumann_configs_take_the_site_closure(name):
    torch.manual_seed(0)
    cfg = configs.make(name, None)
    program, descs = engine.trace_system(cfg["nets"], cfg["conds"], configs.fused_equations(cfg), configs.n_coords(cfg),
                                         compute_func_val=configs.func_val(cfg))
    assert program.site_net == {"w6": [0, 0, 0], "w7": [0, 0], "w8": [0, 1, 0, 1]}[name]
    assert codegen.fuse_mode(program, descs) == "sites"


def _heat(hidden=(32, 32), n_out=1, third=False):
    left, right = (lambda t: 1.0 + t), (lambda t: t * t)
    eq = (lambda u, x, t: [diff(u, t) - diff(u, x, order=3)]) if third else (lambda u, x, t: [diff(u, t) - diff(u, x, order=2)])
    cond = IBVP1D(SP.X0, SP.X1, SP.T0, lambda x: torch.cos(x), x_min_prime=left, x_max_val=right)
    torch.manual_seed(0)
    return engine.trace_system([FCNN(2, n_out, hidden_units=hidden)], [cond], eq, 2)


def test_systems_outside_the_family_stay_on_the_pipeline(monkeypatch):
    # five sites: one network with two Neumann ends, one with one
    torch.manual_seed(0)
    nets = [FCNN(1, 1, hidden_units=(32, 32)) for _ in range(2)]
    conds = [DoubleEndedBVP1D(SP.X0, SP.X1, x_min_prime=0.5, x_max_prime=-0.5), DoubleEndedBVP1D(SP.X0, SP.X1, x_min_prime=0.5, x_max_val=1.0)]
    program, descs = engine.trace_system(nets, conds, SP.equations("pair-0101", diff), 1)
    assert program.site_net == [0, 1, 0, 0, 1] and codegen.fuse_mode(program, descs) is None
    # H = 64
    program, descs = _heat(hidden=(64, 64))
    assert program.site_net == [0, 0] and codegen.fuse_mode(program, descs) is None
    # a third-order stream at the interior site
    program, descs = _heat(third=True)
    assert program.site_net == [0, 0] and program.streams[0].mask3 and codegen.fuse_mode(program, descs) is None
    # a site on a two-output network: one FCNN(1, 2) shared by two conditions, one of them with a Neumann end
    shared = FCNN(1, 2, hidden_units=(32, 32))
    sconds = [DoubleEndedBVP1D(SP.X0, SP.X1, x_min_prime=0.5, x_max_val=1.0), DoubleEndedBVP1D(SP.X0, SP.X1, x_min_val=0.5, x_max_val=1.0)]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        sconds[0].set_impose_on(0)
        sconds[1].set_impose_on(1)
    program, descs = engine.trace_system([shared, shared], sconds, SP.equations("pair-010", diff), 1)
    assert program.n_sites > program.n_nets and program.streams[0].n_out == 2
    assert codegen.fuse_mode(program, descs) is None
    # ... and the mode function turns a two-output descriptor down by itself
    program, descs = SP.trace("heat-nd")
    d = descs[0]
    two = {k: _lib.MlpDesc(d.d, d.first, d.mask2, d.hidden, d.layers, d.act, 2, d.lap, 0, 0, 0, 0, 0) for k in range(2)}
    assert codegen.fuse_mode(program, two) is None
    # the off-switch: no mode, and the sites keep their own stream sets
    assert codegen.fuse_mode(program, descs) == "sites"
    monkeypatch.setenv("NDQ_NO_SITE_FUSE", "1")
    assert codegen.fuse_mode(program, descs) is None
    program, descs = SP.trace("heat-nd")
    assert codegen.fuse_mode(program, descs) is None and len({descs[k].key() for k in range(2)}) == 2


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
    src = None
    torch.manual_seed(0)
    cfg = configs.make("c1", 8)
    program, descs = engine.trace_system(cfg["nets"], cfg["conds"], configs.fused_equations(cfg), 1)
    src = program.fused_source(descs[0])
    assert "SITES" not in src and "NO_PULL" not in src and "ndq::fused_multi_closure_kernel<CFG, 2, PW, true>" in src


def test_unified_stream_set_is_the_union_of_the_sites(monkeypatch):
    for name in ("heat-nn", "pair-011", "bvp-nn"):
        monkeypatch.setenv("NDQ_NO_SITE_FUSE", "1")
        own, _ = SP.trace(name)
        monkeypatch.delenv("NDQ_NO_SITE_FUSE")
        program, descs = SP.trace(name)
        sets = [(st.first, st.mask2, st.lap) for st in own.streams.values()]
        assert len(set(sets)) > 1, name                     # (the sites do differ: a boundary site needs no second x-derivative)
        first, mask2 = max(s[0] for s in sets), 0
        for s in sets:
            mask2 |= s[1]
        assert all((st.first, st.mask2, st.lap) == (first, mask2, 0) for st in program.streams.values()), name
        assert all((descs[k].first, descs[k].mask2) == (first, mask2) for k in range(program.n_sites))


@pytest.mark.parametrize("name", ["pair-0101", "bvp-nn", "heat-nn"])
def test_traits_carry_the_site_map_and_the_boundary_values(name):
    program, descs = SP.trace(name)
    src = program.fused_source(descs[0])
    sites, lits = SP.CASES[name][1], SP.boundary_literals(name)
    S = len(sites)
    assert f"NET[k] = {{{', '.join(map(str, sites))}}}" in src
    chain = lambda vals: " : ".join([f"k == {k} ? {v}" for k, v in enumerate(vals[:-1])] + [str(vals[-1])])
    assert f"static constexpr int net(int k) {{ return {chain(sites)}; }}" in src
    assert f"static constexpr int rank(int k) {{ return {chain([sites[:k].count(sites[k]) for k in range(S)])}; }}" in src
    assert f"static constexpr unsigned vmask(int k) {{ return {chain([f'{sum(1 << d for d in lits[k])}u' for k in range(S)])}; }}" in src
    values = "".join(f"(k == {k} && d == {d}) ? {v!r}f : " for k in range(S) for d, v in sorted(lits[k].items())) + "0.0f"
    assert f"static constexpr float value(int k, int d) {{ return {values}; }}" in src
    if name == "pair-0101":
        assert "site 2 input 0 = -0.5f; site 3 input 0 = 1.5f" in src
    if name == "bvp-nn":        # one input, and it is a boundary value at both boundary sites
        assert program.n_coords == 1 and "vmask(int k) { return k == 0 ? 0u : k == 1 ? 1u : 1u; }" in src
    # the kernel is the multi-network closure on S wave groups; the host side counts parameter sets
    assert f"ndq::fused_multi_closure_kernel<CFG, {S}, PW, true, SITES>" in src and f"fused_multi_closure_tv_kernel<CFG, {S}, PW, SITES>" in src
    assert f"static constexpr int K = {SP.n_nets(name)}," in src and "static constexpr bool NO_PULL = true;" in src
    assert "static constexpr auto loop = nullptr;" in src and f"const float (&jets)[{S}][CFG::NS]" in src


def test_retrace_probe_replays_the_boundary_columns():
    """program.eq_probe (the solver's "do the callables still compute what was compiled?") runs the conditions again; a Neumann
    end asks for its boundary column again and must get the one of the compiled trace, or every probe reports a changed system
    and the solver rebuilds its FusedSystem every epoch.  A boundary that did move is still seen, and leaves nothing behind."""
    for name in ("heat-nn", "pair-0101", "bvp-nn"):
        program, _ = SP.trace(name)
        state = (dict(program.g.vcoords), list(program.g.site_net), dict(program.g.net_deps))
        assert all(program.eq_probe() for _ in range(3)), name
        assert state == (dict(program.g.vcoords), list(program.g.site_net), dict(program.g.net_deps))
    cond = DoubleEndedBVP1D(SP.X0, SP.X1, x_min_prime=0.5, x_max_val=1.0)
    torch.manual_seed(0)
    program, _ = engine.trace_system([FCNN(1, 1, hidden_units=(32, 32))], [cond], SP.equations("bvp-nn", diff), 1)
    state = (dict(program.g.vcoords), list(program.g.site_net), dict(program.g.net_deps))
    assert program.eq_probe()
    cond.x_min = -1.0
    assert not program.eq_probe()
    assert state == (dict(program.g.vcoords), list(program.g.site_net), dict(program.g.net_deps))
    cond.x_min = SP.X0
    assert program.eq_probe()


@pytest.mark.parametrize("name", ["heat-nd", "heat-nn", "heat-nn-sin40", "pair-0101", "pair-0101-h40", "heat-theta"])
def test_site_module_exports_and_launch_geometry(name):
    """The generated module cross-compiles for gfx950 (a cache hit after build()), exports the thirteen names of every closure
    module and answers: parameter sets, 64 threads per site (two tile slots for two sites), LDS inside one workgroup's 160 KiB,
    no pull / loop mode, one workgroup per tile slot group up to 256."""
    program, descs = SP.trace(name)
    S = program.n_sites
    so = codegen.build_fused(program, descs[0])
    assert _exports(so) == EXPORTS
    lib = _load(so)
    G = 2 if S == 2 else 1
    assert lib.ndq_fused_num_nets() == SP.n_nets(name) and lib.ndq_fused_threads() == 64 * S * G
    assert 0 < lib.ndq_fused_lds_bytes() <= 160 * 1024
    assert lib.ndq_fused_pull_ok() == 0 and lib.ndq_fused_loop_ok() == 0
    assert lib.ndq_fused_num_theta() == (1 if name == "heat-theta" else 0)
    for n in (1, 16, 17, 1000, 4096, 4097, 8192, 8193, 16400):
        assert lib.ndq_fused_blocks(n) == min(256, -(-(-(-n // 16)) // G)), n
    if name == "heat-nn":
        assert lib.ndq_fused_threads() == 192
