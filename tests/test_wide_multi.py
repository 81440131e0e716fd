"""The "wide_multi" closure mode without a GPU: which systems codegen.fuse_mode sends to wide_multi_closure_kernel
(csrc/ndq_wide.h: 2 .. 4 networks of ONE WideCfg behind one launch), and what the generated module exports and answers
when it is cross-compiled for gfx950 and loaded (loading and asking touches no GPU)."""
import ctypes
import os
import struct
from functools import partial

import pytest
import torch

from neurodiffeq_amd import _lib, codegen, diff, engine
from neurodiffeq_amd.conditions import IVP
from neurodiffeq_amd.networks import FCNN, Swish
from neurodiffeq_amd.symbolic import TraceUnsupported
from tests import wide_multi_problems as WM

#: the thirteen names every generated closure module exports (csrc/ndq_closure_host.h), restated
EXPORTS = sorted("ndq_fused_" + n for n in (
    "blocks", "num_params", "num_theta", "bind_theta", "num_nets", "threads", "lds_bytes", "launch", "launch_multi", "launch_tv",
    "pull_ok", "launch_loop", "loop_ok"))
#: the switches that decide the mode: every test starts from "none set"
SWITCHES = ("NDQ_NO_WIDE_MULTI_FUSE", "NDQ_WIDE_MULTI_FUSE")


@pytest.fixture(autouse=True)
def _no_switches(monkeypatch):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)


def traced(nets, conds, eqs, n_coords):
    return engine.trace_system(nets, conds, eqs, n_coords)


def system(name, width, act=None):
    torch.manual_seed(0)
    return traced(*WM.make(name, width, act))


#: the cases of the GPU matrix beyond lv / uvp / four: third-order streams, mixed second derivatives on sigmoid / swish / GELU
#: networks, trainable scalars in the equations, and the system that does not fit one workgroup's LDS
NEW_CASES = [c for c in WM.GPU_CASES if c[0] in ("ode3", "mix", "mix4", "lvtheta")]


def _exports(so):
    """ndq_fused_* symbols DEFINED by a shared library: its ELF dynamic symbol table, read directly."""
    with open(so, "rb") as fh:
        elf = fh.read()
    shoff, = struct.unpack_from("<Q", elf, 0x28)
    shentsize, shnum = struct.unpack_from("<HH", elf, 0x3A)
    sections = [struct.unpack_from("<IIQQQQIIQQ", elf, shoff + i * shentsize) for i in range(shnum)]
    names = set()
    for _, kind, _, _, offset, size, link, _, _, entsize in sections:
        if kind != 11:                                    # SHT_DYNSYM
            continue
        strtab = sections[link][4]
        for at in range(offset, offset + size, entsize):
            st_name, _, _, st_shndx = struct.unpack_from("<IBBH", elf, at)
            name = elf[strtab + st_name:elf.index(b"\0", strtab + st_name)].decode()
            if st_shndx != 0 and name.startswith("ndq_fused_"):
                names.add(name)
    return sorted(names)


def _load(so):
    lib = ctypes.CDLL(so)
    lib.ndq_fused_lds_bytes.restype = ctypes.c_ulong
    lib.ndq_fused_blocks.argtypes = [ctypes.c_int]
    return lib


@pytest.mark.parametrize("name,width,nets", [("lv", 80, 2), ("uvp", 128, 3), ("four", 72, 4)])
def test_systems_of_wide_one_layer_networks_take_the_wide_multi_closure(name, width, nets):
    program, descs = system(name, width)
    assert program.n_nets == nets and len({descs[k].key() for k in range(nets)}) == 1
    if name == "uvp":
        assert descs[0].lap == 1                          # the Laplacian stream travels as one stream
    assert codegen.fuse_mode(program, descs) == "wide_multi"
    assert codegen.can_fuse(program, descs) and not codegen.can_fuse_f64(program, descs)


def test_systems_outside_the_family_stay_on_the_pipeline(monkeypatch):
    eq2, conds2 = WM.equations("lv", diff), [IVP(0.0, 1.5), IVP(0.0, 1.0)]
    torch.manual_seed(0)
    # different widths; one of the networks with two hidden layers
    for shapes in (((80,), (96,)), ((80, 80), (80,)), ((80, 80), (80, 80))):
        program, descs = traced([FCNN(1, 1, hidden_units=h) for h in shapes], conds2, eq2, 1)
        assert codegen.fuse_mode(program, descs) is None, shapes
    # five networks
    ring = lambda a, b, c, e, f, t: [diff(a, t) + b, diff(b, t) - c, diff(c, t) + e, diff(e, t) - f, diff(f, t) + a]
    program, descs = traced([FCNN(1, 1, hidden_units=(72,)) for _ in range(5)], [IVP(0.0, 1.0 + k) for k in range(5)], ring, 1)
    assert codegen.fuse_mode(program, descs) is None
    # trainable activation parameters above 64 units: no stream kernels at all, so the system never reaches the fused path ...
    with pytest.raises(TraceUnsupported):
        traced([FCNN(1, 1, hidden_units=(80,), actv=partial(Swish, trainable=True)) for _ in range(2)], conds2, eq2, 1)
    # ... and the mode function turns the descriptor down by itself
    program, descs = system("lv", 80)
    d = descs[0]
    swish = {k: _lib.MlpDesc(d.d, d.first, d.mask2, d.hidden, d.layers, 3, d.n_out, d.lap, 0, d.mask3, 1, 0, 0) for k in range(2)}
    assert codegen.fuse_mode(program, swish) is None
    # the off-switch
    assert codegen.fuse_mode(program, descs) == "wide_multi"
    monkeypatch.setenv("NDQ_NO_WIDE_MULTI_FUSE", "1")
    assert codegen.fuse_mode(program, descs) is None


@pytest.mark.parametrize("name,width,nets", [("lv", 80, 2), ("uvp", 128, 3)])
def test_wide_multi_module_exports_and_launch_geometry(name, width, nets):
    program, descs = system(name, width)
    so = codegen.build_fused(program, descs[0])
    assert _exports(so) == EXPORTS
    lib = _load(so)
    assert lib.ndq_fused_num_nets() == nets
    assert lib.ndq_fused_lds_bytes() <= 160 * 1024
    assert lib.ndq_fused_pull_ok() == 0 and lib.ndq_fused_loop_ok() == 0
    assert lib.ndq_fused_num_params() == sum(p.numel() for p in program.unique_nets[0].parameters())
    # the one-network closure of the same WideCfg: same tiles, same workgroups
    torch.manual_seed(0)
    one, odescs = traced(*WM.make_single(name, width))
    assert codegen.fuse_mode(one, odescs) == "wide" and odescs[0].key() == descs[0].key()
    wide = _load(codegen.build_fused(one, odescs[0]))
    assert wide.ndq_fused_num_nets() == 1 and wide.ndq_fused_threads() == lib.ndq_fused_threads()
    for n in (1, 15, 16, 17, 4096, 65536):
        assert lib.ndq_fused_blocks(n) == wide.ndq_fused_blocks(n), n


def wide_multi_lds_bytes(d, width, n_streams, nets, n_out=1, n_theta=0, waves=4):
    """csrc/ndq_wide.h's WideMulti layout restated: K unit images, then per wave the reduction rows of ONE network and K output
    + K seed slices -- or the block reduction rows, if those are larger."""
    ul = 64 if width > 256 else (32 if width > 128 else 16)
    u, pl = -(-width // ul), 64 // ul
    nc = n_streams * n_out
    ncp = (nc + 3) & ~3
    nx = max(n_streams - 1 - d, 1)
    rs, rp = ul + 4, 16
    while rp > pl and rp * nc * rs * 4 > 20 * 1024 * 4 // waves:
        rp >>= 1
    img = u * (d + 1 + nx + n_out + (n_streams if n_out == 1 else 0)) * ul
    wave = (rp * nc * rs + 2 * nets * 16 * ncp + 3) & ~3
    p = width * d + width + n_out * width + n_out
    red = ((p + 16 + 3) & ~3) + 32 + waves * max(n_theta, 1)
    return 4 * (nets * img + max(waves * wave, red))


@pytest.mark.parametrize("name,width,nets,d,ns", [("lv", 80, 2, 1, 2), ("uvp", 128, 3, 2, 4), ("four", 72, 4, 1, 2), ("four", 512, 4, 1, 2)])
def test_module_size_is_what_the_layout_says_and_decides_whether_the_engine_keeps_it(name, width, nets, d, ns):
    """engine.FusedSystem keeps a closure module only if ndq_fused_lds_bytes() fits one workgroup's 160 KiB; the answer comes
    from the module, for every K -- at K = 4, W = 512 too, whichever way it falls."""
    program, descs = system(name, width)
    assert codegen.fuse_mode(program, descs) == "wide_multi"
    lib = _load(codegen.build_fused(program, descs[0]))
    want = wide_multi_lds_bytes(d, width, ns, nets)
    assert lib.ndq_fused_lds_bytes() == want
    assert lib.ndq_fused_num_nets() == nets
    fits = lib.ndq_fused_lds_bytes() <= 160 * 1024
    assert fits == (want <= 160 * 1024)
    if (name, width) == ("four", 512):
        assert fits, "four 512-unit networks of one input: 12 KiB of unit image each, 91 KiB in all"


@pytest.mark.parametrize("case", NEW_CASES, ids=WM.case_id)
def test_new_systems_take_the_wide_multi_closure_with_one_descriptor(case):
    """Third-order streams, mixed second derivatives, sigmoid / swish / GELU, trainable scalars: all inside the family, every
    network of a system on ONE descriptor (stream set unified over the networks)."""
    name, K, d_in = case[0], WM.SYSTEMS[case[0]][1], WM.SYSTEMS[case[0]][2]
    program, descs = system(*case)
    assert program.n_nets == K and len({descs[k].key() for k in range(K)}) == 1
    assert codegen.fuse_mode(program, descs) == "wide_multi" and codegen.can_fuse(program, descs)
    d = descs[0]
    want = {"ode3": (1, 1, 1, 0), "mix": (1, 7, 0, 0), "mix4": (1, 7, 0, 0), "lvtheta": (1, 0, 0, 0)}[name]
    assert (d.first, d.mask2, d.mask3, d.lap) == want and d.d == d_in and d.hidden == case[1] and d.layers == 1
    assert d.act == {"tanh": 0, "sin": 1, "sigmoid": 2, "swish": 3, "gelu": 7}[WM.activation(case)]
    assert _lib.lib().ndq_mlp_num_streams(ctypes.byref(d)) == WM.n_streams(name)
    assert len(program.g.params) == (2 if name == "lvtheta" else 0) and not program.g.frozen


def test_layout_restatement_at_the_sizes_worked_out_by_hand():
    assert wide_multi_lds_bytes(2, 512, 4, 3) == 131072          # uvp 512
    assert wide_multi_lds_bytes(2, 512, 4, 4) == 151552          # a uvp-shaped system of four: still inside
    assert wide_multi_lds_bytes(2, 200, 6, 2) == 86784           # mix 200
    assert wide_multi_lds_bytes(2, 512, 6, 4) == 175104          # mix4 512: outside
    assert 151552 <= 160 * 1024 < 175104


@pytest.mark.parametrize("case", [c for c in WM.GPU_CASES if c[:2] not in (("lv", 80), ("uvp", 128), ("four", 72), ("four", 512))],
                         ids=WM.case_id)
def test_module_size_of_every_gpu_case_and_which_ones_the_engine_keeps(case):
    """ndq_fused_lds_bytes() of every module the GPU matrix launches is what the layout says -- trainable scalars (their block
    sums behind the reduction rows) included --, and exactly the case listed as over the budget exceeds 160 KiB."""
    name, width = case[:2]
    K, d_in = WM.SYSTEMS[name][1:3]
    program, descs = system(*case)
    lib = _load(codegen.build_fused(program, descs[0]))
    n_theta = len(program.g.params)
    assert n_theta == (2 if name == "lvtheta" else 0) and lib.ndq_fused_num_theta() == n_theta
    want = wide_multi_lds_bytes(d_in, width, WM.n_streams(name), K, n_theta=n_theta)
    assert lib.ndq_fused_lds_bytes() == want and lib.ndq_fused_num_nets() == K
    assert (want > 160 * 1024) == (case in WM.OVER_LDS)
    assert lib.ndq_fused_threads() == 256 and lib.ndq_fused_blocks(16384) == 256 and lib.ndq_fused_blocks(16400) == 256
    assert lib.ndq_fused_blocks(16368) == 256 and lib.ndq_fused_blocks(16320) == 255       # ceil(ceil(n / 16) / 4), at most 256


def test_goldens_are_reproduced_by_the_fp64_oracle(golden_dir):
    """wm1 / wm2 (tests/golden/make_wide_multi_golden.py, from the unmodified reference) against the autograd oracle's
    restatement of the same systems in fp64, on the CPU: loss, gradient, function values and residuals of the recorded batch."""
    import numpy as np
    from oracle import autograd_ref as R
    for gname, (name, width) in WM.GOLDEN.items():
        gold = np.load(os.path.join(golden_dir, f"{gname}.npz"))
        nets, enf, eqs = WM.make_oracle(name, width)
        R.set_flat(nets, torch.from_numpy(gold["params0"]).double())
        out = R.closure(nets, enf, eqs, [torch.from_numpy(c).double() for c in gold["coords"]])
        grad = R.get_flat_grad(nets).numpy()
        rel = lambda a, b: float(np.linalg.norm(np.asarray(a, np.float64) - b) / np.linalg.norm(b))
        assert gold["coords"].shape[1] == 256
        assert abs(out["loss"].item() - float(gold["loss_f64"])) < 1e-12 * abs(float(gold["loss_f64"]))
        assert rel(grad, gold["grad_f64"]) < 1e-12
        assert rel(out["funcs"].numpy(), gold["funcs_f64"]) < 1e-12 and rel(out["residuals"].numpy(), gold["residuals_f64"]) < 1e-12
