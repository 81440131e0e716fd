#!/usr/bin/env python
"""The gfx950 device code of generated modules, kernel by kernel, as JSON: what ``lib_isa_digests.py`` does for the two C-ABI
libraries, for the JIT side.  Run it on two checkouts and compare -- a change to the kernel headers that is meant to leave the
kernels alone shows as an empty difference (no GPU needed).

For each system below, traced with the checkout's own engine, it builds into a scratch directory (never ``_jit``):
  closure        the single-launch closure module (``codegen.fused_build_plan`` + ``_hipcc.compile_shared``)
  closure_8wave  its 8-wave build, where ``closure_source_digests.py`` would record one
  closure_f64    the fp64 closure, where there is one
and one ``codegen.mlp_ext_source`` module each for a wide (csrc/ndq_wide.h) and a deep (csrc/ndq_deep.h) shape.  Systems: the five
BASELINE configs, one system for every fp32 closure mode and fp64 closure kind, and C2 once more with -DNDQ_EPILOGUE_RS=0.  The
JSON is keyed by system label and build, not by the cache key (which hashes the headers).  What is recorded per kernel symbol:
``_isa_digest.py``.  It only hashes and tabulates.
usage: scripts/closure_isa_digests.py TREE OUT.json"""
import sys, os, json, tempfile, types
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _isa_digest

if __name__ == "__main__":
    tree, out = _isa_digest.use_tree(sys.argv[1]), sys.argv[2]
    for name in ("NDQ_JIT_FLAGS", "NDQ_F64_CLOSURE", "NDQ_GROUP_WIDE"):
        os.environ.pop(name, None)
    import torch
    from neurodiffeq_amd import codegen, engine, _hipcc, _lib
    from tests import configs, site_problems, wide_site_problems, wide_multi_problems

    def config(name):
        cfg = configs.make(name, 8 if name.startswith("c") else None)
        return cfg["nets"], cfg["conds"], configs.fused_equations(cfg), configs.n_coords(cfg), configs.func_val(cfg)

    # label -> (system, extra compile flags); the comment names the closure mode (fp32 / fp64) the system is here for
    SYSTEMS = {
        "cfg/c1": (lambda: config("c1"), []),                          # multi / multi
        "cfg/c2": (lambda: config("c2"), []),                          # tile / tile, 8-wave build
        "cfg/c3": (lambda: config("c3"), []),                          # tile (H = 64)
        "cfg/c4": (lambda: config("c4"), []),                          # group
        "cfg/c5": (lambda: config("c5"), []),                          # no closure: its kernels are the deep module below
        "cfg/w6": (lambda: config("w6"), []),                          # sites
        "cfg/w16": (lambda: config("w16"), []),                        # wide
        "wide_multi/lv-80": (lambda: wide_multi_problems.make("lv", 80) + (None,), []),                                  # wide_multi
        "wide_sites/" + wide_site_problems.NAMES[0]: (lambda: wide_site_problems.make(wide_site_problems.NAMES[0]) + (None,), []),
        "sites/" + site_problems.NAMES[0]: (lambda: site_problems.make(site_problems.NAMES[0]) + (None,), []),
        "cfg/c2 -DNDQ_EPILOGUE_RS=0": (lambda: config("c2"), ["-DNDQ_EPILOGUE_RS=0"]),
    }
    EXT = {"wide": "w16", "deep": "w18"}          # stream-kernel extension modules: one hidden layer / several, wider than 64 units

    def trace(make, f64):
        torch.manual_seed(0)
        nets, conds, eqs, nc, cfv = make()
        for net in nets:
            net.double() if f64 else net.float()
        return engine.trace_system(nets, conds, eqs, nc, compute_func_val=cfv, f64=f64)

    def plans(make, more):
        """build name -> (source, flags) of the modules the system is served by"""
        res = {}
        program, descs = trace(make, False)
        if codegen.fuse_mode(program, descs):
            res["closure"] = codegen.fused_build_plan(program, descs[0], more_flags=more)[:2]
            me = types.SimpleNamespace(program=program, descs=descs, L=_lib.lib())
            if engine.FusedSystem._wide_possible(me):
                res["closure_8wave"] = codegen.fused_build_plan(program, descs[0], threads=512, more_flags=more)[:2]
        try:
            program, descs = trace(make, True)
        except Exception:      # noqa: BLE001 -- no fp64 trace of this system: no fp64 closure
            return res
        if codegen.can_fuse_f64(program, descs) or codegen.can_fuse_multi_f64(program, descs):
            res["closure_f64"] = codegen.fused_build_plan(program, descs[0], f64=True, more_flags=more)[:2]
        return res

    todo = {(label, build): plan for label, (make, more) in SYSTEMS.items() for build, plan in plans(make, more).items()}
    for kind, name in EXT.items():
        desc = trace(lambda: config(name), False)[1][0]
        assert codegen.is_wide(desc) and (desc.layers >= 2) == (kind == "deep"), (kind, name)
        todo[(f"cfg/{name}", f"mlp_ext_{kind}")] = (codegen.mlp_ext_source(desc), codegen.WIDE_FLAGS if kind == "wide" else [])
    res = {label: {} for label in SYSTEMS}
    with tempfile.TemporaryDirectory() as work:
        libs = {}
        with _hipcc.deferred():
            for i, (key, (source, flags)) in enumerate(todo.items()):
                src, libs[key] = os.path.join(work, f"m{i}.hip"), os.path.join(work, f"m{i}.so")
                with open(src, "w") as fh:
                    fh.write(source)
                _hipcc.compile_shared(src, libs[key], flags, defer=True)
        for (label, build), lib in libs.items():
            sub = os.path.join(work, "co")
            os.makedirs(sub, exist_ok=True)
            res.setdefault(label, {})[build] = _isa_digest.digest_lib(lib, sub)
            print(label, build, len(res[label][build]), "kernels", flush=True)
    with open(out, "w") as fh:
        json.dump(res, fh, indent=1, sort_keys=True)
