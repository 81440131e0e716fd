#!/usr/bin/env python
"""What the closure code generator decides and emits for every system the CPU tests trace, as JSON: run it on two checkouts and
compare -- a change to the generator that is meant to leave behaviour alone shows as an empty difference (no GPU needed; stream
kernel extension modules a trace asks for are compiled on first use, as everywhere).

Systems: tests/configs.py, tests/zoo.py, tests/site_problems.py, tests/wide_site_problems.py (with its golden cases and the
over-LDS system), tests/wide_multi_problems.py (GPU, CPU, over-LDS and golden cases), tests/f64_multi_problems.py.  Per system:
  fp32      closure mode, SHA-1 of the closure and of the pointwise source, the stream set of every site after unify / widen,
            the compile flags and cache key of the closure module (plain, and the 8-wave build where the engine would try one)
  fp64      the same for the trace in double: which fp64 closure serves it ("tile" / "multi" / none) and its source digest
  switches  closure mode and source digests in fp32 with each off-switch / redirect of SWITCHES set alone
A system that cannot be built or traced is recorded with the exception's type.  "summary" counts the systems per mode.
usage: scripts/closure_source_digests.py TREE OUT.json"""
import sys, os, json, hashlib, types
tree, out = sys.argv[1], sys.argv[2]
sys.path.insert(0, tree)
import torch
from neurodiffeq_amd import codegen, engine, _lib
from tests import configs, zoo, site_problems, wide_site_problems, wide_multi_problems, f64_multi_problems

SWITCHES = ["NDQ_NO_MULTI_FUSE", "NDQ_NO_SITE_FUSE", "NDQ_NO_WIDE_SITE_FUSE", "NDQ_NO_WIDE_MULTI_FUSE", "NDQ_NO_WIDE_FUSE",
            "NDQ_NO_GROUP_FUSE", "NDQ_FUSE_GROUP", "NDQ_NO_LAP"]
sha = lambda text: hashlib.sha1(text.encode()).hexdigest()


def systems():
    """label -> callable returning (nets, conditions, equations, n_coords, compute_func_val)"""
    S = {}

    def config(name):
        cfg = configs.make(name, 8 if name.startswith("c") else None)
        return cfg["nets"], cfg["conds"], configs.fused_equations(cfg), configs.n_coords(cfg), configs.func_val(cfg)

    def from_zoo(name):
        z = zoo.build(name)
        return z.product() + (z.n_coords, None)

    for name in ["c1", "c2", "c3", "c4", "c5"] + [f"w{i}" for i in list(range(1, 22)) + list(range(24, 31))]:
        S["cfg/" + name] = lambda name=name: config(name)
    for name in zoo.NAMES:
        S["zoo/" + name] = lambda name=name: from_zoo(name)
    for name in site_problems.NAMES:
        S["sites/" + name] = lambda name=name: site_problems.make(name) + (None,)
    for name in wide_site_problems.NAMES + [c for c in wide_site_problems.GOLDEN_CASES if c not in wide_site_problems.NAMES]:
        S["wide_sites/" + name] = lambda name=name: wide_site_problems.make(name) + (None,)
    S["wide_sites/" + wide_site_problems.OVER_LDS] = lambda: wide_site_problems.make_over() + (None,)
    wm = wide_multi_problems
    for case in wm.GPU_CASES + wm.CPU_CASES + wm.OVER_LDS + list(wm.GOLDEN.values()):
        S["wide_multi/" + wm.case_id(case)] = lambda case=case: wm.make(*case) + (None,)
    for name in f64_multi_problems.NAMES:
        S["f64_multi/" + name] = lambda name=name: f64_multi_problems.make(name)
    return S


def trace(make, f64):
    torch.manual_seed(0)
    nets, conds, eqs, nc, cfv = make()
    for net in nets:
        net.double() if f64 else net.float()
    return engine.trace_system(nets, conds, eqs, nc, compute_func_val=cfv, f64=f64)


def build_plan(program, desc, **kw):
    """(source, flags, cache key) of the closure module ``codegen.build_fused`` would compile.  A checkout from before
    ``codegen.fused_build_plan`` is asked through build_fused itself, with the compiler call replaced by a recorder."""
    if hasattr(codegen, "fused_build_plan"):
        return codegen.fused_build_plan(program, desc, **kw)
    seen, real = {}, codegen._hipcc.compile_shared
    codegen._hipcc.compile_shared = lambda src, so, flags=(), **_: seen.update(src=src, so=so, flags=list(flags))
    try:
        codegen.build_fused(program, desc, force=True, **kw)
    finally:
        codegen._hipcc.compile_shared = real
    with open(seen["src"]) as fh:
        return fh.read(), seen["flags"], os.path.basename(seen["so"])[len("fused_"):-len(".so")]


def streams(program):
    return {str(k): dict(first=st.first, mask2=st.mask2, mask3=st.mask3, mask4=getattr(st, "mask4", 0), lap=st.lap,
                         deps=list(st.deps)) for k, st in sorted(program.streams.items())}


def module(program, desc, **kw):
    source, flags, key = build_plan(program, desc, **kw)
    return dict(closure=sha(source), flags=flags, key=key)


def fp32(make, full):
    program, descs = trace(make, False)
    mode = codegen.fuse_mode(program, descs)
    rec = dict(mode=mode, closure=sha(program.fused_source(descs[0])) if mode else None, pointwise=sha(program.source))
    if full:
        rec["streams"] = streams(program)
        if mode:
            rec["module"] = module(program, descs[0])
            assert rec["module"]["closure"] == rec["closure"]
            me = types.SimpleNamespace(program=program, descs=descs, L=_lib.lib())
            rec["eight_wave"] = bool(engine.FusedSystem._wide_possible(me))
            if rec["eight_wave"]:
                rec["module_8wave"] = module(program, descs[0], threads=512)
    return rec


def fp64(make):
    program, descs = trace(make, True)
    kind = "tile" if codegen.can_fuse_f64(program, descs) else ("multi" if codegen.can_fuse_multi_f64(program, descs) else None)
    rec = dict(closure_f64=kind, wants_closure=bool(engine.wants_closure(program, descs, True)), streams=streams(program),
               pointwise=sha(codegen.source_f64(program.source)))
    if kind:
        rec["module"] = module(program, descs[0], f64=True)
        assert rec["module"]["closure"] == sha(program.fused_source(descs[0], f64=True))
    return rec


def attempt(fn, *args):
    try:
        return fn(*args)
    except Exception as e:      # noqa: BLE001 -- a system that cannot be built / traced is a result: two checkouts must agree on it
        return dict(error=type(e).__name__)


for name in SWITCHES + ["NDQ_F64_CLOSURE", "NDQ_JIT_FLAGS", "NDQ_GROUP_WIDE"]:
    os.environ.pop(name, None)
res, summary = {}, dict(systems=0, fp32={}, fp64={})
for label, make in systems().items():
    rec = res[label] = dict(fp32=attempt(fp32, make, True), fp64=attempt(fp64, make), switches={})
    for name in SWITCHES:
        os.environ[name] = "1"
        rec["switches"][name] = attempt(fp32, make, False)
        del os.environ[name]
    summary["systems"] += 1
    for prec, field in (("fp32", "mode"), ("fp64", "closure_f64")):
        what = str(rec[prec].get(field)) if "error" not in rec[prec] else "error:" + rec[prec]["error"]
        summary[prec][what] = summary[prec].get(what, 0) + 1
    print(label, rec["fp32"].get("mode", rec["fp32"].get("error")), rec["fp64"].get("closure_f64", rec["fp64"].get("error")), flush=True)
with open(out, "w") as fh:
    json.dump(dict(summary=summary, systems=res), fh, indent=1, sort_keys=True)
print(json.dumps(summary, sort_keys=True))
