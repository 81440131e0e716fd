#!/usr/bin/env python
"""Closure mode and SHA-1 of the generated closure / pointwise sources of every system of tests/configs.py and tests/zoo.py, as
JSON: run it on two checkouts and compare -- a change to the code generator that is meant to leave existing modes alone shows
as an empty difference (no GPU needed).
usage: scripts/closure_source_digests.py TREE OUT.json"""
import sys, json, hashlib
tree, out = sys.argv[1], sys.argv[2]
sys.path.insert(0, tree)
import torch
from neurodiffeq_amd import codegen, engine
from tests import configs, zoo
res = {}
names = ["c1", "c2", "c3", "c4", "c5"] + [f"w{i}" for i in list(range(1, 22)) + list(range(24, 31))]
for name in names:
    torch.manual_seed(0)
    try:
        cfg = configs.make(name, 8 if name.startswith("c") else None)
    except Exception as e:
        continue
    program, descs = engine.trace_system(cfg["nets"], cfg["conds"], configs.fused_equations(cfg), configs.n_coords(cfg), compute_func_val=configs.func_val(cfg))
    mode = codegen.fuse_mode(program, descs)
    res["cfg/" + name] = (mode, hashlib.sha1(program.fused_source(descs[0]).encode()).hexdigest() if mode else None, hashlib.sha1(program.source.encode()).hexdigest())
for name in zoo.NAMES:
    torch.manual_seed(0)
    z = zoo.build(name)
    nets, conds, pde = z.product()
    program, descs = engine.trace_system(nets, conds, pde, z.n_coords)
    mode = codegen.fuse_mode(program, descs)
    res["zoo/" + name] = (mode, hashlib.sha1(program.fused_source(descs[0]).encode()).hexdigest() if mode else None, hashlib.sha1(program.source.encode()).hexdigest())
json.dump(res, open(out, "w"), indent=1)
