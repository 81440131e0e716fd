#!/usr/bin/env python
"""The gfx950 device code of libndq.so and libndq64.so, kernel by kernel, as JSON: run it on two checkouts and compare -- a
change to the C-ABI sources that is meant to leave the kernels alone shows as an empty difference (no GPU needed).

Both libraries are built into a scratch directory with the checkout's own ``_hipcc.compile_shared`` and ``_build`` flags
(assembly fix-up pass included, NDQ_LIB_FLAGS honoured), the gfx950 code object is taken out of the fat binary and
disassembled; what is recorded per kernel symbol: ``_isa_digest.py``.  It only hashes and tabulates.
usage: scripts/lib_isa_digests.py TREE OUT.json"""
import sys, os, json, tempfile
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _isa_digest

if __name__ == "__main__":
    tree, out = _isa_digest.use_tree(sys.argv[1]), sys.argv[2]
    from neurodiffeq_amd import _build
    res = {}
    for label, sources, flags in (("libndq", _build.SOURCES, _build.FLAGS), ("libndq64", _build.SOURCES64, [])):
        with tempfile.TemporaryDirectory() as work:
            res[label] = _isa_digest.digest(sources, flags, work)
        print(label, len(res[label]), "kernels", flush=True)
    with open(out, "w") as fh:
        json.dump(res, fh, indent=1, sort_keys=True)
