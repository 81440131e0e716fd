#!/usr/bin/env python
"""The gfx950 device code of libndq.so and libndq64.so, kernel by kernel, as JSON: run it on two checkouts and compare -- a
change to the C-ABI sources that is meant to leave the kernels alone shows as an empty difference (no GPU needed).

Both libraries are built into a scratch directory with the checkout's own ``_hipcc.compile_shared`` and ``_build`` flags
(assembly fix-up pass included), the gfx950 code object is taken out of the fat binary and disassembled.  Per kernel symbol:
  isa       SHA-1 of the instruction text -- addresses, encodings and the disassembler's branch-target comments stripped
  n_insts   number of instructions
  vgpr / agpr / sgpr / lds / scratch    the figures of the code object's metadata note
It only hashes and tabulates.
usage: scripts/lib_isa_digests.py TREE OUT.json"""
import sys, os, re, json, hashlib, subprocess, tempfile
tree, out = os.path.abspath(sys.argv[1]), sys.argv[2]
sys.path.insert(0, tree)
from neurodiffeq_amd import _build, _hipcc

TARGET = f"hipv4-amdgcn-amd-amdhsa--{_hipcc.ARCH}"
META = dict(vgpr=".vgpr_count", agpr=".agpr_count", sgpr=".sgpr_count", lds=".group_segment_fixed_size",
            scratch=".private_segment_fixed_size")


def tool(name, *args):
    return subprocess.run([os.path.join(_hipcc.LLVM_BIN, name)] + list(args), check=True, capture_output=True, text=True).stdout


def code_object(lib, work):
    fat, co = os.path.join(work, "fatbin"), os.path.join(work, "code_object")
    tool("llvm-objcopy", "--dump-section", f".hip_fatbin={fat}", lib)
    tool("clang-offload-bundler", "--unbundle", "--type=o", f"--targets={TARGET}", f"--input={fat}", f"--output={co}")
    return co


def metadata(co):
    """kernel name -> register / LDS / scratch figures, from the amdhsa.kernels list of the metadata note"""
    notes = tool("llvm-readelf", "--notes", co)
    kernels = notes.split("amdhsa.kernels:", 1)[1].split("amdhsa.target:", 1)[0]
    res = {}
    for entry in re.split(r"^  - ", kernels, flags=re.M)[1:]:          # (a kernel's own fields: first line, or indented by four)
        fields = dict(re.findall(r"^(?:    )?\.(\w+):\s+(\S+)\s*$", entry, flags=re.M))
        res[fields["name"].strip("'\"")] = {k: int(fields.get(v[1:], 0)) for k, v in META.items()}
    return res


def instructions(co):
    """function symbol -> list of instruction lines (mnemonic + operands only)"""
    res, cur = {}, None
    for line in tool("llvm-objdump", "-d", "--no-show-raw-insn", co).split("\n"):
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            cur = res.setdefault(m.group(1), [])
            continue
        text = re.sub(r"\s+", " ", line.split("//")[0].split("<")[0]).strip()
        if cur is not None and text and text != "...":          # ("...": a run of zero bytes the disassembler skipped)
            cur.append(text)
    for insts in res.values():          # what follows a kernel's last instruction only fills up to the next symbol's alignment
        while insts and insts[-1] in ("s_nop 0", "s_code_end"):
            insts.pop()
    return res


def digest(sources, flags, work):
    lib = os.path.join(work, "lib.so")
    _hipcc.compile_shared(sources, lib, flags)
    co = code_object(lib, work)
    meta, insts = metadata(co), instructions(co)
    return {name: dict(isa=hashlib.sha1("\n".join(insts[name]).encode()).hexdigest(), n_insts=len(insts[name]), **figures)
            for name, figures in meta.items()}


res = {}
for label, sources, flags in (("libndq", _build.SOURCES, _build.FLAGS), ("libndq64", _build.SOURCES64, [])):
    with tempfile.TemporaryDirectory() as work:
        res[label] = digest(sources, flags, work)
    print(label, len(res[label]), "kernels", flush=True)
with open(out, "w") as fh:
    json.dump(res, fh, indent=1, sort_keys=True)
