"""Kernel-by-kernel digests of the gfx950 code object inside a shared library built by a checkout's own ``_hipcc.compile_shared``
(assembly fix-up pass included): what ``lib_isa_digests.py`` (the two C-ABI libraries) and ``closure_isa_digests.py`` (generated
modules) tabulate.  Per kernel symbol:
  isa       SHA-1 of the instruction text -- addresses, encodings and the disassembler's branch-target comments stripped
  n_insts   number of instructions
  vgpr / agpr / sgpr / lds / scratch    the figures of the code object's metadata note
It only hashes and tabulates."""
import os, re, sys, hashlib, subprocess

META = dict(vgpr=".vgpr_count", agpr=".agpr_count", sgpr=".sgpr_count", lds=".group_segment_fixed_size",
            scratch=".private_segment_fixed_size")
_hipcc = None


def use_tree(tree):
    """Import the package of the checkout at ``tree`` (its build flags, its fix-up pass); returns the absolute path."""
    global _hipcc
    tree = os.path.abspath(tree)
    sys.path.insert(0, tree)
    from neurodiffeq_amd import _hipcc as module
    _hipcc = module
    return tree


def tool(name, *args):
    return subprocess.run([os.path.join(_hipcc.LLVM_BIN, name)] + list(args), check=True, capture_output=True, text=True).stdout


def code_object(lib, work):
    fat, co = os.path.join(work, "fatbin"), os.path.join(work, "code_object")
    tool("llvm-objcopy", "--dump-section", f".hip_fatbin={fat}", lib)
    tool("clang-offload-bundler", "--unbundle", "--type=o", f"--targets=hipv4-amdgcn-amd-amdhsa--{_hipcc.ARCH}",
         f"--input={fat}", f"--output={co}")
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


def digest_lib(lib, work):
    co = code_object(lib, work)
    meta, insts = metadata(co), instructions(co)
    return {name: dict(isa=hashlib.sha1("\n".join(insts[name]).encode()).hexdigest(), n_insts=len(insts[name]), **figures)
            for name, figures in meta.items()}


def digest(sources, flags, work):
    """Build ``sources`` with ``flags`` into the scratch directory ``work`` and digest the result."""
    lib = os.path.join(work, "lib.so")
    _hipcc.compile_shared(sources, lib, flags)
    return digest_lib(lib, work)
