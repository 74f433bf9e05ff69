#!/usr/bin/env python3
"""Refactoring guard: two builds of libmapdit_hip.so contain the same gfx950 device code.

A change that only deletes dead code or reshapes the host side of a kernel file must not move a single instruction of a shipped
kernel.  This script makes that a checked property: it unbundles the gfx950 code objects of both libraries (the same way
tools/check_packed_fp32.py does), disassembles them, and compares function by function, on demangled names:

  * both libraries contain the same set of device functions;
  * every function's instruction stream is the same, byte for byte (mnemonics and encodings; the addresses the disassembler
    prints beside them, and the symbol + offset it prints after a branch, are not part of the comparison).  One kind of symbol
    address sits inside an encoding: the pc-relative distance to a global (`s_getpc_b64 sN` followed by `s_add_u32 sN, sN,
    <32-bit literal>`, e.g. the zero word the GEMM K tails read).  It moves whenever the functions of a code object are emitted in
    another order, so that literal, and nothing else, is masked; the summary line counts the masked sites;
  * every kernel's descriptor says the same: register counts, spills, LDS (group segment) size, scratch (private segment) size,
    kernel-argument size, workgroup size limit (the code objects' AMDGPU metadata notes).

Needs no GPU.  A template parameter that a refactor removed on purpose is dropped from the OLD names before they are matched:
--drop-template-arg gemm_mfma256_kernel:4 removes the fifth argument of every gemm_mfma256_kernel<...>.

    python tools/compare_device_code.py OLD.so NEW.so [--drop-template-arg NAME:INDEX ...]      exit status 0 = no difference
"""
import argparse
import os
import re
import shutil
import subprocess
import sys

from check_packed_fp32 import LLVM, SYMBOL, code_objects

INSN = re.compile(r"^\s+(\S+)[^/]*// [0-9A-F]+: ((?:[0-9A-F]{8} ?)+)")
PCREL_LO = re.compile(r"^80..FF.. [0-9A-F]{8}$")              # s_add_u32 sN, sN, literal
KD_KEYS = ("agpr_count", "vgpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "group_segment_fixed_size",
           "private_segment_fixed_size", "kernarg_segment_size", "max_flat_workgroup_size", "uses_dynamic_stack")


def drop_template_arg(name, func, index):
    """`func<a0, a1, ...>` -> the same without argument `index` (top-level commas only), wherever it occurs in a demangled name."""
    out, pos = "", 0
    for m in re.finditer(r"\b%s<" % re.escape(func), name):
        if m.start() < pos:
            continue
        depth, i, args, start = 1, m.end(), [], m.end()
        while depth:
            c = name[i]
            if c in "<(":
                depth += 1
            elif c in ">)":
                depth -= 1
            if (c == "," and depth == 1) or depth == 0:
                args.append(name[start:i].strip())
                start = i + 1
            i += 1
        del args[index]
        out += name[pos:m.end()] + ", ".join(args) + ">"
        pos = i
    return out + name[pos:]


def device_code(lib, drops):
    """{demangled name: (instruction stream, descriptor fields or None)} of every device function of every gfx950 code object."""
    raw = []                                                   # (mangled name, [(mnemonic, encoding)], descriptor)
    for path, dis in code_objects(lib):
        notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", path], check=True, capture_output=True, text=True).stdout
        kd = {}
        for entry in re.split(r"^  - (?=\.)", notes, flags=re.M)[1:]:
            fields = dict(re.findall(r"^(?:    )?\.(\w+):\s+(\S+)$", entry, flags=re.M))
            kd[fields["name"]] = tuple((k, fields.get(k)) for k in KD_KEYS)
        cur = None
        for line in dis.splitlines():
            m = SYMBOL.match(line)
            if m:
                cur = []
                raw.append((m.group(1), cur, kd.get(m.group(1))))
                continue
            m = INSN.match(line)
            if m and cur is not None:
                op, enc = m.group(1), m.group(2).strip()
                if op == "s_add_u32" and cur and cur[-1][0] == "s_getpc_b64" and PCREL_LO.match(enc):
                    enc = enc[:8] + " pc-rel"
                cur.append((op, enc))
    cxxfilt = shutil.which("llvm-cxxfilt", path=LLVM + os.pathsep + os.environ.get("PATH", "")) or shutil.which("c++filt")
    if not cxxfilt:
        sys.exit("compare_device_code: needs llvm-cxxfilt or c++filt to demangle kernel names")
    names = subprocess.run([cxxfilt], input="\n".join(r[0] for r in raw), check=True, capture_output=True,
                           text=True).stdout.splitlines()
    out = {}
    for name, (_, insns, desc) in zip(names, raw):
        for func, index in drops:
            name = drop_template_arg(name, func, index)
        n, key = 1, name
        while key in out:                                      # the same internal-linkage name in two translation units
            n += 1
            key = f"{name} #{n}"
        out[key] = (insns, desc)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--drop-template-arg", action="append", default=[], metavar="NAME:INDEX",
                    help="remove template argument INDEX (from 0) of NAME<...> from the OLD library's names before matching")
    a = ap.parse_args()
    drops = [(d.rsplit(":", 1)[0], int(d.rsplit(":", 1)[1])) for d in a.drop_template_arg]
    old, new = device_code(a.old, drops), device_code(a.new, [])
    only_old, only_new = sorted(set(old) - set(new)), sorted(set(new) - set(old))
    common = sorted(set(old) & set(new))
    differing = 0
    for k in common:
        (oi, od), (ni, nd) = old[k], new[k]
        what = []
        if oi != ni:
            first = next((i for i, (x, y) in enumerate(zip(oi, ni)) if x != y), min(len(oi), len(ni)))
            what.append(f"instructions differ from #{first} on ({len(oi)} vs {len(ni)})")
        if od != nd:
            what.append("descriptor: " + ", ".join(f"{k0} {v0} -> {v1}" for (k0, v0), (_, v1) in zip(od or (), nd or ()) if v0 != v1)
                        if od and nd else "descriptor: kernel in one library only")
        if what:
            differing += 1
            print(f"  DIFFERS    {k[:160]}\n             " + "; ".join(what))
    for k in only_old:
        print(f"  ONLY IN OLD  {k[:160]}")
    for k in only_new:
        print(f"  ONLY IN NEW  {k[:160]}")
    kernels = sum(1 for k in common if old[k][1])
    print(f"{len(common)} device functions compared ({kernels} kernels with descriptors, "
          f"{sum(len(old[k][0]) for k in common)} instructions, "
          f"{sum(e.endswith('pc-rel') for k in common for _, e in new[k][0])} pc-relative literals masked), {differing} differing, "
          f"{len(only_old)} only in {a.old}, {len(only_new)} only in {a.new}")
    return 1 if differing or only_old or only_new else 0


if __name__ == "__main__":
    sys.exit(main())
