#!/usr/bin/env python3
"""Compare the gfx950 device code of two source trees, kernel by kernel.

    tools/isa_compare.py PARENT_TREE CHANGE_TREE [--work DIR]

Every .hip translation unit of the three libraries (snappy.jl_amd/csrc, csrc/framing, csrc/multi)
is compiled for the device alone to assembly with its Makefile's flags, in both trees.  Per kernel
(and per device function that was not inlined) the instruction stream and the .amdhsa_kernel block
(VGPRs, SGPRs, LDS, scratch, ...) are compared as text; so is everything else in the file (tables,
the metadata note).  One line per kernel is printed; the exit status is 1 if anything differs.
CPU only: nothing is launched.
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
BASE = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fno-strict-aliasing", "-fPIC", "-Wall"]
SCHED = ["-mllvm", "-amdgpu-sched-strategy=max-ilp"]
CSRC = os.path.join("snappy.jl_amd", "csrc")
# (directory, extra flags, the files that take no SCHED) -- as the three Makefiles build them
LIBS = [(CSRC, ['-DSM_VERSION_STR="isa"'] + SCHED, {"sm_compress_sc.hip"}),
        (os.path.join(CSRC, "framing"), [], set()),
        (os.path.join(CSRC, "multi"), [], set())]


def command(src, extra, out):
    return [HIPCC] + BASE + extra + ["--offload-device-only", "-S", "-o", out, src]


def assemble(tree, work, tag):
    """{(dir, file): assembly text} of every translation unit of `tree`."""
    out = {}
    for d, extra, plain in LIBS:
        for f in sorted(os.listdir(os.path.join(tree, d))):
            if not f.endswith(".hip"):
                continue
            flags = [x for x in extra if f not in plain or x not in SCHED]
            s = os.path.join(work, "%s_%s.s" % (tag, f))
            subprocess.run(command(f, flags, s), cwd=os.path.join(tree, d), check=True)
            out[(d, f)] = open(s).read()
    return out


def split(asm):
    """({function: instructions}, {kernel: .amdhsa_kernel block}, the rest) of one assembly file."""
    funcs, descs, rest = {}, {}, []
    # (the compilation unit's id hashes the file's path)
    asm = re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid", asm)
    lines = [l for l in asm.splitlines() if not re.match(r"\s*\.(file|ident)\b", l)]
    i = 0
    while i < len(lines):
        m = re.match(r"\s*\.type\s+(\S+),@function", lines[i])
        if not m:
            rest.append(lines[i])
            i += 1
            continue
        end = re.compile(r"\s*\.size\s+%s," % re.escape(m.group(1)))
        body, desc = [], []
        while not end.match(lines[i]):
            into = desc if desc and not re.match(r"\s*\.end_amdhsa_kernel", desc[-1]) else body
            (desc if re.match(r"\s*\.amdhsa_kernel\b", lines[i]) else into).append(lines[i])
            i += 1
        funcs[m.group(1)] = "\n".join(body + [lines[i]])
        if desc:
            descs[m.group(1)] = "\n".join(desc)
        i += 1
    return funcs, descs, "\n".join(rest)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent")
    ap.add_argument("change")
    ap.add_argument("--work", default=None)
    a = ap.parse_args()
    work = a.work or tempfile.mkdtemp(prefix="isa_")
    os.makedirs(work, exist_ok=True)
    print("command, per translation unit, in its directory (SCHED = %s; not for sm_compress_sc.hip):" % " ".join(SCHED))
    print("  " + " ".join(command("<file>.hip", ["[SCHED]"], "<file>.s")))
    old, new = assemble(a.parent, work, "parent"), assemble(a.change, work, "change")
    differ = 0
    for key in sorted(set(old) | set(new)):
        name = os.path.join(*key)
        if key not in old or key not in new:
            print("%s: only in the %s tree" % (name, "change" if key in new else "parent"))
            differ += 1
            continue
        (f0, d0, r0), (f1, d1, r1) = split(old[key]), split(new[key])
        for fn in sorted(set(f0) | set(f1)):
            kind = "kernel" if fn in d0 or fn in d1 else "function"
            same = f0.get(fn) == f1.get(fn) and d0.get(fn) == d1.get(fn)
            what = "identical" if same else ("DIFFERENT" if fn in f0 and fn in f1 else "MISSING on one side")
            if kind == "kernel" and f0.get(fn) == f1.get(fn) and not same:
                what = "DIFFERENT (resource metadata only)"
            print("%s: %s %s: %s" % (name, kind, fn, what))
            differ += not same
        same = r0 == r1
        print("%s: everything else (tables, metadata note): %s" % (name, "identical" if same else "DIFFERENT"))
        differ += not same
    print("%d difference(s)" % differ)
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
