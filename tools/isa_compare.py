#!/usr/bin/env python3
"""Compare the gfx950 device code of two source trees, kernel by kernel.

    tools/isa_compare.py PARENT_TREE CHANGE_TREE [--work DIR]

Every .hip translation unit of the eight library directories (snappy.jl_amd/csrc and, under it,
framing, multi, blocks, orc, parquet, avro and table) is compiled for the device alone to assembly
with its Makefile's flags, in both trees.  Per kernel
(and per device function that was not inlined) the instruction stream and the .amdhsa_kernel block
(VGPRs, SGPRs, LDS, scratch, ...) are compared as text; so is everything else in a file that both
trees have (tables, the metadata note).  Kernels are matched by name within a library, so one that
moved to another translation unit is compared with its parent there.  One line per kernel is
printed, with both sides' register, LDS and scratch figures when it differs; the exit status is 1
if anything differs.  CPU only: nothing is launched.
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
# (directory, extra flags, the files that take no SCHED) -- as the Makefiles build them: the main
# library's own, and common/companion.mk's BASE alone for every companion
LIBS = [(CSRC, ['-DSM_VERSION_STR="isa"'] + SCHED, {"sm_compress_sc.hip"})] + [
    (os.path.join(CSRC, d), [], set()) for d in ("framing", "multi", "blocks", "orc", "parquet", "avro", "table")]


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
            s = os.path.join(work, "%s_%s_%s.s" % (tag, os.path.basename(d), f))
            subprocess.run(command(f, flags, s), cwd=os.path.join(tree, d), check=True)
            out[(d, f)] = open(s).read()
    return out


def split(asm):
    """({function: instructions}, {kernel: .amdhsa_kernel block}, the rest) of one assembly file."""
    funcs, descs, rest = {}, {}, []
    # (the compilation unit's id hashes the file's path)
    asm = re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid", asm)
    # (local labels carry the function's index in its file: .LBB7_3, .Lfunc_end7, .LJTI7_0)
    asm = re.sub(r"\.L(JTI|func_begin|func_end)\d+", r".L\1", asm)
    asm = re.sub(r"BB\d+_(\d+)", r"BB_\1", asm)  # (labels and the loop comments that name them)
    asm = re.sub(r"[ \t]+;", " ;", asm)            # (a comment's column moves with the label's width)
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


FIGURES = (("vgpr", "next_free_vgpr"), ("sgpr", "next_free_sgpr"), ("lds", "group_segment_fixed_size"),
           ("scratch", "private_segment_fixed_size"))


def figures(desc):
    """The register, LDS and scratch figures of an .amdhsa_kernel block, as one string."""
    got = dict(re.findall(r"\.amdhsa_(\w+)\s+(\S+)", desc or ""))
    return " ".join("%s=%s" % (short, got.get(key, "?")) for short, key in FIGURES)


def by_name(files):
    """{function: [(file, instructions, descriptor)]} over a library's translation units."""
    out = {}
    for f in sorted(files):
        funcs, descs, _ = files[f]
        for fn, body in funcs.items():
            out.setdefault(fn, []).append((f, body, descs.get(fn)))
    return out


def pairs(a, b):
    """Pair a function's copies in the two trees: the same file first, then moved ones in order."""
    fa, fb = {x[0]: x for x in a}, {x[0]: x for x in b}
    both = sorted(set(fa) & set(fb))
    la, lb = [fa[f] for f in sorted(set(fa) - set(fb))], [fb[f] for f in sorted(set(fb) - set(fa))]
    n = max(len(la), len(lb))
    return [(fa[f], fb[f]) for f in both] + list(zip(la + [None] * (n - len(la)), lb + [None] * (n - len(lb))))


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
    for d, _, _ in LIBS:
        s0 = {f: split(t) for (dd, f), t in old.items() if dd == d}
        s1 = {f: split(t) for (dd, f), t in new.items() if dd == d}
        n0, n1 = by_name(s0), by_name(s1)
        for fn in sorted(set(n0) | set(n1)):
            for x, y in pairs(n0.get(fn, []), n1.get(fn, [])):
                where = os.path.join(d, (y or x)[0])
                if x and y and x[0] != y[0]:
                    where += " (parent: %s)" % x[0]
                kind = "kernel" if (x and x[2]) or (y and y[2]) else "function"
                if not x or not y:
                    what = "only in the %s tree" % ("change" if y else "parent")
                elif x[1:] == y[1:]:
                    what = "identical"
                else:
                    what = "DIFFERENT" if x[1] != y[1] else "DIFFERENT (resource metadata only)"
                    if kind == "kernel":
                        what += "\n    parent: %s\n    change: %s" % (figures(x[2]), figures(y[2]))
                print("%s: %s %s: %s" % (where, kind, fn, what))
                differ += what != "identical"
        for f in sorted(set(s0) | set(s1)):
            name = os.path.join(d, f)
            if f not in s0 or f not in s1:
                print("%s: only in the %s tree" % (name, "change" if f in s1 else "parent"))
                continue
            same = s0[f][2] == s1[f][2]
            print("%s: everything else (tables, metadata note): %s" % (name, "identical" if same else "DIFFERENT"))
            differ += not same
    print("%d difference(s)" % differ)
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
