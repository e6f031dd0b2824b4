#!/usr/bin/env python3
"""Static VALU counts of a decoder kernel's per-tag decode, from its gfx950 assembly.

    tools/count_valu.py FILE.s [--kernel k_decompress]

FILE.s is sm_decompress.hip compiled for the device alone (the command tools/isa_compare.py
prints).  Three counts of instructions that issue on the vector ALU (mnemonics v_*, the
v_readlane/v_readfirstlane reads included), for the first function whose name holds --kernel:

  kernel     every VALU instruction of the function, cold paths included;
  tag decode the straight-line code from the last branch before the tag's ring read (the
             ds_read2_b32 nearest the decode's `v_lshlrev_b64 ..., -1` marker, the only inline asm
             of that form there) and before the marker itself, to the first v_readlane_b32 after
             both (the batch's total output): one tag's fields, the wave scan and the checks that
             every batch runs;
  of which   64-bit compares (v_cmp_*_{i,u}64), and instructions inside exec-masked blocks
             (between an s_and_saveexec and the next s_or_b64 exec).

CPU only: nothing is launched.  The counts are static: they say what one pass over the region
issues, not how often the region runs.
"""
import argparse
import re
import sys


def function_body(asm, key):
    lines = asm.splitlines()
    for i, l in enumerate(lines):
        m = re.match(r"\s*\.type\s+(\S+),@function", l)
        if m and key in m.group(1):
            name = m.group(1)
            end = re.compile(r"\s*\.size\s+%s," % re.escape(name))
            j = i
            while not end.match(lines[j]) and not re.match(r"\s*\.amdhsa_kernel\b", lines[j]):
                j += 1
            return name, lines[i:j]
    sys.exit("no function with %r in its name" % key)


def is_valu(line):
    return re.match(r"\s+v_\w+", line) is not None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("asm")
    ap.add_argument("--kernel", default="k_decompressENS")
    a = ap.parse_args()
    name, body = function_body(open(a.asm).read(), a.kernel)
    total = sum(is_valu(l) for l in body)
    # (k_decompress_frags walks to its first tag with the same marker and no ring read: the batch
    # loop's marker is the first with a ds_read2_b32 within 40 lines of it)
    marks = [i for i, l in enumerate(body) if re.match(r"\s+v_lshlrev_b64 v\[\d+:\d+\], v\d+, -1", l)]
    near = lambda i: [j for j in range(max(i - 40, 0), min(i + 40, len(body))) if re.match(r"\s+ds_read2_b32", body[j])]
    mark = next(i for i in marks if near(i))
    ring = min(near(mark), key=lambda j: abs(j - mark))
    lo = max(i for i in range(min(mark, ring)) if re.match(r"\s+s_cbranch", body[i])) + 1
    hi = next(i for i in range(max(mark, ring), len(body)) if re.match(r"\s+v_readlane_b32", body[i]))
    region = body[lo:hi]
    masked, inside, cmp64 = 0, False, 0
    for l in region:
        if re.match(r"\s+s_and_saveexec_b64", l):
            inside = True
        elif re.match(r"\s+s_or_b64 exec,", l):
            inside = False
        elif is_valu(l):
            masked += inside
            cmp64 += re.match(r"\s+v_cmp_\w+_[iu]64", l) is not None
    print("%s" % name)
    print("kernel      %5d VALU (static, cold paths included)" % total)
    print("tag decode  %5d VALU (block of the ring read to the batch's output total)" % sum(is_valu(l) for l in region))
    print("  of which  %5d 64-bit compares, %d in exec-masked blocks" % (cmp64, masked))
    for m in re.finditer(r"\.set %s\.(num_vgpr|private_seg_size), (\d+)" % re.escape(name), open(a.asm).read()):
        print("%s %s" % (m.group(1), m.group(2)))


if __name__ == "__main__":
    main()
