#!/usr/bin/env python3
"""Per-kernel comparison of two sets of gfx950 assembly files (hipcc ... --cuda-device-only -S, the Makefile's flags).

usage: kernel_asm_diff.py PARENT.s[,PARENT2.s...] BRANCH.s[,BRANCH2.s...] [name-filter]

For every kernel of either side: VGPRs, SGPRs, LDS bytes, private segment, instruction count (parent / branch) and whether the
instruction streams are identical after stripping comments and assembler directives and renumbering the .LBB labels.
Wrote profiles/wta_refactor.txt and profiles/pose_warp_refactor.txt."""
import re
import subprocess
import sys


def kernels(paths):
    body, meta = {}, {}
    for path in paths.split(","):
        cur, name, rec = None, None, {}
        for line in open(path):
            s = line.split(";")[0].rstrip()
            m = re.match(r"\s*\.type\s+(\S+),@function", s)
            if m:
                name, cur = m.group(1), []
                continue
            if cur is not None:
                if re.match(r"\.Lfunc_end", s):
                    body[name], cur = cur, None
                    continue
                t = s.strip()
                if not t or t == name + ":" or (t.startswith(".") and not t.endswith(":")):
                    continue
                cur.append(re.sub(r"\.LBB\d+_(\d+)", r".LBB_\1", t))
            m = re.match(r"    \.(name|vgpr_count|sgpr_count|group_segment_fixed_size|private_segment_fixed_size|wavefront_size):\s+(\S+)", s)
            if m:   # a record of amdhsa.kernels: its own keys sit at indent 4 (argument names deeper), .wavefront_size comes last
                rec[m.group(1)] = m.group(2)
                if m.group(1) == "wavefront_size":
                    meta[rec["name"]], rec = rec, {}
    return body, meta


def main():
    (pb, pm), (bb, bm) = kernels(sys.argv[1]), kernels(sys.argv[2])
    flt = sys.argv[3] if len(sys.argv) > 3 else ""
    names = sorted(n for n in set(pm) | set(bm) if flt in n)
    dem = subprocess.run(["c++filt"] + names, capture_output=True, text=True).stdout.split("\n")
    print("%-66s %9s %9s %13s %7s %11s  %s" % ("kernel", "VGPR p/b", "SGPR p/b", "LDS p/b", "priv", "insts p/b", "stream"))
    same = 0
    for n, d in zip(names, dem):
        p, b = pm.get(n), bm.get(n)
        if p is None or b is None:
            print("%-66s only on the %s side" % (d, "branch" if p is None else "parent"))
            continue
        ident = pb[n] == bb[n]
        same += ident
        cnt = lambda x: sum(1 for l in x if not l.endswith(":"))
        d = re.sub(r"\(.*\)$", "", d.replace("(anonymous namespace)::", "")).replace("void ", "").replace("cart_amd::", "")
        print("%-66s %4s/%-4s %4s/%-4s %6s/%-6s %3s/%-3s %5d/%-5d  %s" % (
            d, p["vgpr_count"], b["vgpr_count"], p["sgpr_count"], b["sgpr_count"], p["group_segment_fixed_size"], b["group_segment_fixed_size"],
            p["private_segment_fixed_size"], b["private_segment_fixed_size"], cnt(pb[n]), cnt(bb[n]), "identical" if ident else "DIFFERENT"))
    print("%d kernels, %d identical" % (len(names), same))


if __name__ == "__main__":
    main()
