#!/usr/bin/env python3
"""profiles/rows_ftest_kernel_resources.txt: the compiler's own resource report (-Rpass-analysis=kernel-resource-usage, the
logs the Makefile leaves under glfer_amd/csrc/build/) of every kernel of this tree against a parent tree's logs, and of every
ROWS instantiation of spectro16_kernel beside its FT twin.

usage: rows_ftest_resources.py <parent build dir with *.log> [this tree's build dir]

spectro16_kernel gained a trailing template parameter (ROWS, default 0): a parent name is matched to this tree's name with
ROWS = 0 appended.  The parent's spectro16 logs are made by adding the same -Rpass-analysis option to its spectro16 rule."""
import glob
import os
import re
import sys

FIELDS = (("VGPR", r"VGPRs"), ("AGPR", r"AGPRs"), ("spill", r"VGPRs Spill"), ("SGPRspill", r"SGPRs Spill"),
          ("scratch", r"ScratchSize \[bytes/lane\]"), ("occ", r"Occupancy \[waves/SIMD\]"), ("LDS", r"LDS Size \[bytes/block\]"))
KERNEL = re.compile(r"_ZN5glfer16spectro16_kernelILi(\d+)ELi(\d)ELb(\d)ELi(\d)ELi(\d+)ELi(\d+)ELi(\d)ELi(\d)(?:ELi(\d))?EEEv13SpectroParams")


def load(build):
    out = {}
    for path in sorted(glob.glob(os.path.join(build, "*.log"))):
        unit = os.path.basename(path)[:-4]
        for b in open(path).read().split("Function Name: ")[1:]:
            name = b.split(" ")[0]
            out[(unit, name)] = tuple(int(re.search(k + r": (\d+)", b).group(1)) for _, k in FIELDS)
    return out


def fmt(r):
    return " ".join("%s %d" % (f[0], v) for f, v in zip(FIELDS, r))


def main():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    parent = load(sys.argv[1])
    new = load(sys.argv[2] if len(sys.argv) > 2 else os.path.join(root, "glfer_amd", "csrc", "build"))

    def renamed(name):                                      # the parent's spectro16_kernel name in this tree: ROWS = 0 appended
        m = KERNEL.fullmatch(name)
        return name.replace("EEEv13SpectroParams", "ELi0EEEv13SpectroParams") if m and m.group(9) is None else name

    same = changed = 0
    lines = []
    for (unit, name), r in sorted(parent.items()):
        key = (unit, renamed(name))
        if key not in new:
            lines.append("  %-16s %s: not in this tree" % (unit, name))
            continue
        if new[key] == r:
            same += 1
        else:
            changed += 1
            lines.append("  %-16s %s\n      parent %s\n      now    %s" % (unit, name, fmt(r), fmt(new[key])))
    print("Existing kernels (the parent's %d), resources identical: %d, changed: %d" % (len(parent), same, changed))
    for ln in lines:
        print(ln)
    print()
    print("spectro16_kernel<LOGN, FMT, GEN, WPS, STG, KM, FT, BAT, ROWS>: every ROWS = 1 instantiation beside its FT twin (ROWS = 0,")
    print("the F entries' kernel of the same size, format, form and batch flag)")
    for (unit, name), r in sorted(new.items()):
        m = KERNEL.fullmatch(name)
        if not m or m.group(9) != "1":
            continue
        logn, f, gen, wps, stg, km, ft, bat, _ = m.groups()
        twin = None
        for (u2, n2), r2 in new.items():
            m2 = KERNEL.fullmatch(n2)
            if u2 == unit and m2 and m2.group(9) == "0" and m2.groups()[:3] == (logn, f, gen) and m2.groups()[5:8] == (km, ft, bat):
                twin = (m2.group(4), r2)
        note = ""
        if twin and (r[5] < twin[1][5] or r[4] > twin[1][4]):
            note = "   <-- fewer waves/SIMD or more scratch than the twin"
        print("  N %-5d fmt %s FT %s BAT %s  rows (WPS %s): %s" % (1 << int(logn), f, ft, bat, wps, fmt(r)))
        print("  %-24s  twin (WPS %s): %s%s" % ("", twin[0], fmt(twin[1]), note))


if __name__ == "__main__":
    main()
