#!/usr/bin/env python3
"""The ragged F entries' kernel resources, from the -Rpass-analysis=kernel-resource-usage logs of two builds made with the same
Makefile: the parent's tree against this one.  Three lists: the instantiations without GLFER_RAGGED (they must be identical),
the ragged instantiations the parent already had (GlferRaggedEntry grew: before and after), and the new ragged F forms beside
the BAT = 1 instantiation of the same template arguments.
    python tools/ragged_ftest_resources.py <the parent tree's glfer_amd/csrc/build>"""
import glob, os, re, subprocess, sys

root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = [("VGPR", "VGPRs"), ("AGPR", "AGPRs"), ("spill", "VGPRs Spill"), ("SGPR", "TotalSGPRs"), ("SGPRspill", "SGPRs Spill"),
          ("scratch", r"ScratchSize \[bytes/lane\]"), ("occ", r"Occupancy \[waves/SIMD\]"), ("LDS", r"LDS Size \[bytes/block\]")]


def read(build):
    out, names = {}, []
    for path in sorted(glob.glob(os.path.join(build, "*.log"))):
        for b in open(path).read().split("Function Name: ")[1:]:
            names.append(b.split(" ")[0])
            out[names[-1]] = tuple(int(re.search(k + r": (\d+)", b).group(1)) for _, k in FIELDS)
    dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    short = lambda s: re.sub(r"\(.*\)$", "", s.replace("void glfer::", "").replace("void ", ""))
    return {short(d): out[n] for n, d in zip(names, dem)}


def fmt(r):
    return " ".join("%s %d" % (f[0], v) for f, v in zip(FIELDS, r))


def is_ragged(name):
    return "_ragged_kernel" in name


old, new = read(sys.argv[1]), read(os.path.join(root, "glfer_amd", "csrc", "build"))
for title, pick in (("without GLFER_RAGGED", lambda n: not is_ragged(n)), ("ragged, already in the parent", is_ragged)):
    names = [n for n in old if pick(n)]
    missing = [n for n in names if n not in new]
    changed = [n for n in names if n in new and old[n] != new[n]]
    print("instantiations %s: %d in the parent, %d missing in this tree, %d with identical VGPR / AGPR / spill / SGPR / scratch / "
          "occupancy / LDS, %d changed" % (title, len(names), len(missing), len(names) - len(missing) - len(changed), len(changed)))
    for n in missing:
        print("  MISSING %s" % n)
    for n in changed:
        print("  CHANGED %s\n    parent %s\n    now    %s" % (n, fmt(old[n]), fmt(new[n])))
fresh = sorted(n for n in new if n not in old)
print("new instantiations: %d (not ragged: %d)" % (len(fresh), sum(not is_ragged(n) for n in fresh)))
differ = 0
for n in fresh:
    tw = new.get(n.replace("_ragged_kernel", "_kernel")) if is_ragged(n) else None
    mark = ""
    if tw and tw != new[n]:
        differ += 1
        mark = "  <-- differs"
    print("  %-58s %s | BAT = 1 twin %s%s" % (n, fmt(new[n]), fmt(tw) if tw else "-", mark))
print("new ragged forms whose resources differ from their twins' in any field: %d" % differ)
