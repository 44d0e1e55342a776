#!/usr/bin/env python3
"""The ragged batches' kernel resources: every instantiation in another build's -Rpass-analysis=kernel-resource-usage logs
(the parent's tree, built with the same Makefile) against the one of the same name in this tree's, then the ragged
instantiations beside the instantiation they were made from.
    python tools/ragged_resources.py <the other tree's glfer_amd/csrc/build> > profiles/ragged_kernel_resources.txt"""
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


old, new = read(sys.argv[1]), read(os.path.join(root, "glfer_amd", "csrc", "build"))
# a name gained a defaulted template argument where a kernel gained a RAG form: <.., 0> is the instantiation that was <..>
twin = {}
for name in new:
    m = re.match(r"((?:hop_means_seq|submean|submean_reg)_kernel<.*), 0>$", name)
    twin[m.group(1) + ">" if m else name] = name
same = [n for n in old if n in twin]
changed = [n for n in same if old[n] != new[twin[n]]]
print("instantiations in the parent: %d, with the same name in this tree: %d, resources identical: %d, changed: %d"
      % (len(old), len(same), len(same) - len(changed), len(changed)))
for n in changed:
    print("  CHANGED %s\n    parent %s\n    now    %s" % (n, fmt(old[n]), fmt(new[twin[n]])))
missing = [n for n in old if n not in twin]
for n in missing:
    print("  MISSING in this tree: %s" % n)
fresh = sorted(n for n in new if n not in [twin[s] for s in same])
print("new instantiations: %d" % len(fresh))
worse = 0
for n in fresh:
    t = n.replace("_ragged_kernel", "_kernel")
    t = re.sub(r", 1>$", ", 0>", t) if t == n else t
    tw = new.get(t)
    if tw and (new[n][2] > tw[2] or new[n][6] < tw[6] or new[n][5] > tw[5]):
        worse += 1
    print("  %-58s %s | twin %s" % (n, fmt(new[n]), fmt(tw) if tw else "-"))
print("ragged forms that spill more or hold fewer wavefronts than their twins: %d" % worse)
