#!/usr/bin/env python3
"""hparma.hip's kernel resources in the parent and in this tree, from two -Rpass-analysis=kernel-resource-usage logs of the
same compile line (the Makefile's, which writes build/hparma.log): every instantiation of the parent beside the single-stream
placement that does its work here, then the batch and ragged placements.  VGPRs, AGPRs, spills, scratch, occupancy and static
LDS of the former must be the parent's; the new ones must have no VGPR spills, no scratch and three waves per SIMD.  SGPRs are
printed with their difference (the kernel keeps more scalars than there are SGPRs in every form, the parent's too: "SGPRspill" are
scalars parked in VGPR lanes, not in memory -- scratch stays 0).
    python tools/hparma_batch_resources.py <the parent's hparma.log> [this tree's, default glfer_amd/csrc/build/hparma.log]"""
import os, re, subprocess, sys

root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = [("VGPR", "VGPRs"), ("AGPR", "AGPRs"), ("spill", "VGPRs Spill"), ("SGPR", "TotalSGPRs"), ("SGPRspill", "SGPRs Spill"),
          ("scratch", r"ScratchSize \[bytes/lane\]"), ("occ", r"Occupancy \[waves/SIMD\]"), ("LDS", r"LDS Size \[bytes/block\]")]
SGPR = 3
PLACES = {"0": "One", "1": "Batch", "2": "Ragged"}                  # enum class HpPlace


def short(s):
    s = s.replace("void ", "").replace("glfer::", "")
    s = s[:s.rindex(">(") + 1] if ">(" in s else s.split("(")[0]    # without the argument list
    return re.sub(r"\(HpPlace\)(\d)", lambda m: PLACES[m.group(1)], s)


def read(path):
    out, names = {}, []
    for b in open(path).read().split("Function Name: ")[1:]:
        names.append(b.split(" ")[0])
        out[names[-1]] = tuple(int(re.search(k + r": (\d+)", b).group(1)) for _, k in FIELDS)
    dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    return {short(d): out[n] for n, d in zip(names, dem)}


def fmt(r):
    return " ".join("%s %d" % (f[0], v) for f, v in zip(FIELDS, r))


def here(name):
    """the instantiation of this tree that does the work of the parent's `name`"""
    m = re.match(r"hparma_kernel<(\d+), (\d+), (\d+), (\d+)>$", name)
    return "hparma_kernel<%s, %s, %s, %s, One>" % m.groups() if m else name


old = read(sys.argv[1])
new = read(sys.argv[2] if len(sys.argv) > 2 else os.path.join(root, "glfer_amd", "csrc", "build", "hparma.log"))
pairs = [(n, here(n)) for n in sorted(old)]
missing = [(n, h) for n, h in pairs if h not in new]
fixed = lambda r: r[:SGPR] + r[SGPR + 1:]
moved = [(n, h) for n, h in pairs if h in new and fixed(old[n]) != fixed(new[h])]
sgpr = [(n, h) for n, h in pairs if h in new and old[n][SGPR] != new[h][SGPR]]
fresh = sorted(set(new) - {h for _, h in pairs})
names = [f[0] for f in FIELDS]
bad = [n for n in fresh if new[n][names.index("spill")] or new[n][names.index("scratch")] or new[n][names.index("occ")] != 3]
print("instantiations in the parent: %d, without a counterpart here: %d, new here: %d" % (len(old), len(missing), len(fresh)))
print("VGPR / AGPR / spill / SGPR spill / scratch / occupancy / LDS differ from the parent's: %d; SGPR counts differ: %d" % (len(moved), len(sgpr)))
print("new instantiations with VGPR spills, scratch or an occupancy other than 3 waves per SIMD: %d" % len(bad))
for n, h in pairs:
    print("  %-40s %s" % (n, fmt(old[n])))
    if h not in new:
        print("    MISSING %s" % h)
        continue
    mark = ("   <-- DIFFERS" if (n, h) in moved else "") + ("   (SGPR %+d)" % (new[h][SGPR] - old[n][SGPR]) if (n, h) in sgpr else "")
    print("    %-38s %s%s" % ("= " + h if h != n else "  here", fmt(new[h]), mark))
for n in fresh:
    print("  NEW %-36s %s%s" % (n, fmt(new[n]), "   <-- BAD" if n in bad else ""))
sys.exit(1 if missing or moved or bad else 0)
