#!/usr/bin/env python3
"""stats_kernels.hip's kernel resources in the parent and in this tree, from two -Rpass-analysis=kernel-resource-usage logs of
the same compile line (the Makefile's, which writes build/stats_kernels.log): every instantiation of the parent is shown
beside the one that does its work here.  A parent that still has the stream-carrying siblings (lmp_*_streams_kernel) is mapped
onto the placement parameter of the three LMP kernels; any other name maps onto itself, so the tool also compares two trees
with the same kernels.  VGPRs, AGPRs, spills, scratch, occupancy and static LDS must be the parent's; SGPRs are printed with
their difference.
    python tools/lmp_batch_resources.py <the parent's stats_kernels.log> [this tree's, default glfer_amd/csrc/build/stats_kernels.log]"""
import os, re, subprocess, sys

root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = [("VGPR", "VGPRs"), ("AGPR", "AGPRs"), ("spill", "VGPRs Spill"), ("SGPR", "TotalSGPRs"), ("SGPRspill", "SGPRs Spill"),
          ("scratch", r"ScratchSize \[bytes/lane\]"), ("occ", r"Occupancy \[waves/SIMD\]"), ("LDS", r"LDS Size \[bytes/block\]")]
SGPR = 3
PLACES = {"0": "One", "1": "Batch", "2": "Ragged"}                  # enum class LmpPlace


def short(s):
    s = s.replace("void ", "").replace("glfer::", "")
    s = s[:s.rindex(">(") + 1] if ">(" in s else s.split("(")[0]    # without the argument list
    return re.sub(r"\(LmpPlace\)(\d)", lambda m: PLACES[m.group(1)], s)


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
    place = lambda b: "Ragged" if b == "true" else "Batch"
    for pat, to in ((r"lmp_ring_streams_kernel<(\d+), (\d+), (\w+)>$", lambda m: "lmp_ring_kernel<%s, %s, %s>" % (m[1], m[2], place(m[3]))),
                    (r"lmp_ring_any_streams_kernel<(\w+)>$", lambda m: "lmp_ring_any_kernel<%s>" % place(m[1])),
                    (r"lmp_streams_kernel<(\w+)>$", lambda m: "lmp_kernel<0, %s>" % place(m[1])),
                    (r"lmp_ring_kernel<(\d+), (\d+)>$", lambda m: "lmp_ring_kernel<%s, %s, One>" % (m[1], m[2])),
                    (r"lmp_ring_any_kernel$", lambda m: "lmp_ring_any_kernel<One>"),
                    (r"lmp_kernel<(\d+)>$", lambda m: "lmp_kernel<%s, One>" % m[1])):
        m = re.match(pat, name)
        if m:
            return to(m)
    return name


old = read(sys.argv[1])
new = read(sys.argv[2] if len(sys.argv) > 2 else os.path.join(root, "glfer_amd", "csrc", "build", "stats_kernels.log"))
pairs = [(n, here(n)) for n in sorted(old)]
missing = [(n, h) for n, h in pairs if h not in new]
fixed = lambda r: r[:SGPR] + r[SGPR + 1:]
moved = [(n, h) for n, h in pairs if h in new and fixed(old[n]) != fixed(new[h])]
sgpr = [(n, h) for n, h in pairs if h in new and old[n][SGPR] != new[h][SGPR]]
fresh = sorted(set(new) - {h for _, h in pairs})
print("instantiations in the parent: %d, without a counterpart here: %d, here without one in the parent: %d" % (len(old), len(missing), len(fresh)))
print("VGPR / AGPR / spill / SGPR spill / scratch / occupancy / LDS differ from the parent's: %d; SGPR counts differ: %d" % (len(moved), len(sgpr)))
for n, h in pairs:
    print("  %-40s %s" % (n, fmt(old[n])))
    if h not in new:
        print("    MISSING %s" % h)
        continue
    mark = ("   <-- DIFFERS" if (n, h) in moved else "") + ("   (SGPR %+d)" % (new[h][SGPR] - old[n][SGPR]) if (n, h) in sgpr else "")
    print("    %-38s %s%s" % ("= " + h if h != n else "  here", fmt(new[h]), mark))
for n in fresh:
    print("  NEW %-36s %s" % (n, fmt(new[n])))
sys.exit(1 if missing or moved or fresh else 0)
