#!/usr/bin/env python3
"""stats_kernels.hip's kernel resources before and after the LMP statistic's stream dimension, from two
-Rpass-analysis=kernel-resource-usage logs of the same compile line (the Makefile's, which this change gives the log; the
parent's source is compiled once more with that line): every instantiation the parent has must keep its figures, and every
new stream-carrying form is shown beside its single-stream twin.
    python tools/lmp_batch_resources.py <the parent's stats_kernels.log> [this tree's, default glfer_amd/csrc/build/stats_kernels.log]"""
import os, re, subprocess, sys

root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = [("VGPR", "VGPRs"), ("AGPR", "AGPRs"), ("spill", "VGPRs Spill"), ("SGPR", "TotalSGPRs"), ("SGPRspill", "SGPRs Spill"),
          ("scratch", r"ScratchSize \[bytes/lane\]"), ("occ", r"Occupancy \[waves/SIMD\]"), ("LDS", r"LDS Size \[bytes/block\]")]


def read(path):
    out, names = {}, []
    for b in open(path).read().split("Function Name: ")[1:]:
        names.append(b.split(" ")[0])
        out[names[-1]] = tuple(int(re.search(k + r": (\d+)", b).group(1)) for _, k in FIELDS)
    dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    short = lambda s: re.sub(r"\(.*\)$", "", s.replace("void ", "").replace("glfer::", ""))
    return {short(d): out[n] for n, d in zip(names, dem)}


def fmt(r):
    return " ".join("%s %d" % (f[0], v) for f, v in zip(FIELDS, r))


def twin(name):
    m = re.match(r"lmp_ring_streams_kernel<(\d+), (\d+), \w+>", name)
    if m:
        return "lmp_ring_kernel<%s, %s>" % m.groups()
    if name.startswith("lmp_ring_any_streams_kernel"):
        return "lmp_ring_any_kernel"
    if name.startswith("lmp_streams_kernel"):
        return "lmp_kernel<0>"
    return None


old = read(sys.argv[1])
new = read(sys.argv[2] if len(sys.argv) > 2 else os.path.join(root, "glfer_amd", "csrc", "build", "stats_kernels.log"))
missing = [n for n in old if n not in new]
changed = [n for n in old if n in new and old[n] != new[n]]
print("instantiations in the parent: %d, missing in this tree: %d, identical VGPR / AGPR / spill / SGPR / SGPR spill / scratch / "
      "occupancy / LDS: %d, changed: %d" % (len(old), len(missing), len(old) - len(missing) - len(changed), len(changed)))
for n in sorted(old):
    print("  %-44s %s%s" % (n, fmt(new.get(n, old[n])), "" if n not in changed else "   <-- parent: " + fmt(old[n])))
for n in missing:
    print("  MISSING %s" % n)
fresh = sorted(n for n in new if n not in old)
print("new instantiations: %d (the third template value: true = ragged, false = batch)" % len(fresh))
for n in fresh:
    t = twin(n)
    tw = new.get(t) if t else None
    print("  %-44s %s\n  %-44s %s" % (n, fmt(new[n]), "    twin " + (t or "-"), fmt(tw) if tw else "-"))
