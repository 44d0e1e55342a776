#!/usr/bin/env python3
"""Compare the device code of two builds of glfer_amd/csrc, kernel by kernel.

    python tools/device_code_identity.py <parent build dir> [this build dir]

For every object (*.o) of either build directory: the gfx950 code object is taken out of the object's .hip_fatbin section,
and its kernels are compared BY NAME (their order inside an object is free) in three ways --

  names      the set of kernels (the .kd descriptors of the code object) and, where the build kept a log, the
             "Function Name" lines of -Rpass-analysis=kernel-resource-usage: no instantiation gained or lost
  resources  every kernel's resource-usage block of that log (registers, spills, scratch, occupancy, LDS), as text
  code       every function's disassembly (llvm-objdump -d --no-show-raw-insn --no-leading-addr, split by symbol), as
             text; the padding line "..." that may follow the last function of a section is not part of any function

A diff of two builds: it prints the counts per object and every name that differs, and exits 1 if anything does.
Host-only objects (no .hip_fatbin section) are listed as such.  The default for the second directory is this tree's
glfer_amd/csrc/build."""
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("GLFER_LLVM_BIN", "/opt/rocm/llvm/bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--" + os.environ.get("GLFER_ARCH", "gfx950")


def tool(name):
    p = os.path.join(LLVM, name)
    return p if os.path.exists(p) else name


def code_object(obj, tmp):
    """the object's device code object (a path under tmp), or None for a host-only object"""
    fat = os.path.join(tmp, "fatbin")
    out = os.path.join(tmp, "device.co")
    for f in (fat, out):
        if os.path.exists(f):
            os.remove(f)
    subprocess.run([tool("llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, obj, os.devnull],
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    if not os.path.exists(fat) or os.path.getsize(fat) == 0:
        return None
    subprocess.run([tool("clang-offload-bundler"), "--unbundle", "--type=o", "--targets=" + TARGET,
                    "--input=" + fat, "--output=" + out], check=True)
    return out if os.path.getsize(out) else None


def functions(co):
    """{symbol: disassembly text} of a code object's .text, and the set of its kernels (symbols with a .kd descriptor)"""
    syms = subprocess.run([tool("llvm-objdump"), "-t", co], check=True, capture_output=True, text=True).stdout
    kernels = {ln.split()[-1][:-3] for ln in syms.splitlines() if ln.endswith(".kd")}
    dis = subprocess.run([tool("llvm-objdump"), "-d", "--no-show-raw-insn", "--no-leading-addr", co],
                         check=True, capture_output=True, text=True).stdout
    funcs, name = {}, None
    for ln in dis.splitlines():
        m = re.match(r"^(?:[0-9a-f]+ )?<([^>]+)>:$", ln)
        if m:
            name = m.group(1)
            funcs[name] = []
        elif name is not None and ln.strip() and ln.strip() != "...":
            if ln.startswith("Disassembly of section"):
                name = None
            else:
                # (this objdump still appends "// <address>: <encoding>" to an instruction: the address is the function's place
                # in the object, which is free; the encoding words and a branch's <symbol+offset> stay in the comparison)
                funcs[name].append(re.sub(r"(//) [0-9A-Fa-f]+:", r"\1", ln.rstrip()))
    return {k: "\n".join(v) for k, v in funcs.items()}, kernels


def resource_blocks(log):
    """{kernel: its resource-usage block} from a -Rpass-analysis=kernel-resource-usage log (source positions dropped)"""
    blocks, name = {}, None
    if not os.path.exists(log):
        return None
    for ln in open(log, errors="replace"):
        m = re.search(r"remark: (.*) \[-Rpass-analysis=kernel-resource-usage\]", ln)
        if not m:
            continue
        body = m.group(1).strip()
        f = re.match(r"Function Name: (\S+)", body)
        if f:
            name = f.group(1)
            blocks[name] = []
        elif name is not None:
            blocks[name].append(body)
    return {k: "\n".join(v) for k, v in blocks.items()}


def describe(build, obj, tmp):
    co = code_object(os.path.join(build, obj), tmp)
    if co is None:
        return None
    funcs, kernels = functions(co)
    return funcs, kernels, resource_blocks(os.path.join(build, obj[:-2] + ".log"))


def main():
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    here = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "glfer_amd", "csrc", "build")
    a_dir, b_dir = sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else here
    objs_a = {f for f in os.listdir(a_dir) if f.endswith(".o")}
    objs_b = {f for f in os.listdir(b_dir) if f.endswith(".o")}
    bad = 0
    for f in sorted(objs_a ^ objs_b):
        print("DIFFERENT object set: %s only in %s" % (f, a_dir if f in objs_a else b_dir))
        bad += 1
    tot_k = tot_f = 0
    with tempfile.TemporaryDirectory() as tmp:
        for obj in sorted(objs_a & objs_b):
            a, b = describe(a_dir, obj, tmp), describe(b_dir, obj, tmp)
            if a is None or b is None:
                if (a is None) != (b is None):
                    print("DIFFERENT %s: device code in one build only" % obj)
                    bad += 1
                else:
                    print("%-28s host only" % obj)
                continue
            (fa, ka, ra), (fb, kb, rb) = a, b
            diffs = []
            for n in sorted(ka ^ kb):
                diffs.append("kernel only in %s: %s" % ("parent" if n in ka else "this", n))
            for n in sorted(set(fa) ^ set(fb)):
                if n not in ka ^ kb:
                    diffs.append("function only in %s: %s" % ("parent" if n in fa else "this", n))
            for n in sorted(set(fa) & set(fb)):
                if fa[n] != fb[n]:
                    diffs.append("disassembly differs: %s" % n)
            res = "no log"
            if ra is not None and rb is not None:
                for n in sorted(set(ra) ^ set(rb)):
                    diffs.append("resource block only in %s: %s" % ("parent" if n in ra else "this", n))
                for n in sorted(set(ra) & set(rb)):
                    if ra[n] != rb[n]:
                        diffs.append("resource usage differs: %s" % n)
                if set(ra) != ka or set(rb) != kb:
                    diffs.append("the log's kernel names are not the code object's")
                res = "%d resource blocks" % len(rb)
            elif (ra is None) != (rb is None):
                diffs.append("a resource log in one build only")
            tot_k += len(kb)
            tot_f += len(fb)
            print("%-28s %3d kernels, %3d functions, %s: %s" % (obj, len(kb), len(fb), res, "identical" if not diffs else "DIFFERENT"))
            for d in diffs:
                print("    " + d)
            bad += len(diffs)
    print("total: %d objects, %d kernels, %d functions compared; %d differences" % (len(objs_a & objs_b), tot_k, tot_f, bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
