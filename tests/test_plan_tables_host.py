"""glfer_amd/csrc/plan_tables.cpp, the host half of a plan, without a GPU and without the HIP runtime: tests/c_plan_tables.cpp
builds every table of a grid of configurations (the smallest size that reaches each branch of the builders, both sides of every
gate) through the named builders and prints, per table, the configuration, the name, the length and a 64-bit FNV-1a hash of the
bytes.  tests/golden/plan_tables.txt holds the same lines as glfer_hip_plan_create and ftest_tables computed them inline, before
the builders had names.  Equality line by line: no tolerance is involved.  The program is its own main, run as a plain child
process."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "glfer_amd", "csrc")
HIP_INCLUDE = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")


def _golden():
    with open(os.path.join(ROOT, "tests", "golden", "plan_tables.txt")) as f:
        return f.read().splitlines()


def _build(tmp_path, name, *flags):
    exe = tmp_path / name
    # host_tables.o's flags; the argument-block headers the builders read their constants from include the HIP runtime's header
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", *flags, "-D__HIP_PLATFORM_AMD__",
                    "-I" + HIP_INCLUDE, "-I" + CSRC, os.path.join(ROOT, "tests", "c_plan_tables.cpp"),
                    os.path.join(CSRC, "plan_tables.cpp"), os.path.join(CSRC, "host_tables.cpp"), "-o", str(exe), "-lpthread"],
                   check=True)
    return exe


def _run(exe):
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stdout[-500:], r.stderr[-2000:])
    return r.stdout.splitlines()


def _same(got, want):
    assert len(got) == len(want), (len(got), len(want))
    for g, w in zip(got, want):
        assert g == w


def test_every_table_is_the_one_the_plan_built_inline(tmp_path):
    exe = _build(tmp_path, "c_plan_tables")
    _same(_run(exe), _golden())
    # the builders need no HIP runtime: the program links none
    ldd = subprocess.run(["ldd", str(exe)], check=True, capture_output=True, text=True).stdout
    assert "amdhip64" not in ldd


def test_the_grid_reaches_every_table_and_both_sides_of_every_gate():
    """Read from the fixture: every table is present in some configuration and absent in another; the F tables are there."""
    present, absent, names = set(), set(), set()
    for line in _golden():
        part = line.split()
        if part[2] == "=":
            continue
        names.add(part[1])
        (present if int(part[2]) > 0 else absent).add(part[1])
    always = {"window", "taps", "tw"} | {"U0", "hn", "ftaps", "cj", "ftaps2"}    # (a plan always has the first three)
    assert names == present and names - always == absent - always
    assert {"htaps", "htw", "hrot", "wtaps", "wtw", "wcomb", "bigtw", "xtaps", "ytaps", "ltaps", "iqtaps", "ataps", "lagmap",
            "rot_sched", "unit", "tapers", "sig"} <= absent
    assert always <= present


def test_the_program_under_address_and_undefined_sanitizers(tmp_path):
    """The same program built with g++'s address and undefined-behaviour sanitizers: same lines, no report.  This needs gcc's
    libasan and libubsan; on a machine without them the test SKIPS -- a sanitizer run is claimed only where this test is
    reported as passed."""
    for lib in ("libasan.so", "libubsan.so"):
        path = subprocess.run(["g++", "-print-file-name=" + lib], check=True, capture_output=True, text=True).stdout.strip()
        if not os.path.isabs(path):
            pytest.skip("g++'s sanitizer runtime is not installed")
    _same(_run(_build(tmp_path, "c_plan_tables_san", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")), _golden())
