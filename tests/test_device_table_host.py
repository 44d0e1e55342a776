"""glfer_amd/csrc/device_table.hpp, the owner of a plan-lifetime device table (glfer::DeviceTable<T>), walked without a GPU and
without the HIP runtime: tests/c_device_table.cpp defines the three functions the header calls (hipMalloc, hipMemcpy, hipFree)
over malloc / free with a log and asserts the owner's rules -- every table freed exactly once, by the destructor; nothing kept
after a failed allocation or a failed copy; a second upload frees the first table; a move leaves the source empty; nothing out
at exit.  The program is its own main, run as a plain child process."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP_INCLUDE = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")


def _build(tmp_path, name, *flags):
    exe = tmp_path / name
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-D__HIP_PLATFORM_AMD__", "-I" + HIP_INCLUDE,
                    "-I" + os.path.join(ROOT, "glfer_amd", "csrc"), os.path.join(ROOT, "tests", "c_device_table.cpp"),
                    "-o", str(exe)], check=True)
    return exe


def _run(exe):
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-2000:])
    return r.stdout


def test_the_owner_rules_without_the_hip_runtime(tmp_path):
    exe = _build(tmp_path, "c_device_table")
    out = _run(exe)
    assert out.split()[0] == "tables" and int(out.split()[1]) > 0 and out.split()[2:] == ["failures", "0"]
    # the header alone needs no HIP runtime: the program links none
    ldd = subprocess.run(["ldd", str(exe)], check=True, capture_output=True, text=True).stdout
    assert "amdhip64" not in ldd


def test_the_program_under_address_and_undefined_sanitizers(tmp_path):
    """The same program built with g++'s address and undefined-behaviour sanitizers (the leak check with them): same output,
    no report.  This needs gcc's libasan and libubsan; on a machine without them the test SKIPS -- a sanitizer run is claimed
    only where this test is reported as passed."""
    for lib in ("libasan.so", "libubsan.so"):
        path = subprocess.run(["g++", "-print-file-name=" + lib], check=True, capture_output=True, text=True).stdout.strip()
        if not os.path.isabs(path):
            pytest.skip("g++'s sanitizer runtime is not installed")
    out = _run(_build(tmp_path, "c_device_table_san", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    assert out == _run(_build(tmp_path, "c_device_table_plain"))
