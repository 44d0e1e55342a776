"""glfer_amd/csrc/scratch.hpp, the owner of a per-call scratch buffer (glfer::Scratch<T>), walked without a GPU and without the
HIP runtime: tests/c_scratch_guard.cpp defines the three functions the header calls (glfer::scratch_malloc, glfer::scratch_free,
hipMemcpyAsync) over malloc / free with a log of (pointer, stream, order) and asserts the owner's rules -- one give-back, on the
guard's stream, at scope exit and at an early return; nothing kept after a failed take or a failed copy; release() idempotent;
a second take gives the first buffer back; a moved-from guard gives nothing back; reverse order of declaration; nothing out at
exit.  The program is its own main, run as a plain child process."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP_INCLUDE = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")


def _build(tmp_path, name, *flags):
    exe = tmp_path / name
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-D__HIP_PLATFORM_AMD__", "-I" + HIP_INCLUDE,
                    "-I" + os.path.join(ROOT, "glfer_amd", "csrc"), os.path.join(ROOT, "tests", "c_scratch_guard.cpp"),
                    "-o", str(exe)], check=True)
    return exe


def _run(exe):
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-2000:])
    return r.stdout


def test_the_guard_rules_without_the_hip_runtime(tmp_path):
    exe = _build(tmp_path, "c_scratch_guard")
    out = _run(exe)
    assert out.split()[0] == "events" and int(out.split()[1]) > 0 and out.split()[2:] == ["failures", "0"]
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
    out = _run(_build(tmp_path, "c_scratch_guard_san", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    assert out == _run(_build(tmp_path, "c_scratch_guard_plain"))
