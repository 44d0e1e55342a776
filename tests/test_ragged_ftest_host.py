"""The ragged F entries without a GPU: exported, their argument rules in the order include/glfer_hip.h states (where a plan
can be made), a clean failure where no device exists."""
import ctypes as C
import os
import subprocess
import sys

import pytest

from _ragged_ftest_cases import ENTRIES, METHODS, argument_rules, call

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ragged_ftest_entries_exported(lib):
    L = lib.api.lib()
    for name in ENTRIES:
        assert hasattr(L, name), name
        assert name in lib.api.EXPORTS, name
    for name in METHODS:
        assert callable(getattr(lib.Spectrogram, name, None)), name
    assert L.glfer_hip_abi_version() == 5                        # entries added: the ABI number stays


def test_ragged_ftest_null_plan(lib):
    L = lib.api.lib()
    offs = (C.c_size_t * 2)(0, 4096)
    lens = (C.c_size_t * 2)(4096, 8192)
    assert L.glfer_hip_mtm_ftest_ragged_device(None, None, 2, offs, lens, None, 1, None, None) == -1         # GLFER_E_ARG
    assert L.glfer_hip_mtm_ftest_ragged_device(None, None, 0, None, None, None, 1, None, None) == -1
    assert L.glfer_hip_mtm_rows_ftest_ragged_device(None, None, 2, offs, lens, None, None, 1, None, None) == -1
    assert L.glfer_hip_mtm_rows_ftest_ragged_device(None, None, 0, None, None, None, None, 0, None, None) == -1


def test_ragged_ftest_argument_order(lib):
    """(the same assertions run in tests/test_gpu_ragged_ftest.py::test_argument_order, where a plan always exists)"""
    L = lib.api.lib()
    made = []

    def plan(params):
        cfg = lib.api.make_config(params)
        h = C.c_void_p()
        if L.glfer_hip_plan_create(C.byref(cfg), C.byref(h)) != 0:
            pytest.skip("a plan needs a device for its tables: none here")
        made.append(h)
        return h

    try:
        argument_rules(lib, plan)
    finally:
        for h in made:
            L.glfer_hip_plan_destroy(h)


_NO_DEVICE = r"""
import ctypes as C, sys
sys.path.insert(0, sys.argv[1])
import glfer_amd as G
L = G.api.lib()
cfg = G.api.make_config(G.MtmParams(n=1024, overlap=0.0, w=2.5, kmax=4))
h = C.c_void_p()
rc = L.glfer_hip_plan_create(C.byref(cfg), C.byref(h))
print("plan", rc)
offs = (C.c_size_t * 2)(0, 8192)
lens = (C.c_size_t * 2)(4096, 6000)
# the entries themselves, with no device: a NULL plan, and (where a plan could be made after all) no samples
print("null_f", L.glfer_hip_mtm_ftest_ragged_device(None, None, 2, offs, lens, None, 1, None, None))
print("null_rf", L.glfer_hip_mtm_rows_ftest_ragged_device(None, None, 2, offs, lens, None, None, 1, None, None))
if rc == 0:
    print("f", L.glfer_hip_mtm_ftest_ragged_device(h, None, 2, offs, lens, None, 1, None, None))
    print("rf", L.glfer_hip_mtm_rows_ftest_ragged_device(h, None, 2, offs, lens, None, None, 1, None, None))
    L.glfer_hip_plan_destroy(h)
"""


def test_ragged_ftest_without_device_fails_cleanly():
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, "-c", _NO_DEVICE, ROOT], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    keys = ("plan", "null_f", "null_rf", "f", "rf")
    out = dict(line.split() for line in r.stdout.splitlines() if line.split() and line.split()[0] in keys)
    assert int(out["null_f"]) == -1 and int(out["null_rf"]) == -1, r.stdout      # GLFER_E_ARG, no crash
    if int(out["plan"]) == 0:
        assert int(out["f"]) < 0 and int(out["rf"]) < 0, r.stdout
    else:
        assert int(out["plan"]) < 0, r.stdout
