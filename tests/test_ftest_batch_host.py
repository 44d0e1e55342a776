"""The many-streams F-test entry without a GPU: exported, argument errors, a clean failure where no device exists."""
import os
import subprocess
import sys

import numpy as np
import pytest

import _ftest_batch_cases as B
import _ftest_cases as K
from _ftest_check import check_ftest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ftest_batch_entry_exported(lib):
    L = lib.api.lib()
    assert hasattr(L, "glfer_hip_mtm_ftest_batch_device")
    assert "glfer_hip_mtm_ftest_batch_device" in lib.api.EXPORTS
    assert callable(getattr(lib.Spectrogram, "ftest_batch", None))
    assert L.glfer_hip_abi_version() == 5                        # an entry added: the ABI number stays


def test_ftest_batch_null_plan(lib):
    L = lib.api.lib()
    assert L.glfer_hip_mtm_ftest_batch_device(None, None, 3, 4096, 4096, 0, 1, None, 1, None) == -1   # GLFER_E_ARG
    assert L.glfer_hip_mtm_ftest_batch_device(None, None, 0, 0, 0, 0, 0, None, 1, None) == -1         # before the empty-call shortcut


_NO_DEVICE = r"""
import ctypes as C, sys
sys.path.insert(0, sys.argv[1])
import glfer_amd as G
L = G.api.lib()
cfg = G.api.make_config(G.MtmParams(n=1024, overlap=0.5, w=2.5, kmax=4))
h = C.c_void_p()
rc = L.glfer_hip_plan_create(C.byref(cfg), C.byref(h))
print("plan", rc)
# the batch entry itself, with no device: a NULL plan, and (where a plan could be made after all) no streams
print("null", L.glfer_hip_mtm_ftest_batch_device(None, None, 2, 4096, 4096, 0, 4, None, 1, None))
if rc == 0:
    print("batch", L.glfer_hip_mtm_ftest_batch_device(h, None, 2, 4096, 4096, 0, 4, None, 1, None))
    L.glfer_hip_plan_destroy(h)
"""


def test_ftest_batch_without_device_fails_cleanly():
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, "-c", _NO_DEVICE, ROOT], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    out = dict(line.split() for line in r.stdout.splitlines() if line.split() and line.split()[0] in ("plan", "null", "batch"))
    assert int(out["null"]) == -1, r.stdout                      # GLFER_E_ARG, no crash
    if int(out["plan"]) == 0:
        assert int(out["batch"]) == -1, r.stdout
    else:
        assert int(out["plan"]) < 0, r.stdout


@pytest.mark.parametrize("c,b", [pytest.param(c, b, id="%s-stream%d" % (K.case_id(c), b))
                                 for c in B.PARITY_CASES for b in range(B.NSTREAMS)])
def test_reference_passes_the_rule_on_every_parity_stream(oracle, c, b):
    """The batch's oracle parity (tests/test_gpu_ftest_batch.py) varies seed, amplitude and DC level per stream: the reference
    alone, against float64 arithmetic, by the rule and at the TOL the device's rows are then held to."""
    _, want, num, den = B.reference(oracle, c, b)
    rows = num / den
    rows[:, -1] = np.inf
    frac = check_ftest(rows, want, num, den, c.kmax)
    print("ftest-batch-criterion %s stream %d oracle/float64 %.4f of the bound" % (K.case_id(c), b, frac))
    assert frac <= 1.0
