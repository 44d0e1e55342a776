"""The rows-and-F entries without a GPU: exported, argument errors, a clean failure where no device exists, and the reference
alone held to the rules tests/test_gpu_rows_ftest.py uses against it, on every input of tests/_rows_ftest_cases.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

import _ftest_cases as K
import _rows_ftest_cases as R
from _ftest_check import check_ftest
from _rows_check import tau_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("glfer_hip_mtm_rows_ftest_device", "glfer_hip_mtm_rows_ftest_batch_device")


def test_rows_ftest_entries_exported(lib):
    import glfer_amd                                             # (the package imports)
    L = lib.api.lib()
    for name in ENTRIES:
        assert hasattr(L, name), name
        assert name in lib.api.EXPORTS, name
    assert callable(getattr(glfer_amd.Spectrogram, "rows_ftest", None))
    assert callable(getattr(glfer_amd.Spectrogram, "rows_ftest_batch", None))
    assert L.glfer_hip_abi_version() == 5                        # entries added: the ABI number stays


def test_rows_ftest_null_plan(lib):
    L = lib.api.lib()
    assert L.glfer_hip_mtm_rows_ftest_device(None, None, 4096, 0, 1, None, None, 1, None) == -1                  # GLFER_E_ARG
    assert L.glfer_hip_mtm_rows_ftest_device(None, None, 0, 0, 0, None, None, 1, None) == -1                     # before the empty-call shortcut
    assert L.glfer_hip_mtm_rows_ftest_batch_device(None, None, 3, 4096, 4096, 0, 1, None, None, 1, None) == -1
    assert L.glfer_hip_mtm_rows_ftest_batch_device(None, None, 0, 0, 0, 0, 0, None, None, 1, None) == -1


_NO_DEVICE = r"""
import ctypes as C, sys
sys.path.insert(0, sys.argv[1])
import glfer_amd as G
L = G.api.lib()
cfg = G.api.make_config(G.MtmParams(n=1024, overlap=0.5, w=2.5, kmax=4))
h = C.c_void_p()
rc = L.glfer_hip_plan_create(C.byref(cfg), C.byref(h))
print("plan", rc)
# the entries themselves, with no device: a NULL plan, and (where a plan could be made after all) no streams
print("null", L.glfer_hip_mtm_rows_ftest_device(None, None, 4096, 0, 4, None, None, 1, None))
print("nullb", L.glfer_hip_mtm_rows_ftest_batch_device(None, None, 2, 4096, 4096, 0, 4, None, None, 1, None))
if rc == 0:
    print("single", L.glfer_hip_mtm_rows_ftest_device(h, None, 4096, 0, 4, None, None, 1, None))
    print("batch", L.glfer_hip_mtm_rows_ftest_batch_device(h, None, 2, 4096, 4096, 0, 4, None, None, 1, None))
    L.glfer_hip_plan_destroy(h)
"""


def test_rows_ftest_without_device_fails_cleanly():
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, "-c", _NO_DEVICE, ROOT], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    keys = ("plan", "null", "nullb", "single", "batch")
    out = dict(line.split() for line in r.stdout.splitlines() if line.split() and line.split()[0] in keys)
    assert int(out["null"]) == -1 and int(out["nullb"]) == -1, r.stdout      # GLFER_E_ARG, no crash
    if int(out["plan"]) == 0:
        assert int(out["single"]) == -1 and int(out["batch"]) == -1, r.stdout
    else:
        assert int(out["plan"]) < 0, r.stdout


@pytest.mark.parametrize("c", R.ALL_CASES, ids=K.case_id)
def test_reference_stays_within_the_rules(oracle, c):
    """The oracle's F rows by check_ftest against ftest64; its PSD rows of the pair are oracle.spectrogram_mtm's and pass rule
    (3) against themselves; their float64 distance (what rule (3)'s bound is made of) and their tau are printed.  The
    bin-by-bin rule (2) is a device-against-float64 rule and is not asserted for the oracle."""
    r = R.reference(oracle, c)
    rows = r.num / r.den
    rows[:, -1] = np.inf
    frac = check_ftest(rows, r.want_ft, r.num, r.den, c.kmax)
    m = 1 if c.sub_mean else 0
    alone = oracle.spectrogram_mtm(r.xf, c.n, c.ovl, c.nw, c.kmax, sub_mean=m, history_mode=c.history_mode)
    assert np.array_equal(alone.view(np.uint32), r.want_psd.view(np.uint32))
    assert R.check_against_oracle(r.want_psd, r, what=K.case_id(c)) == 0.0
    assert np.isfinite(r.tau) and r.tau > 0 and np.isfinite(r.e_ref)
    print("rows-ftest-criterion %-40s F oracle/float64 %.4f of the bound; psd oracle/float64 %.3e (bound (3) %.3e), oracle tau %.3e, "
          "tau_f32 %.3e, bound (2) %.3e" % (K.case_id(c), frac, r.e_ref, R.oracle_bound(r.e_ref), tau_of(r.want_psd, r.exact),
                                            r.tau_f32, r.tau))
    assert frac <= 1.0
