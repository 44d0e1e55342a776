"""The many-streams moving average without a GPU: exported, argument errors, a clean failure where no device exists."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("glfer_hip_avg_batch_device", "glfer_hip_spectrogram_avg_batch_device")


def test_avg_batch_entries_exported(lib):
    L = lib.api.lib()
    for name in ENTRIES:
        assert hasattr(L, name), name
        assert name in lib.api.EXPORTS, name
    assert callable(getattr(lib.Spectrogram, "run_avg_batch", None))
    assert callable(getattr(lib, "update_avg_batch", None))


def test_avg_batch_null_plan_and_buffers(lib):
    L = lib.api.lib()
    assert L.glfer_hip_spectrogram_avg_batch_device(None, None, 3, 4096, 4096, 0, 1, 2, 4, 0, 2049, 0, 2049,
                                                    None, None, None, None) == -1               # GLFER_E_ARG
    assert L.glfer_hip_spectrogram_avg_batch_device(None, None, 0, 0, 0, 0, 0, 2, 4, 0, 2049, 0, 2049, None, None, None, None) == -1
    # glfer_hip_avg_batch_device: a bad mode, depth or band, and NULL buffers with streams to average
    assert L.glfer_hip_avg_batch_device(0, None, 3, 4, 129, 129, 4, 0, 129, 0, None, None, None) == -1
    assert L.glfer_hip_avg_batch_device(2, None, 3, 4, 129, 129, 0, 0, 129, 0, None, None, None) == -1
    assert L.glfer_hip_avg_batch_device(2, None, 3, 4, 129, 129, 4, 0, 130, 0, None, None, None) == -1
    assert L.glfer_hip_avg_batch_device(2, None, 3, 4, 129, 129, 4, 0, 129, 0, None, None, None) == -1
    assert L.glfer_hip_avg_batch_device(2, None, 0, 4, 129, 129, 4, 0, 129, 0, None, None, None) == 0   # nothing to do


_NO_DEVICE = r"""
import ctypes as C, sys
sys.path.insert(0, sys.argv[1])
import glfer_amd as G
L = G.api.lib()
cfg = G.api.make_config(G.FftParams(n=1024, window_type=0, overlap=0.5))
h = C.c_void_p()
rc = L.glfer_hip_plan_create(C.byref(cfg), C.byref(h))
print("plan", rc)
print("null", L.glfer_hip_spectrogram_avg_batch_device(None, None, 2, 4096, 4096, 0, 4, 2, 4, 0, 513, 0, 513, None, None, None, None))
if rc == 0:
    print("batch", L.glfer_hip_spectrogram_avg_batch_device(h, None, 2, 4096, 4096, 0, 4, 2, 4, 0, 513, 0, 513, None, None, None, None))
    L.glfer_hip_plan_destroy(h)
"""


def test_avg_batch_without_device_fails_cleanly():
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, "-c", _NO_DEVICE, ROOT], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    out = dict(line.split() for line in r.stdout.splitlines() if line.split() and line.split()[0] in ("plan", "null", "batch"))
    assert int(out["null"]) == -1, r.stdout                      # GLFER_E_ARG, no crash
    if int(out["plan"]) == 0:
        assert int(out["batch"]) == -1, r.stdout
    else:
        assert int(out["plan"]) < 0, r.stdout
