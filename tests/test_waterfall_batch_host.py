"""The many-streams waterfall without a GPU: exported, argument errors, a clean failure where no device exists."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "glfer_hip_waterfall_batch_device"


def test_waterfall_batch_entry_exported(lib):
    L = lib.api.lib()
    assert hasattr(L, ENTRY)
    assert ENTRY in lib.api.EXPORTS
    assert callable(getattr(lib, "waterfall_batch", None))
    assert lib.waterfall_batch is lib.api.waterfall_batch


def test_waterfall_batch_null_and_argument_errors(lib):
    W = getattr(lib.api.lib(), ENTRY)
    arr = (lib.Display * 3)(*[lib.Display() for _ in range(3)])
    # disps NULL with streams, NULL rows / pixels with columns to map
    assert W(None, 3, 0, 1, 0, 1, 0, None, 10, 129, None, None, None, None) == -1               # GLFER_E_ARG
    assert W(arr, 3, 0, 1, 0, 1, 0, None, 10, 129, None, None, None, None) == -1
    # options that differ between entries: refused, no state changed
    arr[1].palette = 3
    arr[2].first_buffer = 0
    arr[2].display_max_lvl = 1.5
    assert W(arr, 3, 0, 1, 0, 1, 0, None, 10, 129, None, None, None, None) == -1
    assert (arr[2].first_buffer, arr[2].display_max_lvl, arr[0].first_buffer) == (0, 1.5, 1)
    arr[1].palette = 0
    # waterfall_device's rules: bins, mode, depth, band, pitch below bins, scale type
    assert W(arr, 3, 0, 1, 0, 1, 0, None, 10, 0, None, None, None, None) == -1
    assert W(arr, 3, 0, 1, 0, 1, 0, None, 10, 40000, None, None, None, None) == -1
    assert W(arr, 3, 5, 4, 0, 129, 0, None, 10, 129, None, None, None, None) == -1
    assert W(arr, 3, 2, 0, 0, 129, 0, None, 10, 129, None, None, None, None) == -1
    assert W(arr, 3, 2, 4, 0, 130, 0, None, 10, 129, None, None, None, None) == -1
    for d in arr:
        d.psd_pitch = 100
    assert W(arr, 3, 0, 1, 0, 1, 0, None, 10, 129, None, None, None, None) == -1
    for d in arr:
        d.psd_pitch = 0
        d.scale_type = 7
    assert W(arr, 3, 0, 1, 0, 1, 0, None, 10, 129, None, None, None, None) == -1
    # nothing to do
    assert W(None, 0, 0, 1, 0, 1, 0, None, 10, 129, None, None, None, None) == 0
    assert W(arr, 3, 0, 1, 0, 1, 0, None, 0, 129, None, None, None, None) == 0
    assert (arr[2].first_buffer, arr[2].display_max_lvl, arr[0].first_buffer) == (0, 1.5, 1)


_NO_DEVICE = r"""
import ctypes as C, sys
sys.path.insert(0, sys.argv[1])
import glfer_amd as G
L = G.api.lib()
arr = (G.Display * 2)(G.Display(), G.Display())
print("null", L.glfer_hip_waterfall_batch_device(None, 2, 0, 1, 0, 1, 0, None, 4, 129, None, None, None, None))
cfg = G.api.make_config(G.FftParams(n=1024, window_type=0, overlap=0.5))
h = C.c_void_p()
rc = L.glfer_hip_plan_create(C.byref(cfg), C.byref(h))
print("plan", rc)
if rc != 0:    # no device: a call that passes every argument rule fails at the device, and changes nothing
    print("bad", L.glfer_hip_waterfall_batch_device(arr, 2, 0, 1, 0, 1, 0, C.c_void_p(4096), 4, 129, C.c_void_p(8192), None, None, None))
else:
    L.glfer_hip_plan_destroy(h)
print("state", arr[0].first_buffer, arr[1].first_buffer)
"""


def test_waterfall_batch_without_device_fails_cleanly():
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, "-c", _NO_DEVICE, ROOT], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    out = {line.split()[0]: line.split()[1:] for line in r.stdout.splitlines() if line.split()}
    assert int(out["null"][0]) == -1, r.stdout                  # GLFER_E_ARG, no crash
    if int(out["plan"][0]) != 0:
        assert int(out["bad"][0]) < 0, r.stdout                 # no device: an error, not a crash or a fall-back
    assert out["state"] == ["1", "1"], r.stdout                 # and no state changed
