"""The ragged-batch entries without a GPU: exported, argument errors, the row counts of glfer_hip_ragged_frames, a clean
failure where no device exists."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ragged_entries_exported(lib):
    L = lib.api.lib()
    for name in ("glfer_hip_spectrogram_ragged_device", "glfer_hip_ragged_frames"):
        assert hasattr(L, name), name
        assert name in lib.api.EXPORTS, name
    assert callable(getattr(lib.Spectrogram, "run_ragged", None))
    assert callable(getattr(lib.Spectrogram, "run_list", None))


def test_ragged_null_plan(lib):
    L = lib.api.lib()
    offs = (C.c_size_t * 2)(0, 4096)
    lens = (C.c_size_t * 2)(4096, 4096)
    assert L.glfer_hip_spectrogram_ragged_device(None, None, 2, offs, lens, None, None, None) == -1   # GLFER_E_ARG
    assert L.glfer_hip_spectrogram_ragged_device(None, None, 0, None, None, None, None, None) == -1
    assert L.glfer_hip_ragged_frames(None, 2, lens, None) == 0


def _plan(lib, **k):
    """A plan where one can be made (a plan needs a device for its tables), else None."""
    L = lib.api.lib()
    cfg = lib.api.make_config(lib.FftParams(**dict(dict(n=1024, window_type=0, overlap=0.5), **k)))
    h = C.c_void_p()
    return h if L.glfer_hip_plan_create(C.byref(cfg), C.byref(h)) == 0 else None


def test_ragged_frames_counts(lib):
    """(the same checks run in tests/test_gpu_ragged.py::test_ragged_frames_and_argument_checks, where a plan always exists)"""
    L = lib.api.lib()
    h = _plan(lib)
    if h is None:
        pytest.skip("a plan needs a device for its tables: none here")
    try:
        hop = L.glfer_hip_hop(h)
        lens = np.array([0, hop - 1, hop, hop + 1, 7 * hop + hop // 2, 0, 40 * hop], np.uint64)
        starts = np.full(lens.size + 1, 2 ** 63, np.uint64)
        total = L.glfer_hip_ragged_frames(h, lens.size, lens.ctypes.data, starts.ctypes.data)
        frames = lens // np.uint64(hop)
        assert list(frames[:4]) == [0, 0, 1, 1]
        assert total == int(frames.sum())
        assert list(starts) == [0] + list(np.cumsum(frames))
        assert L.glfer_hip_ragged_frames(h, lens.size, lens.ctypes.data, None) == total      # row_starts is optional
        assert L.glfer_hip_ragged_frames(h, 0, None, None) == 0
        # the entry's own argument checks need no samples: NULL arrays, NULL d_psd with frames, too many frames, no frames
        offs = np.zeros(lens.size, np.uint64)
        assert L.glfer_hip_spectrogram_ragged_device(h, None, lens.size, None, lens.ctypes.data, None, None, None) == -1
        assert L.glfer_hip_spectrogram_ragged_device(h, None, lens.size, offs.ctypes.data, None, None, None, None) == -1
        assert L.glfer_hip_spectrogram_ragged_device(h, None, lens.size, offs.ctypes.data, lens.ctypes.data, None, None, None) == -1
        big = np.array([hop, hop * 2 ** 31], np.uint64)
        assert L.glfer_hip_spectrogram_ragged_device(h, None, 2, offs.ctypes.data, big.ctypes.data, None, None, None) == -1
        none = np.array([hop - 1, 0, 3], np.uint64)
        st = np.full(4, 9, np.uint64)
        assert L.glfer_hip_spectrogram_ragged_device(h, None, 3, offs.ctypes.data, none.ctypes.data, None, st.ctypes.data, None) == 0
        assert list(st) == [0, 0, 0, 0]
        assert L.glfer_hip_spectrogram_ragged_device(h, None, 0, None, None, None, None, None) == 0
    finally:
        L.glfer_hip_plan_destroy(h)


_NO_DEVICE = r"""
import ctypes as C, sys
sys.path.insert(0, sys.argv[1])
import glfer_amd as G
L = G.api.lib()
cfg = G.api.make_config(G.FftParams(n=1024, window_type=0, overlap=0.5))
h = C.c_void_p()
rc = L.glfer_hip_plan_create(C.byref(cfg), C.byref(h))
print("plan", rc)
offs = (C.c_size_t * 2)(0, 8192)
lens = (C.c_size_t * 2)(4096, 6000)
# the ragged entry itself, with no device: a NULL plan, and (where a plan could be made after all) no samples
print("null", L.glfer_hip_spectrogram_ragged_device(None, None, 2, offs, lens, None, None, None))
if rc == 0:
    print("ragged", L.glfer_hip_spectrogram_ragged_device(h, None, 2, offs, lens, None, None, None))
    L.glfer_hip_plan_destroy(h)
"""


def test_ragged_without_device_fails_cleanly():
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, "-c", _NO_DEVICE, ROOT], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    out = dict(line.split() for line in r.stdout.splitlines() if line.split() and line.split()[0] in ("plan", "null", "ragged"))
    assert int(out["null"]) == -1, r.stdout                      # GLFER_E_ARG, no crash
    if int(out["plan"]) == 0:
        assert int(out["ragged"]) == -1, r.stdout
    else:
        assert int(out["plan"]) < 0, r.stdout
