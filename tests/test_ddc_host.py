"""The down-converter's host-only entries without a GPU: exported and listed, the phase word against Python integers, the design
against the numpy float64 formula (symmetry, sum, every tap, defaults), glfer_hip_ddc_tables bit for bit against the restatement
of tests/_ddc_exact.py, glfer_hip_ddc_supported at each edge of its ranges, and the refusals of the device entries that need no
handle.  tests/test_gpu_ddc.py runs device_entry_refusals with real handles."""
import ctypes as C
import os

import numpy as np
import pytest

import _ddc_exact as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, E_ARG = 0, -1
ENTRIES = ("glfer_hip_ddc_phase_word", "glfer_hip_ddc_design", "glfer_hip_ddc_supported", "glfer_hip_ddc_tables", "glfer_hip_ddc_create",
           "glfer_hip_ddc_destroy", "glfer_hip_ddc_device", "glfer_hip_ddc_batch_device", "glfer_hip_spectrogram_zoom_device")


def test_ddc_entries_exported(lib):
    L = lib.api.lib()
    header = open(os.path.join(ROOT, "include", "glfer_hip.h")).read()
    for name in ENTRIES:
        assert hasattr(L, name), name
        assert name in lib.api.EXPORTS, name
        assert name + "(" in header, name
    for name in ("run", "run_batch", "tables", "num_out", "close"):
        assert callable(getattr(lib.Ddc, name, None)), name
    assert callable(getattr(lib.Spectrogram, "run_zoom", None))
    assert L.glfer_hip_abi_version() == 5 and "#define GLFER_HIP_ABI 5" in header


def test_phase_word_matches_python_integers(lib):
    for freq in (0.0, 2.0 ** -64, -2.0 ** -64, 0.25, -0.5, 0.1, 0.1234567, 0.25 + 2.0 ** -40, -0.49, 0.5 - 2.0 ** -54):
        want = round(freq * 2.0 ** 64) % (1 << 64)
        assert lib.ddc_phase_word(freq) == want == X.phase_word(freq), freq
    assert lib.ddc_phase_word(0.0) == 0 and lib.ddc_phase_word(2.0 ** -64) == 1 and lib.ddc_phase_word(-2.0 ** -64) == (1 << 64) - 1
    assert lib.ddc_phase_word(0.25) == 1 << 62 and lib.ddc_phase_word(-0.5) == 1 << 63


def _ulps(a, b):
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    ia = np.where(ia < 0, -(ia & 0x7fffffff), ia)
    ib = np.where(ib < 0, -(ib & 0x7fffffff), ib)
    return np.abs(ia - ib)


@pytest.mark.parametrize("decim,ntaps,cutoff,beta", [(2, 0, 0, 0), (3, 0, 0, 0), (16, 0, 0, 0), (64, 0, 0, 0), (100, 401, 0, 0), (1024, 0, 0, 0),
                                                     (7, 8192, 0, 0), (5, 4, 0, 0), (8, 64, 0.05, 5.0), (1, 33, 0.2, 12.0), (4, 2, 0, 0)])
def test_design(lib, decim, ntaps, cutoff, beta):
    h = lib.ddc_design(decim, ntaps, cutoff, beta)
    T = len(h)
    assert h.dtype == np.float32 and T == (ntaps if ntaps > 0 else (1 if decim == 1 else min(8 * decim + 1, 8192)))
    assert np.array_equal(h.view(np.int32), h[::-1].view(np.int32))                          # exactly symmetric
    assert abs(float(h.astype(np.float64).sum()) - 1.0) <= T * 2.0 ** -24
    ref = X.design64(decim, ntaps, cutoff, beta).astype(np.float32)
    assert _ulps(h, ref).max() <= 1, int(np.argmax(_ulps(h, ref)))


def test_design_defaults_and_refusals(lib):
    L = lib.api.lib()
    assert np.array_equal(lib.ddc_design(1), np.ones(1, np.float32))                          # decim 1: the pure mixer
    assert len(lib.ddc_design(64)) == 513 and len(lib.ddc_design(1024)) == 8192 and len(lib.ddc_design(1023)) == 8185
    assert np.array_equal(lib.ddc_design(16), lib.ddc_design(16, 129, 0.4 / 16, 8.0))
    assert np.array_equal(lib.ddc_design(16, -3, -1.0, -2.0), lib.ddc_design(16))
    assert L.glfer_hip_ddc_design(16, 0, 0.0, 0.0, None) == 129                               # the count alone
    for bad in ((0, 0, 0.0, 0.0), (1025, 0, 0.0, 0.0), (-1, 9, 0.0, 0.0), (4, 8193, 0.0, 0.0), (4, 33, 0.6, 0.0)):
        assert L.glfer_hip_ddc_design(*bad, None) == E_ARG, bad


@pytest.mark.parametrize("freq", [0.0, 0.1234567, -0.49, 0.25 + 2.0 ** -40, -0.5, 2.0 ** -64])
@pytest.mark.parametrize("decim,ntaps", [(1, 1), (2, 9), (16, 129), (100, 401), (7, 8192)])
def test_tables_bit_for_bit(lib, decim, ntaps, freq):
    h = lib.ddc_design(decim, ntaps)
    g = lib.ddc_tables(freq, h)
    want = X.tables(X.phase_word(freq), h)
    assert g.dtype == np.complex64 and g.shape == (ntaps,)
    assert np.array_equal(g.view(np.int32), want.view(np.int32))
    if freq == 0.0:
        assert np.array_equal(g.real, h) and not g.imag.any()


def _supported(lib, decim=16, ntaps=129, freq=0.1, complex_in=0, sample_format=0):
    cfg = lib.DdcConfig(decim, ntaps, freq, complex_in, sample_format, 0)
    return lib.api.lib().glfer_hip_ddc_supported(C.byref(cfg))


def test_supported_edges(lib):
    L = lib.api.lib()
    assert L.glfer_hip_ddc_supported(None) == E_ARG
    for decim in (1, 2, 1024):
        for ntaps in (1, 2, 8192):
            assert _supported(lib, decim=decim, ntaps=ntaps) == OK, (decim, ntaps)
    for decim in (0, -1, 1025):
        assert _supported(lib, decim=decim) == E_ARG, decim
    for ntaps in (0, -5, 8193):
        assert _supported(lib, ntaps=ntaps) == E_ARG, ntaps
    for freq in (-0.5, 0.0, np.nextafter(0.5, 0.0)):
        assert _supported(lib, freq=freq) == OK, freq
    for freq in (0.5, np.nextafter(-0.5, -1.0), 1.0, float("nan"), float("inf")):
        assert _supported(lib, freq=freq) == E_ARG, freq
    for fmt in (0, 1, 2):
        for cplx in (0, 1):
            assert _supported(lib, sample_format=fmt, complex_in=cplx) == OK
    for fmt in (-1, 3):
        assert _supported(lib, sample_format=fmt) == E_ARG
    assert _supported(lib, complex_in=2) == E_ARG
    assert lib.ddc_supported(64, 513, 0.1) and not lib.ddc_supported(2048, 513, 0.1)
    h = np.ones(4, np.float32)
    g = np.empty(8, np.float32)
    cfg = lib.DdcConfig(4, 4, 0.5, 0, 0, 0)
    assert L.glfer_hip_ddc_tables(C.byref(cfg), h.ctypes.data, g.ctypes.data) == E_ARG       # an unsupported shape
    cfg = lib.DdcConfig(4, 4, 0.1, 0, 0, 0)
    assert L.glfer_hip_ddc_tables(C.byref(cfg), None, g.ctypes.data) == E_ARG
    assert L.glfer_hip_ddc_tables(C.byref(cfg), h.ctypes.data, None) == E_ARG
    out = C.c_void_p(0x1234)
    assert L.glfer_hip_ddc_create(None, h.ctypes.data, C.byref(out)) == E_ARG and out.value is None
    assert L.glfer_hip_ddc_create(C.byref(cfg), None, C.byref(out)) == E_ARG
    assert L.glfer_hip_ddc_create(C.byref(cfg), h.ctypes.data, None) == E_ARG


def _handle(lib, decim, ntaps, complex_in, fmt):
    """A handle where one can be made (its tables live on a device), else None."""
    L = lib.api.lib()
    cfg = lib.DdcConfig(decim, ntaps, 0.1, complex_in, fmt, 0)
    h = np.ascontiguousarray(lib.ddc_design(decim, ntaps))
    out = C.c_void_p()
    return out if L.glfer_hip_ddc_create(C.byref(cfg), h.ctypes.data, C.byref(out)) == 0 else None


def device_entry_refusals(lib):
    """Every refusal of the DDC device entries that needs a handle, in the documented order; shared with tests/test_gpu_ddc.py.  The
    buffers are fake addresses: a refusal must come before anything reads them or is launched.  Returns the handles it could make."""
    L = lib.api.lib()
    one, many = L.glfer_hip_ddc_device, L.glfer_hip_ddc_batch_device
    fake, out = 0x10000, 0x4000000
    made = 0
    D, T = 16, 129
    for fmt, ssz in ((lib.SAMPLES_F32, 4), (lib.SAMPLES_S16, 2), (lib.SAMPLES_U8, 1)):
        for cplx in (0, 1):
            h = _handle(lib, D, T, cplx, fmt)
            if h is None:
                continue
            made += 1
            try:
                esz, ns = ssz * (2 if cplx else 1), 100 * D + 9
                for pitch in (1, 39):                                                       # out_pitch below nout
                    assert many(h, fake, 2, ns, ns, 0, 40, out, pitch, None) == E_ARG
                    assert many(h, None, 0, ns, ns, 0, 40, None, pitch, None) == E_ARG      # (refused even with no work)
                assert one(h, None, ns, 0, 0, None, None) == OK                             # no outputs, no streams: nothing to do
                assert one(h, None, ns, 10 ** 9, 0, None, None) == OK
                assert many(h, None, 0, ns, ns, 0, 40, None, 0, None) == OK
                assert many(h, None, 3, ns, ns, 0, 0, None, 0, None) == OK
                assert one(h, None, ns, 0, 40, out, None) == E_ARG                          # NULL buffers while there is work
                assert one(h, fake, ns, 0, 40, None, None) == E_ARG
                assert many(h, None, 2, ns, ns, 0, 40, out, 0, None) == E_ARG
                assert one(h, fake, ns, 61, 40, out, None) == E_ARG                         # an output past the stream (100 outputs)
                assert one(h, fake, ns, 100, 1, out, None) == E_ARG
                assert many(h, fake, 2, ns, ns, 99, 2, out, 0, None) == E_ARG
                assert one(h, fake, ns, 2 ** 64 - 2, 4, out, None) == E_ARG                 # first_out + nout wraps
                assert one(h, fake, 2 ** 40 * D, 0, 2 ** 31, out, None) == E_ARG            # nout > 0x7fffffff
                for off in range(1, esz):                                                   # off one input sample
                    assert one(h, fake + off, ns, 0, 40, out, None) == E_ARG
                    assert many(h, fake + off, 2, ns, ns, 0, 40, out, 0, None) == E_ARG
                assert many(h, fake, 2 ** 40, 2 ** 40, ns, 0, 40, out, 0, None) == E_ARG    # sizes that overflow
                assert one(h, fake, 2 ** 63, 0, 40, out, None) == E_ARG
            finally:
                L.glfer_hip_ddc_destroy(h)
    return made


def test_null_handle_and_device_entry_refusals(lib):
    L = lib.api.lib()
    fake = 0x10000
    assert L.glfer_hip_ddc_device(None, fake, 4096, 0, 1, fake, None) == E_ARG
    assert L.glfer_hip_ddc_device(None, None, 0, 0, 0, None, None) == E_ARG
    assert L.glfer_hip_ddc_batch_device(None, fake, 2, 4096, 4096, 0, 1, fake, 0, None) == E_ARG
    assert L.glfer_hip_spectrogram_zoom_device(None, None, fake, 4096, 0, 1, fake, 0, 0, None) == E_ARG
    L.glfer_hip_ddc_destroy(None)                                                            # a no-op
    assert device_entry_refusals(lib) in (0, 6)                                              # (a handle needs a device: 0 without one)
