"""The complex I/Q entries without a GPU: exported and listed, the ABI number, glfer_hip_iq_supported over sizes, modes and options,
glfer_hip_iq_tables against numpy, and every refusal of the two device entries (the ones that need a plan: where a plan can be made;
tests/test_gpu_iq.py runs the same helper where one always can)."""
import ctypes as C
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, E_ARG = 0, -1
ENTRIES = ("glfer_hip_iq_supported", "glfer_hip_iq_tables", "glfer_hip_spectrogram_iq_device", "glfer_hip_spectrogram_iq_batch_device")
SIZES = (256, 512, 1024, 2048, 4096, 8192, 16384)


def test_iq_entries_exported(lib):
    L = lib.api.lib()
    for name in ENTRIES:
        assert hasattr(L, name), name
        assert name in lib.api.EXPORTS, name
    for name in ("run_iq", "run_iq_batch"):
        assert callable(getattr(lib.Spectrogram, name, None)), name
    assert callable(lib.iq_supported) and callable(lib.iq_tables)
    assert (lib.IQ_CENTERED, lib.IQ_SWAP) == (1, 2)
    assert L.glfer_hip_abi_version() == 5
    header = open(os.path.join(ROOT, "include", "glfer_hip.h")).read()
    assert "#define GLFER_HIP_ABI 5" in header
    assert "#define GLFER_IQ_CENTERED 1u" in header and "#define GLFER_IQ_SWAP     2u" in header
    for name in ENTRIES:
        assert name + "(" in header, name


def _supported(lib, params):
    cfg = lib.api.make_config(params)
    return lib.api.lib().glfer_hip_iq_supported(C.byref(cfg))


def test_iq_supported(lib):
    L = lib.api.lib()
    assert L.glfer_hip_iq_supported(None) == E_ARG
    for n in SIZES:
        assert _supported(lib, lib.FftParams(n=n, window_type=0, overlap=0.5)) == OK, n
        assert _supported(lib, lib.MtmParams(n=n, overlap=0.0, w=2.5, kmax=4)) == OK, n
    for fmt in (lib.SAMPLES_F32, lib.SAMPLES_S16, lib.SAMPLES_U8):
        for hist in (lib.HISTORY_ZERO_FIRST, lib.HISTORY_ZERO_ALWAYS):
            assert _supported(lib, lib.FftParams(n=1024, window_type=5, overlap=0.3, sample_format=fmt, history_mode=hist)) == OK
    for n in (128, 32768, 1000):
        assert _supported(lib, lib.FftParams(n=n, window_type=0)) == E_ARG, n
        assert _supported(lib, lib.MtmParams(n=n, w=2.5, kmax=4)) == E_ARG, n
    assert _supported(lib, lib.HparmaParams(n=4096)) == E_ARG
    assert _supported(lib, lib.LmpParams(n=1024)) == E_ARG
    for m in (1, 2):
        assert _supported(lib, lib.FftParams(n=1024, window_type=0, sub_mean=m)) == E_ARG
        assert _supported(lib, lib.MtmParams(n=1024, w=2.5, kmax=4, sub_mean=m)) == E_ARG
    assert _supported(lib, lib.FftParams(n=1024, window_type=0, limiter=1)) == E_ARG
    assert _supported(lib, lib.FftParams(n=1024, window_type=0, a=0.5)) == E_ARG
    assert lib.iq_supported(lib.FftParams(n=1024, window_type=0)) and not lib.iq_supported(lib.FftParams(n=128, window_type=0))


def _ulps(a, b):
    """Distance in float32 steps between two float32 arrays of one sign pattern (or zeros)."""
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    ia = np.where(ia < 0, -(ia & 0x7fffffff), ia)
    ib = np.where(ib < 0, -(ib & 0x7fffffff), ib)
    return np.abs(ia - ib)


@pytest.mark.parametrize("n", [256, 4096])
@pytest.mark.parametrize("name", ["hanning", "blackman", "gaussian", "welch", "bartlett", "rectangular", "hamming", "kaiser"])
def test_iq_table_of_every_window(lib, n, name):
    """window (the library's float32 table; ones for 'rectangular', which is never applied: fft.c:132,139) times sqrt(1 / N),
    the product in double, rounded once."""
    wt = lib.WINDOWS[name]
    tab = lib.iq_tables(lib.FftParams(n=n, window_type=wt))
    assert tab.shape == (1, n) and tab.dtype == np.float32
    w = np.ones(n) if name == "rectangular" else lib.make_window(wt, n).astype(np.float64)
    ref = (w * np.sqrt(1.0 / n)).astype(np.float32)
    assert _ulps(tab[0], ref).max() <= 1
    assert (tab[0] ** 2).astype(np.float64).sum() == pytest.approx(1.0 if name == "rectangular" else 1.0 / n, rel=1e-5)


@pytest.mark.parametrize("n", [1024, 4096])
@pytest.mark.parametrize("kmax", [0, 3, 4])
def test_iq_table_of_the_tapers(lib, n, kmax):
    """1, 4 and 5 tapers: v_j sqrt(1 / (N (1 + sig_j))) from the library's double tapers and eigenvalues, rounded once."""
    nw = 2.5 if kmax else 2.0
    tab = lib.iq_tables(lib.MtmParams(n=n, w=nw, kmax=kmax))
    assert tab.shape == (kmax + 1, n)
    v, sig = lib.make_dpss(n, kmax, nw)
    ref = (v * np.sqrt(1.0 / (n * (1.0 + sig)))[:, None]).astype(np.float32)
    assert _ulps(tab, ref).max() <= 1


def test_iq_tables_refusals(lib):
    L = lib.api.lib()
    assert L.glfer_hip_iq_tables(None, None) == E_ARG
    for params in (lib.FftParams(n=128, window_type=0), lib.LmpParams(n=1024), lib.FftParams(n=1024, window_type=0, sub_mean=1),
                   lib.FftParams(n=1024, window_type=9), lib.MtmParams(n=1024, w=2.5, kmax=32), lib.MtmParams(n=1024, w=0.0, kmax=4)):
        cfg = lib.api.make_config(params)
        assert L.glfer_hip_iq_tables(C.byref(cfg), None) == E_ARG
    cfg = lib.api.make_config(lib.MtmParams(n=1024, w=4.0, kmax=7))
    assert L.glfer_hip_iq_tables(C.byref(cfg), None) == 8                       # the count alone
    cfg = lib.api.make_config(lib.FftParams(n=1024, window_type=0))
    assert L.glfer_hip_iq_tables(C.byref(cfg), None) == 1


def _plan(lib, params):
    """A plan where one can be made (a plan needs a device for its tables), else None."""
    L = lib.api.lib()
    cfg = lib.api.make_config(params)
    h = C.c_void_p()
    return h if L.glfer_hip_plan_create(C.byref(cfg), C.byref(h)) == 0 else None


def device_entry_refusals(lib):
    """Every refusal of the two device entries that needs a plan; shared with tests/test_gpu_iq.py.  The buffers are fake
    addresses: a refusal must come before anything reads them or is launched.  Returns the number of plans it could make."""
    L = lib.api.lib()
    one, many = L.glfer_hip_spectrogram_iq_device, L.glfer_hip_spectrogram_iq_batch_device
    made = 0
    fake, out = 0x10000, 0x4000000
    for fmt, csz in ((lib.SAMPLES_F32, 8), (lib.SAMPLES_S16, 4), (lib.SAMPLES_U8, 2)):
        n = 1024
        h = _plan(lib, lib.FftParams(n=n, window_type=0, overlap=0.5, sample_format=fmt))
        if h is None:
            continue
        made += 1
        try:
            hop = L.glfer_hip_hop(h)
            ns = 10 * hop
            for flags in (4, 8, 0x80000000, 0xfffffffc):                                   # unknown flag bits
                assert one(h, fake, ns, 0, 4, out, 0, flags, None) == E_ARG
                assert many(h, fake, 2, ns, ns, 0, 4, out, 0, flags, None) == E_ARG
            for pitch in (1, n - 1, n // 2 + 1):                                            # a pitch below N
                assert one(h, fake, ns, 0, 4, out, pitch, 0, None) == E_ARG
                assert many(h, fake, 2, ns, ns, 0, 4, out, pitch, 0, None) == E_ARG
            for off in range(1, csz):                                                       # off one complex sample
                if off & (csz - 1):
                    assert one(h, fake + off, ns, 0, 4, out, 0, 0, None) == E_ARG
                    assert many(h, fake + off, 2, ns, ns, 0, 4, out, 0, 0, None) == E_ARG
            assert one(h, fake, ns, 7, 4, out, 0, 0, None) == E_ARG                         # a frame past the stream
            assert one(h, fake, ns, 10, 1, out, 0, 0, None) == E_ARG
            assert many(h, fake, 3, ns, ns, 7, 4, out, 0, 0, None) == E_ARG
            assert one(h, fake, ns, 2 ** 64 - 2, 4, out, 0, 0, None) == E_ARG               # first + nframes wraps
            assert many(h, fake, 2, ns, ns, 2 ** 64 - 2, 4, out, 0, 0, None) == E_ARG
            assert one(h, fake, 2 ** 33 * hop, 0, 2 ** 31, out, 0, 0, None) == E_ARG        # nframes > 0x7fffffff
            assert many(h, fake, 2, 2 ** 33 * hop, 2 ** 33 * hop, 0, 2 ** 31, out, 0, 0, None) == E_ARG
            assert one(h, None, ns, 0, 4, out, 0, 0, None) == E_ARG                         # NULL buffers while there is work
            assert one(h, fake, ns, 0, 4, None, 0, 0, None) == E_ARG
            assert many(h, None, 2, ns, ns, 0, 4, out, 0, 0, None) == E_ARG
            assert many(h, fake, 2, ns, ns, 0, 4, None, 0, 0, None) == E_ARG
            assert many(h, fake, 2 ** 40, 2 ** 40, ns, 0, 4, out, 0, 0, None) == E_ARG      # sizes that overflow size_t
            assert one(h, None, ns, 0, 0, None, 0, 0, None) == OK                           # no frames: nothing to do
            assert one(h, None, ns, 99, 0, None, n + 8, 3, None) == OK
            assert many(h, None, 0, ns, ns, 0, 4, None, 0, 0, None) == OK                   # no streams
            assert many(h, None, 5, ns, ns, 0, 0, None, 0, 0, None) == OK
            assert one(None, fake, ns, 0, 4, out, 0, 0, None) == E_ARG
        finally:
            L.glfer_hip_plan_destroy(h)
    # plans that make no I/Q rows: other modes, other N, mean removal, the limiter
    for params in (lib.LmpParams(n=1024, overlap=0.5), lib.HparmaParams(n=1024, t=32, p_e=8), lib.FftParams(n=128, window_type=0),
                   lib.FftParams(n=32768, window_type=0), lib.FftParams(n=1024, window_type=0, sub_mean=1),
                   lib.MtmParams(n=1024, w=2.5, kmax=4, sub_mean=2), lib.FftParams(n=1024, window_type=0, limiter=1),
                   lib.FftParams(n=1024, window_type=0, a=0.25)):
        h = _plan(lib, params)
        if h is None:
            continue
        made += 1
        try:
            ns = 10 * L.glfer_hip_hop(h)
            assert one(h, fake, ns, 0, 4, out, 0, 0, None) == E_ARG
            assert many(h, fake, 2, ns, ns, 0, 4, out, 0, 0, None) == E_ARG
            assert one(h, None, ns, 0, 0, None, 0, 0, None) == E_ARG                        # (refused even with no work)
        finally:
            L.glfer_hip_plan_destroy(h)
    return made


def test_null_plan_and_device_entry_refusals(lib):
    L = lib.api.lib()
    fake = 0x10000
    assert L.glfer_hip_spectrogram_iq_device(None, fake, 4096, 0, 1, fake, 0, 0, None) == E_ARG
    assert L.glfer_hip_spectrogram_iq_device(None, None, 0, 0, 0, None, 0, 0, None) == E_ARG
    assert L.glfer_hip_spectrogram_iq_batch_device(None, fake, 2, 4096, 4096, 0, 1, fake, 0, 0, None) == E_ARG
    made = device_entry_refusals(lib)              # (a plan needs a device: 0 here without one)
    assert made in (0, 11)
