"""The cross-spectrum entries without a GPU: exported and listed, the ABI number, glfer_hip_cross_supported over sizes, modes and
options, and every refusal of the two device entries (the ones that need a plan: where a plan can be made; tests/test_gpu_cross.py
runs the same helper where one always can)."""
import ctypes as C
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, E_ARG = 0, -1
ENTRIES = ("glfer_hip_cross_supported", "glfer_hip_mtm_cross_device", "glfer_hip_mtm_cross_batch_device")
SIZES = (256, 512, 1024, 2048, 4096, 8192)


def test_cross_entries_exported(lib):
    L = lib.api.lib()
    for name in ENTRIES:
        assert hasattr(L, name), name
        assert name in lib.api.EXPORTS, name
    for name in ("cross", "cross_batch"):
        assert callable(getattr(lib.Spectrogram, name, None)), name
    assert callable(lib.cross_supported)
    assert lib.Cross._fields == ("sxx", "syy", "sxy", "coh")
    assert L.glfer_hip_abi_version() == 5                        # entries added: the ABI number stays
    header = open(os.path.join(ROOT, "include", "glfer_hip.h")).read()
    assert "#define GLFER_HIP_ABI 5" in header
    for name in ENTRIES:
        assert name + "(" in header, name
    for words in ("rounding of the PAIR", "like level", "identically 1"):    # the accuracy note, and why FFT plans are refused
        assert words in header, words


def _supported(lib, params):
    cfg = lib.api.make_config(params)
    return lib.api.lib().glfer_hip_cross_supported(C.byref(cfg))


def test_cross_supported(lib):
    L = lib.api.lib()
    assert L.glfer_hip_cross_supported(None) == E_ARG
    for n in SIZES:
        for kmax, nw in ((1, 2.0), (4, 2.5), (7, 4.0)):
            for overlap in (0.0, 0.3, 0.5, 0.75):
                assert _supported(lib, lib.MtmParams(n=n, overlap=overlap, w=nw, kmax=kmax)) == OK, (n, kmax, overlap)
        assert _supported(lib, lib.MtmParams(n=n, w=2.0, kmax=0)) == E_ARG, n           # one taper: coherence is identically 1
        assert _supported(lib, lib.FftParams(n=n, window_type=0, overlap=0.5)) == E_ARG, n  # one window: the same
    for fmt in (lib.SAMPLES_F32, lib.SAMPLES_S16, lib.SAMPLES_U8):
        for hist in (lib.HISTORY_ZERO_FIRST, lib.HISTORY_ZERO_ALWAYS):
            assert _supported(lib, lib.MtmParams(n=1024, overlap=0.3, w=2.5, kmax=4, sample_format=fmt, history_mode=hist)) == OK
    for n in (128, 16384, 32768, 1000):
        assert _supported(lib, lib.MtmParams(n=n, w=2.5, kmax=4)) == E_ARG, n
    assert _supported(lib, lib.HparmaParams(n=4096)) == E_ARG
    assert _supported(lib, lib.LmpParams(n=1024)) == E_ARG
    for m in (1, 2):
        assert _supported(lib, lib.MtmParams(n=1024, w=2.5, kmax=4, sub_mean=m)) == E_ARG
    assert lib.cross_supported(lib.MtmParams(n=1024, w=2.5, kmax=4)) and not lib.cross_supported(lib.MtmParams(n=128, w=2.5, kmax=4))
    # every plan that gives cross rows takes I/Q input: the kernel reads the plan's I/Q table
    assert lib.iq_supported(lib.MtmParams(n=1024, w=2.5, kmax=4))


def _plan(lib, params):
    """A plan where one can be made (a plan needs a device for its tables), else None."""
    L = lib.api.lib()
    cfg = lib.api.make_config(params)
    h = C.c_void_p()
    return h if L.glfer_hip_plan_create(C.byref(cfg), C.byref(h)) == 0 else None


def device_entry_refusals(lib):
    """Every refusal of the two device entries that needs a plan; shared with tests/test_gpu_cross.py.  The buffers are fake
    addresses: a refusal must come before anything reads them or is launched.  Returns the number of plans it could make."""
    L = lib.api.lib()
    one, many = L.glfer_hip_mtm_cross_device, L.glfer_hip_mtm_cross_batch_device
    made = 0
    fake, o1, o2, o3, o4 = 0x10000, 0x4000000, 0x5000000, 0x6000000, 0x7000000
    for fmt, csz in ((lib.SAMPLES_F32, 8), (lib.SAMPLES_S16, 4), (lib.SAMPLES_U8, 2)):
        n = 1024
        bins = n // 2 + 1
        h = _plan(lib, lib.MtmParams(n=n, overlap=0.5, w=2.5, kmax=4, sample_format=fmt))
        if h is None:
            continue
        made += 1
        try:
            hop = L.glfer_hip_hop(h)
            ns = 10 * hop
            for pitch in (1, bins - 1, n // 4):                                             # a pitch below N/2 + 1, either one
                assert one(h, fake, ns, 0, 4, o1, o2, o3, pitch, o4, 0, None) == E_ARG
                assert one(h, fake, ns, 0, 4, o1, o2, o3, 0, o4, pitch, None) == E_ARG
                assert many(h, fake, 2, ns, ns, 0, 4, o1, o2, o3, pitch, o4, 0, None) == E_ARG
                assert many(h, fake, 2, ns, ns, 0, 4, o1, o2, o3, 0, o4, pitch, None) == E_ARG
            assert one(h, fake, ns, 0, 4, None, None, None, 0, None, 0, None) == E_ARG      # all four outputs NULL
            assert many(h, fake, 2, ns, ns, 0, 4, None, None, None, 0, None, 0, None) == E_ARG
            for off in range(1, csz):                                                       # off one pair
                assert one(h, fake + off, ns, 0, 4, o1, o2, o3, 0, o4, 0, None) == E_ARG
                assert many(h, fake + off, 2, ns, ns, 0, 4, o1, o2, o3, 0, o4, 0, None) == E_ARG
            assert one(h, fake, ns, 7, 4, o1, None, None, 0, None, 0, None) == E_ARG        # a frame past the stream
            assert one(h, fake, ns, 10, 1, o1, None, None, 0, None, 0, None) == E_ARG
            assert many(h, fake, 3, ns, ns, 7, 4, None, None, o3, 0, None, 0, None) == E_ARG
            assert one(h, fake, ns, 2 ** 64 - 2, 4, o1, o2, o3, 0, o4, 0, None) == E_ARG    # first + nframes wraps
            assert many(h, fake, 2, ns, ns, 2 ** 64 - 2, 4, o1, o2, o3, 0, o4, 0, None) == E_ARG
            assert one(h, fake, 2 ** 33 * hop, 0, 2 ** 31, o1, o2, o3, 0, o4, 0, None) == E_ARG   # nframes > 0x7fffffff
            assert many(h, fake, 2, 2 ** 33 * hop, 2 ** 33 * hop, 0, 2 ** 31, o1, o2, o3, 0, o4, 0, None) == E_ARG
            assert one(h, None, ns, 0, 4, o1, o2, o3, 0, o4, 0, None) == E_ARG              # no input while there is work
            assert many(h, None, 2, ns, ns, 0, 4, o1, o2, o3, 0, o4, 0, None) == E_ARG
            assert many(h, fake, 2 ** 40, 2 ** 40, ns, 0, 4, o1, o2, o3, 0, o4, 0, None) == E_ARG   # sizes that overflow size_t
            assert one(h, None, ns, 0, 0, None, None, None, 0, None, 0, None) == OK         # no frames: nothing to do
            assert one(h, None, ns, 99, 0, None, None, None, bins + 8, None, bins, None) == OK
            assert many(h, None, 0, ns, ns, 0, 4, None, None, None, 0, None, 0, None) == OK   # no streams
            assert many(h, None, 5, ns, ns, 0, 0, None, None, None, 0, None, 0, None) == OK
            assert one(None, fake, ns, 0, 4, o1, o2, o3, 0, o4, 0, None) == E_ARG
        finally:
            L.glfer_hip_plan_destroy(h)
    # plans that make no cross rows: one window or one taper, other modes, other N, mean removal
    for params in (lib.FftParams(n=1024, window_type=0, overlap=0.5), lib.MtmParams(n=1024, w=2.0, kmax=0),
                   lib.LmpParams(n=1024, overlap=0.5), lib.HparmaParams(n=1024, t=32, p_e=8), lib.MtmParams(n=128, w=2.5, kmax=4),
                   lib.MtmParams(n=16384, w=2.5, kmax=4), lib.MtmParams(n=1024, w=2.5, kmax=4, sub_mean=2)):
        h = _plan(lib, params)
        if h is None:
            continue
        made += 1
        try:
            ns = 10 * L.glfer_hip_hop(h)
            assert one(h, fake, ns, 0, 4, o1, o2, o3, 0, o4, 0, None) == E_ARG
            assert many(h, fake, 2, ns, ns, 0, 4, o1, o2, o3, 0, o4, 0, None) == E_ARG
            assert one(h, None, ns, 0, 0, None, None, None, 0, None, 0, None) == E_ARG      # (refused even with no work)
        finally:
            L.glfer_hip_plan_destroy(h)
    return made


def test_null_plan_and_device_entry_refusals(lib):
    L = lib.api.lib()
    fake = 0x10000
    assert L.glfer_hip_mtm_cross_device(None, fake, 4096, 0, 1, fake, None, None, 0, None, 0, None) == E_ARG
    assert L.glfer_hip_mtm_cross_device(None, None, 0, 0, 0, None, None, None, 0, None, 0, None) == E_ARG
    assert L.glfer_hip_mtm_cross_batch_device(None, fake, 2, 4096, 4096, 0, 1, fake, None, None, 0, None, 0, None) == E_ARG
    made = device_entry_refusals(lib)              # (a plan needs a device: 0 here without one)
    assert made in (0, 10)
