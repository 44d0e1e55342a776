"""The Welch cross-spectrum entries without a GPU: exported and listed, glfer_hip_welch_cross_supported over plans, segment counts
and steps (the step bound at its exact edge), glfer_hip_welch_rows against its formula, the refusals that need no plan, the
header's words.  The refusals that need a plan: device_entry_refusals, where a plan can be made (tests/test_gpu_welch.py runs it
where one always can)."""
import ctypes as C
import os

import pytest

import _welch_exact as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, E_ARG = 0, -1
ENTRIES = ("glfer_hip_welch_cross_supported", "glfer_hip_welch_rows", "glfer_hip_welch_cross_device", "glfer_hip_welch_cross_batch_device")
SIZES = (256, 512, 1024, 2048, 4096, 8192)
PAIR_BYTES = {"f32": 8, "s16": 4, "u8": 2}


def test_welch_entries_exported(lib):
    L = lib.api.lib()
    for name in ENTRIES:
        assert hasattr(L, name), name
        assert name in lib.api.EXPORTS, name
    for name in ("cross_welch", "cross_welch_batch", "welch_rows"):
        assert callable(getattr(lib.Spectrogram, name, None)), name
    assert callable(lib.welch_cross_supported)
    assert L.glfer_hip_abi_version() == 5                        # entries added: the ABI number stays


def test_header_words():
    header = open(os.path.join(ROOT, "include", "glfer_hip.h")).read()
    for name in ENTRIES:
        assert name + "(" in header, name
    # the accuracy note of the per-frame entries stays, and why they refuse FFT plans
    for words in ("rounding of the PAIR", "like level", "identically 1",
                  "ACCURACY: both channels ride one transform, so a channel's separated spectrum carries the rounding of the PAIR, not its own."):
        assert words in header, words
    # the Welch paragraph: the definition, the row count, the order, the scale, the bound on step
    for words in ("(1/L) sum_s sum_j c_j X_{f,j}[k] conj(Y_{f,j}[k])", "(F - first_frame - L) / step + 1", "segments outermost",
                  "0.25 / L rounded once", "(FPB - 1) step H + N <= (2^31 - 1) / (bytes of a pair)", "ANY of a row's L segments"):
        assert words in header, words
    assert "Welch-style averaging of Sxy over frames for FFT plans" not in header        # no longer among the things not built


def _supported(lib, params, segments, step):
    cfg = lib.api.make_config(params)
    return lib.api.lib().glfer_hip_welch_cross_supported(C.byref(cfg), segments, step)


def test_welch_supported_accepts(lib):
    for n in SIZES:
        for name, wt in lib.WINDOWS.items():
            for seg in (2, 3, 16, 4096):
                assert _supported(lib, lib.FftParams(n=n, window_type=wt, overlap=0.5), seg, seg) == OK, (n, name, seg)
        for overlap in (0.0, 0.3, 0.5, 0.75):
            assert _supported(lib, lib.FftParams(n=n, window_type=0, overlap=overlap), 2, 1) == OK, (n, overlap)
        assert _supported(lib, lib.MtmParams(n=n, w=2.0, kmax=0), 2, 1) == OK, n
        assert _supported(lib, lib.MtmParams(n=n, w=2.0, kmax=0), 5, 7) == OK, n
        for kmax, nw in ((1, 2.0), (4, 2.5), (7, 4.0)):
            assert _supported(lib, lib.MtmParams(n=n, w=nw, kmax=kmax), 1, 1) == OK, (n, kmax)     # one segment: the tapers average
            assert _supported(lib, lib.MtmParams(n=n, w=nw, kmax=kmax), 4, 2) == OK, (n, kmax)
    for fmt in (lib.SAMPLES_F32, lib.SAMPLES_S16, lib.SAMPLES_U8):
        for hist in (lib.HISTORY_ZERO_FIRST, lib.HISTORY_ZERO_ALWAYS):
            assert _supported(lib, lib.FftParams(n=1024, window_type=0, overlap=0.3, sample_format=fmt, history_mode=hist), 3, 5) == OK
    assert lib.welch_cross_supported(lib.FftParams(n=1024, window_type=0, overlap=0.5), 16, 16)
    assert not lib.welch_cross_supported(lib.FftParams(n=1024, window_type=0, overlap=0.5), 1, 1)


def test_welch_supported_refuses(lib):
    L = lib.api.lib()
    assert L.glfer_hip_welch_cross_supported(None, 2, 2) == E_ARG
    fft = lib.FftParams(n=1024, window_type=0, overlap=0.5)
    assert _supported(lib, fft, 1, 1) == E_ARG                                   # L J = 1: identically 1
    assert _supported(lib, lib.MtmParams(n=1024, w=2.0, kmax=0), 1, 1) == E_ARG
    for params in (fft, lib.MtmParams(n=1024, w=2.5, kmax=4)):
        assert _supported(lib, params, 0, 1) == E_ARG                            # L = 0
        assert _supported(lib, params, 4097, 1) == E_ARG                         # L > 4096
        assert _supported(lib, params, 4096, 1) == OK
        assert _supported(lib, params, 4, 0) == E_ARG                            # step = 0
    for n in (128, 16384, 1000):
        assert _supported(lib, lib.FftParams(n=n, window_type=0, overlap=0.5), 4, 4) == E_ARG, n
        assert _supported(lib, lib.MtmParams(n=n, w=2.5, kmax=4), 4, 4) == E_ARG, n
    assert _supported(lib, lib.LmpParams(n=1024), 4, 4) == E_ARG
    assert _supported(lib, lib.HparmaParams(n=4096), 4, 4) == E_ARG
    for m in (1, 2):
        assert _supported(lib, lib.FftParams(n=1024, window_type=0, sub_mean=m), 4, 4) == E_ARG
        assert _supported(lib, lib.MtmParams(n=1024, w=2.5, kmax=4, sub_mean=m), 4, 4) == E_ARG
    assert _supported(lib, lib.FftParams(n=1024, window_type=0, a=0.5, limiter=1), 4, 4) == E_ARG      # limiter on
    assert _supported(lib, lib.FftParams(n=1024, window_type=0, a=0.5), 4, 4) == E_ARG                 # RA9MB


@pytest.mark.parametrize("fmt", ["f32", "s16", "u8"])
@pytest.mark.parametrize("n,overlap", [(256, 0.0), (256, 0.75), (2048, 0.5), (2048, 0.0)])
def test_step_bound_at_its_edge(lib, n, overlap, fmt):
    """(FPB - 1) step H + N <= (2^31 - 1) / pair_bytes with FPB = 4096 / N: the largest step that holds it is accepted, the next refused."""
    sf = {"f32": lib.SAMPLES_F32, "s16": lib.SAMPLES_S16, "u8": lib.SAMPLES_U8}[fmt]
    params = lib.FftParams(n=n, window_type=0, overlap=overlap, sample_format=sf)
    fpb, hop = 4096 // n, W.hop_len(n, overlap)
    pairs = (2 ** 31 - 1) // PAIR_BYTES[fmt]
    edge = (pairs - n) // ((fpb - 1) * hop)
    assert (fpb - 1) * edge * hop + n <= pairs < (fpb - 1) * (edge + 1) * hop + n
    assert _supported(lib, params, 4, edge) == OK
    assert _supported(lib, params, 4, edge + 1) == E_ARG
    assert _supported(lib, params, 4, 2 ** 63) == E_ARG


@pytest.mark.parametrize("n", [4096, 8192])
def test_no_step_bound_where_a_block_has_one_row(lib, n):
    for step in (2 ** 31, 2 ** 40, 2 ** 64 - 1):
        assert _supported(lib, lib.FftParams(n=n, window_type=0, overlap=0.75), 4, step) == OK, step


def _plan(lib, params):
    """A plan where one can be made (a plan needs a device for its tables), else None."""
    L = lib.api.lib()
    cfg = lib.api.make_config(params)
    h = C.c_void_p()
    return h if L.glfer_hip_plan_create(C.byref(cfg), C.byref(h)) == 0 else None


def check_welch_rows(lib):
    """glfer_hip_welch_rows against (F - first - L) / step + 1; shared with tests/test_gpu_welch.py.  Returns the plans made."""
    L = lib.api.lib()
    made = 0
    for params in (lib.FftParams(n=1024, window_type=0, overlap=0.5), lib.MtmParams(n=256, overlap=0.3, w=2.5, kmax=4)):
        h = _plan(lib, params)
        if h is None:
            continue
        made += 1
        try:
            hop = L.glfer_hip_hop(h)
            for F in (0, 1, 7, 40):
                for ns in (F * hop, F * hop + hop - 1):
                    for first in (0, 1, 5, F, F + 1):
                        for seg in (1, 2, 7, 40, 41):
                            for step in (1, 2, seg, seg + 3):
                                got = L.glfer_hip_welch_rows(h, ns, first, seg, step)
                                assert got == W.rows_of(F, seg, step, first), (F, ns, first, seg, step, got)
            assert L.glfer_hip_welch_rows(h, 10 * hop, 3, 8, 2) == 0            # F - first < L
            assert L.glfer_hip_welch_rows(h, 10 * hop, 3, 7, 2) == 1            # F - first = L
            assert L.glfer_hip_welch_rows(h, 10 * hop, 2 ** 64 - 2, 4, 1) == 0  # first + L wraps
            assert L.glfer_hip_welch_rows(h, 10 * hop, 0, 0, 1) == 0 and L.glfer_hip_welch_rows(h, 10 * hop, 0, 2, 0) == 0
        finally:
            L.glfer_hip_plan_destroy(h)
    return made


def device_entry_refusals(lib):
    """Every refusal of the two device entries that needs a plan; shared with tests/test_gpu_welch.py.  The buffers are fake
    addresses: a refusal must come before anything reads them or is launched.  Returns the number of plans it could make."""
    L = lib.api.lib()
    one, many = L.glfer_hip_welch_cross_device, L.glfer_hip_welch_cross_batch_device
    made = 0
    fake, o1, o2, o3, o4 = 0x10000, 0x4000000, 0x5000000, 0x6000000, 0x7000000
    for fmt, csz in ((lib.SAMPLES_F32, 8), (lib.SAMPLES_S16, 4), (lib.SAMPLES_U8, 2)):
        n = 1024
        bins = n // 2 + 1
        h = _plan(lib, lib.FftParams(n=n, window_type=0, overlap=0.5, sample_format=fmt))
        if h is None:
            continue
        made += 1
        try:
            hop = L.glfer_hip_hop(h)
            ns = 10 * hop                                                                   # ten frames: (L, step) = (4, 2) has 4 rows
            for pitch in (1, bins - 1, n // 4):                                             # a pitch below N/2 + 1, either one
                assert one(h, fake, ns, 0, 4, 2, 4, o1, o2, o3, pitch, o4, 0, None) == E_ARG
                assert one(h, fake, ns, 0, 4, 2, 4, o1, o2, o3, 0, o4, pitch, None) == E_ARG
                assert many(h, fake, 2, ns, ns, 0, 4, 2, 4, o1, o2, o3, pitch, o4, 0, None) == E_ARG
                assert many(h, fake, 2, ns, ns, 0, 4, 2, 4, o1, o2, o3, 0, o4, pitch, None) == E_ARG
            assert one(h, fake, ns, 0, 4, 2, 4, None, None, None, 0, None, 0, None) == E_ARG   # all four outputs NULL
            assert many(h, fake, 2, ns, ns, 0, 4, 2, 4, None, None, None, 0, None, 0, None) == E_ARG
            for off in range(1, csz):                                                       # off one pair
                assert one(h, fake + off, ns, 0, 4, 2, 4, o1, o2, o3, 0, o4, 0, None) == E_ARG
                assert many(h, fake + off, 2, ns, ns, 0, 4, 2, 4, o1, o2, o3, 0, o4, 0, None) == E_ARG
            assert one(h, fake, ns, 0, 4, 2, 5, o1, None, None, 0, None, 0, None) == E_ARG     # a row's last frame past the stream
            assert one(h, fake, ns, 7, 4, 2, 1, o1, None, None, 0, None, 0, None) == E_ARG
            assert one(h, fake, ns, 10, 1, 1, 1, o1, None, None, 0, None, 0, None) == E_ARG
            assert many(h, fake, 3, ns, ns, 1, 4, 2, 4, None, None, o3, 0, None, 0, None) == E_ARG
            assert one(h, fake, ns, 2 ** 64 - 2, 4, 2, 1, o1, o2, o3, 0, o4, 0, None) == E_ARG    # first + segments wraps
            assert many(h, fake, 2, ns, ns, 2 ** 64 - 2, 4, 2, 1, o1, o2, o3, 0, o4, 0, None) == E_ARG
            assert one(h, fake, 2 ** 33 * hop, 0, 2, 1, 2 ** 31, o1, o2, o3, 0, o4, 0, None) == E_ARG   # nrows > 0x7fffffff
            assert many(h, fake, 2, 2 ** 33 * hop, 2 ** 33 * hop, 0, 2, 1, 2 ** 31, o1, o2, o3, 0, o4, 0, None) == E_ARG
            assert one(h, None, ns, 0, 4, 2, 4, o1, o2, o3, 0, o4, 0, None) == E_ARG           # no input while there is work
            assert many(h, None, 2, ns, ns, 0, 4, 2, 4, o1, o2, o3, 0, o4, 0, None) == E_ARG
            assert many(h, fake, 2 ** 40, 2 ** 40, ns, 0, 4, 2, 4, o1, o2, o3, 0, o4, 0, None) == E_ARG   # sizes that overflow size_t
            for seg, step in ((1, 1), (0, 1), (4097, 1), (4, 0), (4, 2 ** 31)):               # what _supported refuses (N = 1024: the step bound)
                assert one(h, fake, ns, 0, seg, step, 1, o1, o2, o3, 0, o4, 0, None) == E_ARG, (seg, step)
                assert many(h, fake, 2, ns, ns, 0, seg, step, 1, o1, o2, o3, 0, o4, 0, None) == E_ARG, (seg, step)
                assert one(h, None, ns, 0, seg, step, 0, None, None, None, 0, None, 0, None) == E_ARG   # (refused even with no work)
            assert one(h, None, ns, 0, 4, 2, 0, None, None, None, 0, None, 0, None) == OK      # no rows: nothing to do
            assert one(h, None, ns, 99, 4, 2, 0, None, None, None, bins + 8, None, bins, None) == OK
            assert many(h, None, 0, ns, ns, 0, 4, 2, 4, None, None, None, 0, None, 0, None) == OK   # no streams
            assert many(h, None, 5, ns, ns, 0, 4, 2, 0, None, None, None, 0, None, 0, None) == OK
            assert one(None, fake, ns, 0, 4, 2, 4, o1, o2, o3, 0, o4, 0, None) == E_ARG
        finally:
            L.glfer_hip_plan_destroy(h)
    # plans that make no Welch rows: other modes, other N, mean removal
    for params in (lib.LmpParams(n=1024, overlap=0.5), lib.HparmaParams(n=1024, t=32, p_e=8), lib.FftParams(n=128, window_type=0),
                   lib.MtmParams(n=16384, w=2.5, kmax=4), lib.FftParams(n=1024, window_type=0, sub_mean=2)):
        h = _plan(lib, params)
        if h is None:
            continue
        made += 1
        try:
            ns = 10 * L.glfer_hip_hop(h)
            assert one(h, fake, ns, 0, 4, 2, 4, o1, o2, o3, 0, o4, 0, None) == E_ARG
            assert many(h, fake, 2, ns, ns, 0, 4, 2, 4, o1, o2, o3, 0, o4, 0, None) == E_ARG
            assert one(h, None, ns, 0, 4, 2, 0, None, None, None, 0, None, 0, None) == E_ARG   # (refused even with no work)
        finally:
            L.glfer_hip_plan_destroy(h)
    # the per-frame entries still refuse an FFT plan
    h = _plan(lib, lib.FftParams(n=1024, window_type=0, overlap=0.5))
    if h is not None:
        made += 1
        try:
            ns = 10 * L.glfer_hip_hop(h)
            assert L.glfer_hip_mtm_cross_device(h, fake, ns, 0, 4, o1, o2, o3, 0, o4, 0, None) == E_ARG
            assert L.glfer_hip_mtm_cross_batch_device(h, fake, 2, ns, ns, 0, 4, o1, o2, o3, 0, o4, 0, None) == E_ARG
        finally:
            L.glfer_hip_plan_destroy(h)
    return made


def test_null_plan_refusals_and_rows(lib):
    L = lib.api.lib()
    fake = 0x10000
    assert L.glfer_hip_welch_cross_device(None, fake, 4096, 0, 2, 2, 1, fake, None, None, 0, None, 0, None) == E_ARG
    assert L.glfer_hip_welch_cross_device(None, None, 0, 0, 2, 2, 0, None, None, None, 0, None, 0, None) == E_ARG
    assert L.glfer_hip_welch_cross_batch_device(None, fake, 2, 4096, 4096, 0, 2, 2, 1, fake, None, None, 0, None, 0, None) == E_ARG
    assert L.glfer_hip_welch_rows(None, 4096, 0, 2, 2) == 0
    assert check_welch_rows(lib) in (0, 2)          # (a plan needs a device: 0 here without one)
    assert device_entry_refusals(lib) in (0, 9)


def test_rows_formula_of_the_test_helper():
    assert W.rows_of(10, 8, 2, 3) == 0 and W.rows_of(10, 7, 2, 3) == 1 and W.rows_of(10, 2, 3) == 3 and W.rows_of(10, 2, 3, 1) == 3
    assert W.rows_of(0, 1, 1) == 0 and W.rows_of(16, 16, 16) == 1 and W.rows_of(48, 16, 16) == 3
