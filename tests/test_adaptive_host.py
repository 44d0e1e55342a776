"""The adaptive-weight entries without a GPU: exported and listed, the ABI number, glfer_hip_adaptive_supported over modes, sizes,
taper counts and options, glfer_hip_adaptive_weights against make_dpss in double, the launcher table against the Makefile and the
library, and every refusal of the two device entries (the ones that need a plan: where a plan can be made;
tests/test_gpu_adaptive.py runs the same helper where one always can)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "glfer_amd", "csrc")
OK, E_ARG = 0, -1
ENTRIES = ("glfer_hip_adaptive_supported", "glfer_hip_adaptive_weights", "glfer_hip_mtm_adaptive_device",
           "glfer_hip_mtm_adaptive_batch_device")
SIZES = (256, 512, 1024, 2048, 4096)


def test_adaptive_entries_exported(lib):
    L = lib.api.lib()
    for name in ENTRIES:
        assert hasattr(L, name), name
        assert name in lib.api.EXPORTS, name
    for name in ("adaptive", "adaptive_batch"):
        assert callable(getattr(lib.Spectrogram, name, None)), name
    assert callable(lib.adaptive_supported) and callable(lib.adaptive_weights)
    assert lib.Adaptive._fields == ("psd", "dof")
    assert L.glfer_hip_abi_version() == 5                        # entries added: the ABI number stays
    header = open(os.path.join(ROOT, "include", "glfer_hip.h")).read()
    for name in ENTRIES:
        assert name + "(" in header, name
    # the header says that the row is a weighted mean where run's is a sum, and that the sweep count defines the result
    for words in ("weighted MEAN", "weighted SUM", "DEFINED BY THE SWEEP COUNT, NOT BY CONVERGENCE", "sweeps to a tolerance"):
        assert words in header, words


def _supported(lib, params):
    cfg = lib.api.make_config(params)
    return lib.api.lib().glfer_hip_adaptive_supported(C.byref(cfg))


def test_adaptive_supported(lib):
    L = lib.api.lib()
    assert L.glfer_hip_adaptive_supported(None) == E_ARG
    for n in SIZES:
        for kmax, nw in ((1, 2.0), (4, 2.5), (7, 4.5)):
            for overlap in (0.0, 0.3, 0.5, 0.75):
                assert _supported(lib, lib.MtmParams(n=n, overlap=overlap, w=nw, kmax=kmax)) == OK, (n, kmax, overlap)
        assert _supported(lib, lib.MtmParams(n=n, w=2.0, kmax=0)) == E_ARG, n             # one taper: nothing to weight
        assert _supported(lib, lib.MtmParams(n=n, w=6.0, kmax=8)) == E_ARG, n             # nine tapers: more than a lane keeps
        assert _supported(lib, lib.MtmParams(n=n, w=8.5, kmax=15)) == E_ARG, n
        assert _supported(lib, lib.FftParams(n=n, window_type=0, overlap=0.5)) == E_ARG, n
    for fmt in (lib.SAMPLES_F32, lib.SAMPLES_S16, lib.SAMPLES_U8):
        for hist in (lib.HISTORY_ZERO_FIRST, lib.HISTORY_ZERO_ALWAYS):
            assert _supported(lib, lib.MtmParams(n=1024, overlap=0.3, w=2.5, kmax=4, sample_format=fmt, history_mode=hist)) == OK
    for n in (128, 8192, 16384, 32768, 1000):
        assert _supported(lib, lib.MtmParams(n=n, w=2.5, kmax=4)) == E_ARG, n
    assert _supported(lib, lib.HparmaParams(n=4096)) == E_ARG
    assert _supported(lib, lib.LmpParams(n=1024)) == E_ARG
    for m in (1, 2):
        assert _supported(lib, lib.MtmParams(n=1024, w=2.5, kmax=4, sub_mean=m)) == E_ARG
    # FftParams carries the limiter and RA9MB; an MTM configuration with either set is refused as glfer_hip_iq_supported refuses it
    for field, value in (("enable_limiter", 1), ("limiter_a", 0.5)):
        cfg = lib.api.make_config(lib.MtmParams(n=1024, w=2.5, kmax=4))
        setattr(cfg, field, value)
        assert L.glfer_hip_iq_supported(C.byref(cfg)) == E_ARG, field
        assert L.glfer_hip_adaptive_supported(C.byref(cfg)) == E_ARG, field
    assert lib.adaptive_supported(lib.MtmParams(n=1024, w=2.5, kmax=4)) and not lib.adaptive_supported(lib.MtmParams(n=128, w=2.5, kmax=4))


def test_adaptive_weights_against_make_dpss(lib):
    L = lib.api.lib()
    for n, kmax, nw in ((256, 1, 2.0), (1024, 4, 2.5), (1024, 7, 4.5), (4096, 4, 2.5), (512, 7, 4.0)):
        params = lib.MtmParams(n=n, w=nw, kmax=kmax)
        lam, beta = lib.adaptive_weights(params)
        _, sig = lib.make_dpss(n, kmax, nw)
        assert lam.dtype == np.float32 and beta.dtype == np.float32 and len(lam) == len(beta) == kmax + 1
        b64 = np.maximum(-np.asarray(sig, np.float64), 0.0)
        assert (beta == b64.astype(np.float32)).all()                              # formed in double, rounded once
        assert (lam == (1.0 - b64).astype(np.float32)).all()
        assert (beta >= 0).all() and (lam > 0).all() and (lam <= 1).all()
        assert (np.diff(lam.astype(np.float64)) <= 0).all()                        # non-increasing in j
        # lambda_j + beta_j = 1 to float rounding: half an ulp of 1 for lambda, half an ulp of beta_j for beta
        err = np.abs(lam.astype(np.float64) + beta.astype(np.float64) - 1.0)
        assert (err <= 2.0 ** -25 + 2.0 ** -24 * beta.astype(np.float64)).all(), err
        # either pointer may be NULL; the count comes back
        cfg = lib.api.make_config(params)
        assert L.glfer_hip_adaptive_weights(C.byref(cfg), None, None) == kmax + 1
    bad = lib.api.make_config(lib.MtmParams(n=8192, w=2.5, kmax=4))
    assert L.glfer_hip_adaptive_weights(C.byref(bad), None, None) == E_ARG
    assert L.glfer_hip_adaptive_weights(None, None, None) == E_ARG


def test_launcher_table_makefile_and_library(lib):
    """spectro_adaptive_params.h's table, the Makefile's ALOGNS and the library's symbols name the same launchers."""
    hdr = open(os.path.join(CSRC, "spectro_adaptive_params.h")).read()
    table = {int(l) for l in re.findall(r"X\((\d+)\)", re.search(r"#define GLFER_LAUNCHERS16A\(X\)(.*)", hdr).group(1))}
    mk = open(os.path.join(CSRC, "Makefile")).read()
    alogns = {int(l) for l in re.search(r"^ALOGNS\s*=\s*([\d ]+)$", mk, re.M).group(1).split()}
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "glfer_amd", "lib", "libglfer_hip.so")],
                         check=True, capture_output=True, text=True).stdout
    library = {int(l) for l in re.findall(r"\bglfer_launch_adaptive16_n(\d+)$", out, re.M)}
    assert table == alogns == library == {8, 9, 10, 11, 12}, (table, alogns, library)
    assert {1 << l for l in table} == set(SIZES)


def _plan(lib, params):
    """A plan where one can be made (a plan needs a device for its tables), else None."""
    L = lib.api.lib()
    cfg = lib.api.make_config(params)
    h = C.c_void_p()
    return h if L.glfer_hip_plan_create(C.byref(cfg), C.byref(h)) == 0 else None


def device_entry_refusals(lib):
    """Every refusal of the two device entries that needs a plan; shared with tests/test_gpu_adaptive.py.  The buffers are fake
    addresses: a refusal must come before anything reads them or is launched.  Returns the number of plans it could make."""
    L = lib.api.lib()
    one, many = L.glfer_hip_mtm_adaptive_device, L.glfer_hip_mtm_adaptive_batch_device
    made = 0
    fake, o1, o2 = 0x10000, 0x4000000, 0x5000000
    for fmt, csz in ((lib.SAMPLES_F32, 4), (lib.SAMPLES_S16, 2), (lib.SAMPLES_U8, 1)):
        n = 1024
        bins = n // 2 + 1
        h = _plan(lib, lib.MtmParams(n=n, overlap=0.5, w=2.5, kmax=4, sample_format=fmt))
        if h is None:
            continue
        made += 1
        try:
            hop = L.glfer_hip_hop(h)
            ns = 10 * hop
            for pitch in (1, bins - 1, n // 4):                                             # a pitch below N/2 + 1
                assert one(h, fake, ns, 0, 4, o1, o2, pitch, 8, None) == E_ARG
                assert many(h, fake, 2, ns, ns, 0, 4, o1, o2, pitch, 8, None) == E_ARG
            for iters in (0, -1, 65, 1 << 20):                                              # sweeps outside 1 .. 64
                assert one(h, fake, ns, 0, 4, o1, o2, 0, iters, None) == E_ARG
                assert many(h, fake, 2, ns, ns, 0, 4, o1, o2, 0, iters, None) == E_ARG
                assert one(h, None, ns, 0, 0, None, None, 0, iters, None) == E_ARG          # (refused even with no work)
            assert one(h, fake, ns, 0, 4, None, None, 0, 8, None) == E_ARG                  # both outputs NULL
            assert many(h, fake, 2, ns, ns, 0, 4, None, None, 0, 8, None) == E_ARG
            for off in range(1, csz):                                                       # off one sample
                assert one(h, fake + off, ns, 0, 4, o1, o2, 0, 8, None) == E_ARG
                assert many(h, fake + off, 2, ns, ns, 0, 4, o1, o2, 0, 8, None) == E_ARG
            assert one(h, fake, ns, 7, 4, o1, None, 0, 8, None) == E_ARG                    # a frame past the stream
            assert one(h, fake, ns, 10, 1, None, o2, 0, 8, None) == E_ARG
            assert many(h, fake, 3, ns, ns, 7, 4, None, o2, 0, 8, None) == E_ARG
            assert one(h, fake, ns, 2 ** 64 - 2, 4, o1, o2, 0, 8, None) == E_ARG            # first + nframes wraps
            assert many(h, fake, 2, ns, ns, 2 ** 64 - 2, 4, o1, o2, 0, 8, None) == E_ARG
            assert one(h, fake, 2 ** 33 * hop, 0, 2 ** 31, o1, o2, 0, 8, None) == E_ARG     # nframes > 0x7fffffff
            assert many(h, fake, 2, 2 ** 33 * hop, 2 ** 33 * hop, 0, 2 ** 31, o1, o2, 0, 8, None) == E_ARG
            assert one(h, None, ns, 0, 4, o1, o2, 0, 8, None) == E_ARG                      # no input while there is work
            assert many(h, None, 2, ns, ns, 0, 4, o1, o2, 0, 8, None) == E_ARG
            assert many(h, fake, 2 ** 40, 2 ** 40, ns, 0, 4, o1, o2, 0, 8, None) == E_ARG   # sizes that overflow size_t
            assert one(h, None, ns, 0, 0, None, None, 0, 8, None) == OK                     # no frames: nothing to do
            assert one(h, None, ns, 99, 0, None, None, bins + 8, 1, None) == OK
            assert many(h, None, 0, ns, ns, 0, 4, None, None, 0, 64, None) == OK            # no streams
            assert many(h, None, 5, ns, ns, 0, 0, None, None, 0, 8, None) == OK
            assert one(None, fake, ns, 0, 4, o1, o2, 0, 8, None) == E_ARG
        finally:
            L.glfer_hip_plan_destroy(h)
    # plans that make no adaptive rows: one window or one taper, nine tapers, other modes, other N, mean removal
    for params in (lib.FftParams(n=1024, window_type=0, overlap=0.5), lib.MtmParams(n=1024, w=2.0, kmax=0),
                   lib.MtmParams(n=1024, w=6.0, kmax=8), lib.LmpParams(n=1024, overlap=0.5), lib.HparmaParams(n=1024, t=32, p_e=8),
                   lib.MtmParams(n=128, w=2.5, kmax=4), lib.MtmParams(n=8192, w=2.5, kmax=4),
                   lib.MtmParams(n=1024, w=2.5, kmax=4, sub_mean=2)):
        h = _plan(lib, params)
        if h is None:
            continue
        made += 1
        try:
            ns = 10 * L.glfer_hip_hop(h)
            assert one(h, fake, ns, 0, 4, o1, o2, 0, 8, None) == E_ARG
            assert many(h, fake, 2, ns, ns, 0, 4, o1, o2, 0, 8, None) == E_ARG
            assert one(h, None, ns, 0, 0, None, None, 0, 8, None) == E_ARG                  # (refused even with no work)
        finally:
            L.glfer_hip_plan_destroy(h)
    return made


def test_null_plan_and_device_entry_refusals(lib):
    L = lib.api.lib()
    fake = 0x10000
    assert L.glfer_hip_mtm_adaptive_device(None, fake, 4096, 0, 1, fake, None, 0, 8, None) == E_ARG
    assert L.glfer_hip_mtm_adaptive_device(None, None, 0, 0, 0, None, None, 0, 8, None) == E_ARG
    assert L.glfer_hip_mtm_adaptive_batch_device(None, fake, 2, 4096, 4096, 0, 1, fake, None, 0, 8, None) == E_ARG
    made = device_entry_refusals(lib)              # (a plan needs a device: 0 here without one)
    assert made in (0, 11)
