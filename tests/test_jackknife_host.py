"""The jackknife entries without a GPU: exported and listed, the ABI number, glfer_hip_jackknife_supported over modes, sizes, taper
counts and options, the launcher table against the Makefile and the library, glfer_hip_jackknife_factor against tabulated Student
quantiles, and every refusal of the two device entries (the ones that need a plan: where a plan can be made;
tests/test_gpu_jackknife.py runs the same helper where one always can)."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "glfer_amd", "csrc")
OK, E_ARG = 0, -1
ENTRIES = ("glfer_hip_jackknife_supported", "glfer_hip_jackknife_factor", "glfer_hip_mtm_jackknife_device",
           "glfer_hip_mtm_jackknife_batch_device")
SIZES = (256, 512, 1024, 2048, 4096)


def test_jackknife_entries_exported(lib):
    L = lib.api.lib()
    for name in ENTRIES:
        assert hasattr(L, name), name
        assert name in lib.api.EXPORTS, name
    for name in ("jackknife", "jackknife_batch"):
        assert callable(getattr(lib.Spectrogram, name, None)), name
    assert callable(lib.jackknife_supported) and callable(lib.jackknife_factor) and callable(lib.jackknife_interval)
    assert lib.Jackknife._fields == ("psd", "dof", "logvar")
    assert lib.Adaptive._fields == ("psd", "dof")                # Adaptive stays as it is
    assert L.glfer_hip_abi_version() == 5                        # entries added: the ABI number stays
    header = open(os.path.join(ROOT, "include", "glfer_hip.h")).read()
    for name in ENTRIES:
        assert name + "(" in header, name
    # the header says what the interval is, that it is not bias-corrected, and how the degenerate cases fall
    for words in ("THERE IS NO BIAS CORRECTION", "exp(-/+ t sqrt(logvar))", "never formed as total - term", "is ever NaN"):
        assert words in header, words


def _supported(lib, params):
    cfg = lib.api.make_config(params)
    return lib.api.lib().glfer_hip_jackknife_supported(C.byref(cfg))


def test_jackknife_supported(lib):
    L = lib.api.lib()
    assert L.glfer_hip_jackknife_supported(None) == E_ARG
    for n in SIZES:
        for kmax, nw in ((1, 2.0), (4, 2.5), (7, 4.5)):
            for overlap in (0.0, 0.3, 0.5, 0.75):
                assert _supported(lib, lib.MtmParams(n=n, overlap=overlap, w=nw, kmax=kmax)) == OK, (n, kmax, overlap)
        assert _supported(lib, lib.MtmParams(n=n, w=2.0, kmax=0)) == E_ARG, n             # one taper: nothing to delete
        assert _supported(lib, lib.MtmParams(n=n, w=6.0, kmax=8)) == E_ARG, n             # nine tapers: more than a lane keeps
        assert _supported(lib, lib.FftParams(n=n, window_type=0, overlap=0.5)) == E_ARG, n
    for fmt in (lib.SAMPLES_F32, lib.SAMPLES_S16, lib.SAMPLES_U8):
        for hist in (lib.HISTORY_ZERO_FIRST, lib.HISTORY_ZERO_ALWAYS):
            assert _supported(lib, lib.MtmParams(n=1024, overlap=0.3, w=2.5, kmax=4, sample_format=fmt, history_mode=hist)) == OK
    for n in (128, 8192, 16384, 1000):
        assert _supported(lib, lib.MtmParams(n=n, w=2.5, kmax=4)) == E_ARG, n
    assert _supported(lib, lib.HparmaParams(n=4096)) == E_ARG
    assert _supported(lib, lib.LmpParams(n=1024)) == E_ARG
    for m in (1, 2):
        assert _supported(lib, lib.MtmParams(n=1024, w=2.5, kmax=4, sub_mean=m)) == E_ARG
    for field, value in (("enable_limiter", 1), ("limiter_a", 0.5)):
        cfg = lib.api.make_config(lib.MtmParams(n=1024, w=2.5, kmax=4))
        setattr(cfg, field, value)
        assert L.glfer_hip_jackknife_supported(C.byref(cfg)) == E_ARG, field
    assert lib.jackknife_supported(lib.MtmParams(n=1024, w=2.5, kmax=4)) and not lib.jackknife_supported(lib.MtmParams(n=8192, w=2.5, kmax=4))


def test_launcher_table_makefile_and_library(lib):
    """spectro_adaptive_params.h's GLFER_LAUNCHERS16J, the Makefile's JLOGNS and the library's symbols name the same launchers,
    and every one of them is a size of the adaptive kernel (the jackknife instantiations ride in its translation units)."""
    hdr = open(os.path.join(CSRC, "spectro_adaptive_params.h")).read()
    table = {int(l) for l in re.findall(r"X\((\d+)\)", re.search(r"#define GLFER_LAUNCHERS16J\(X\)(.*)", hdr).group(1))}
    mk = open(os.path.join(CSRC, "Makefile")).read()
    jlogns = {int(l) for l in re.search(r"^JLOGNS\s*=\s*([\d ]+)$", mk, re.M).group(1).split()}
    alogns = {int(l) for l in re.search(r"^ALOGNS\s*=\s*([\d ]+)$", mk, re.M).group(1).split()}
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "glfer_amd", "lib", "libglfer_hip.so")],
                         check=True, capture_output=True, text=True).stdout
    library = {int(l) for l in re.findall(r"\bglfer_launch_jackknife16_n(\d+)$", out, re.M)}
    assert table == jlogns == library, (table, jlogns, library)
    assert table <= alogns and {8, 9, 10} <= table                     # N = 256, 512, 1024 must be built
    for n in (128,) + SIZES + (8192,):
        assert (_supported(lib, lib.MtmParams(n=n, w=2.5, kmax=4)) == OK) == (n.bit_length() - 1 in table), n
    # no new object in the Makefile's OBJS, and none written into it as a spectro16 term
    assert "jackknife" not in re.search(r"^OBJS\s*=(.*?)\n\n", mk, re.M | re.S).group(1)


# (1 + level) / 2, nu = K - 1, t
STUDENT = ((0.975, 1, 12.706204736), (0.975, 4, 2.776445105), (0.975, 7, 2.364624252), (0.95, 2, 2.919985580), (0.995, 3, 5.840909310))


def test_jackknife_factor(lib):
    L = lib.api.lib()
    t = C.c_double(-1.0)
    for q, nu, want in STUDENT:
        params = lib.MtmParams(n=1024, w=4.5, kmax=nu)
        cfg = lib.api.make_config(params)
        assert L.glfer_hip_jackknife_factor(C.byref(cfg), 2.0 * q - 1.0, C.byref(t)) == OK
        assert abs(t.value / want - 1.0) <= 1e-9, (q, nu, t.value)
        assert abs(lib.jackknife_factor(params, 2.0 * q - 1.0) / want - 1.0) <= 1e-9
    # rises with the level, falls with the taper count, and the default level is 0.95
    p4 = lib.MtmParams(n=512, w=2.5, kmax=4)
    assert lib.jackknife_factor(p4, 0.5) < lib.jackknife_factor(p4, 0.9) < lib.jackknife_factor(p4) < lib.jackknife_factor(p4, 0.999)
    assert lib.jackknife_factor(p4) == lib.jackknife_factor(p4, 0.95)
    assert lib.jackknife_factor(lib.MtmParams(n=512, w=4.5, kmax=7)) < lib.jackknife_factor(p4)
    assert abs(lib.jackknife_factor(lib.MtmParams(n=512, w=2.0, kmax=1), 0.5) - 1.0) <= 1e-12     # Cauchy: the quartile is 1
    # refusals: the level outside (0, 1), no output, plans that are not supported
    cfg = lib.api.make_config(p4)
    for level in (0.0, 1.0, -0.5, 1.5, float("nan"), float("inf")):
        t.value = -1.0
        assert L.glfer_hip_jackknife_factor(C.byref(cfg), level, C.byref(t)) == E_ARG, level
        assert t.value == -1.0
    assert L.glfer_hip_jackknife_factor(C.byref(cfg), 0.95, None) == E_ARG
    assert L.glfer_hip_jackknife_factor(None, 0.95, C.byref(t)) == E_ARG
    for params in (lib.MtmParams(n=8192, w=2.5, kmax=4), lib.MtmParams(n=1024, w=2.0, kmax=0), lib.MtmParams(n=1024, w=6.0, kmax=8),
                   lib.FftParams(n=1024, window_type=0, overlap=0.5)):
        bad = lib.api.make_config(params)
        assert L.glfer_hip_jackknife_factor(C.byref(bad), 0.95, C.byref(t)) == E_ARG
        with pytest.raises(lib.GlferHipError):
            lib.jackknife_factor(params)


def _plan(lib, params):
    """A plan where one can be made (a plan needs a device for its tables), else None."""
    L = lib.api.lib()
    cfg = lib.api.make_config(params)
    h = C.c_void_p()
    return h if L.glfer_hip_plan_create(C.byref(cfg), C.byref(h)) == 0 else None


def device_entry_refusals(lib):
    """Every refusal of the two device entries that needs a plan; shared with tests/test_gpu_jackknife.py.  The buffers are fake
    addresses: a refusal must come before anything reads them or is launched.  Returns the number of plans it could make."""
    L = lib.api.lib()
    one, many = L.glfer_hip_mtm_jackknife_device, L.glfer_hip_mtm_jackknife_batch_device
    made = 0
    fake, o1, o2, o3 = 0x10000, 0x4000000, 0x5000000, 0x6000000
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
                assert one(h, fake, ns, 0, 4, o1, o2, o3, pitch, 8, None) == E_ARG
                assert many(h, fake, 2, ns, ns, 0, 4, o1, o2, o3, pitch, 8, None) == E_ARG
            for iters in (-1, 65, 1 << 20, -(1 << 31)):                                     # sweeps outside 0 .. 64
                assert one(h, fake, ns, 0, 4, o1, o2, o3, 0, iters, None) == E_ARG
                assert many(h, fake, 2, ns, ns, 0, 4, o1, o2, o3, 0, iters, None) == E_ARG
                assert one(h, None, ns, 0, 0, None, None, None, 0, iters, None) == E_ARG    # (refused even with no work)
            for iters in (0, 8):
                assert one(h, fake, ns, 0, 4, None, None, None, 0, iters, None) == E_ARG    # all three outputs NULL
                assert many(h, fake, 2, ns, ns, 0, 4, None, None, None, 0, iters, None) == E_ARG
            for off in range(1, csz):                                                       # off one sample
                assert one(h, fake + off, ns, 0, 4, o1, o2, o3, 0, 8, None) == E_ARG
                assert many(h, fake + off, 2, ns, ns, 0, 4, o1, o2, o3, 0, 8, None) == E_ARG
            assert one(h, fake, ns, 7, 4, o1, None, None, 0, 8, None) == E_ARG              # a frame past the stream
            assert one(h, fake, ns, 10, 1, None, o2, None, 0, 0, None) == E_ARG
            assert one(h, fake, ns, 10, 1, None, None, o3, 0, 0, None) == E_ARG
            assert many(h, fake, 3, ns, ns, 7, 4, None, None, o3, 0, 8, None) == E_ARG
            assert one(h, fake, ns, 2 ** 64 - 2, 4, o1, o2, o3, 0, 8, None) == E_ARG        # first + nframes wraps
            assert many(h, fake, 2, ns, ns, 2 ** 64 - 2, 4, o1, o2, o3, 0, 8, None) == E_ARG
            assert one(h, fake, 2 ** 33 * hop, 0, 2 ** 31, o1, o2, o3, 0, 8, None) == E_ARG  # nframes > 0x7fffffff
            assert many(h, fake, 2, 2 ** 33 * hop, 2 ** 33 * hop, 0, 2 ** 31, o1, o2, o3, 0, 8, None) == E_ARG
            assert one(h, None, ns, 0, 4, o1, o2, o3, 0, 8, None) == E_ARG                  # no input while there is work
            assert many(h, None, 2, ns, ns, 0, 4, o1, o2, o3, 0, 0, None) == E_ARG
            assert many(h, fake, 2 ** 40, 2 ** 40, ns, 0, 4, o1, o2, o3, 0, 8, None) == E_ARG   # sizes that overflow size_t
            assert one(h, None, ns, 0, 0, None, None, None, 0, 8, None) == OK               # no frames: nothing to do
            assert one(h, None, ns, 99, 0, None, None, None, bins + 8, 0, None) == OK
            assert many(h, None, 0, ns, ns, 0, 4, None, None, None, 0, 64, None) == OK      # no streams
            assert many(h, None, 5, ns, ns, 0, 0, None, None, None, 0, 0, None) == OK
            assert one(None, fake, ns, 0, 4, o1, o2, o3, 0, 8, None) == E_ARG
        finally:
            L.glfer_hip_plan_destroy(h)
    # plans that make no jackknife rows: one window or one taper, nine tapers, other modes, other N, mean removal
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
            assert one(h, fake, ns, 0, 4, o1, o2, o3, 0, 8, None) == E_ARG
            assert many(h, fake, 2, ns, ns, 0, 4, o1, o2, o3, 0, 0, None) == E_ARG
            assert one(h, None, ns, 0, 0, None, None, None, 0, 8, None) == E_ARG            # (refused even with no work)
        finally:
            L.glfer_hip_plan_destroy(h)
    return made


def test_null_plan_and_device_entry_refusals(lib):
    L = lib.api.lib()
    fake = 0x10000
    assert L.glfer_hip_mtm_jackknife_device(None, fake, 4096, 0, 1, fake, None, None, 0, 8, None) == E_ARG
    assert L.glfer_hip_mtm_jackknife_device(None, None, 0, 0, 0, None, None, None, 0, 0, None) == E_ARG
    assert L.glfer_hip_mtm_jackknife_batch_device(None, fake, 2, 4096, 4096, 0, 1, None, None, fake, 0, 8, None) == E_ARG
    made = device_entry_refusals(lib)              # (a plan needs a device: 0 here without one)
    assert made in (0, 11)
