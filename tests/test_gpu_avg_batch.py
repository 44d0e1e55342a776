"""The moving average of many streams per call (-m gpu): glfer_hip_avg_batch_device / update_avg_batch and
glfer_hip_spectrogram_avg_batch_device / Spectrogram.run_avg_batch against a loop of the single-stream entries over the
same streams, double for double with torch.equal.

The streams of a batch differ in seed, amplitude and DC level, so that a row or an averaging window taken from the wrong
stream cannot come out equal by accident.
"""
import ctypes as C

import numpy as np
import pytest

from _signals import synth

pytestmark = pytest.mark.gpu
HANNING = 0


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _streams(torch, lib, fmt, nb, nsamples):
    """[nb, nsamples] of the plan's sample type, one seed, amplitude and DC level per stream (an even pitch for integers)."""
    pitch = nsamples + (nsamples & 1 if fmt != lib.SAMPLES_F32 else 0)
    out = np.zeros((nb, pitch), np.float64)
    for b in range(nb):
        amp = 0.4 + 0.6 * ((b * 7919) % 11) / 10.0
        dc = 0.05 * (((b * 104729) % 9) - 4)
        out[b, :nsamples] = amp * synth(nsamples, seed=2000 + b) + dc
    if fmt == lib.SAMPLES_F32:
        buf = out.astype(np.float32)
    elif fmt == lib.SAMPLES_S16:
        buf = np.clip(np.round(out * 20000.0), -32768, 32767).astype(np.int16)
    else:
        buf = np.clip(np.round(128.0 + out * 90.0), 0, 255).astype(np.uint8)
    return torch.from_numpy(buf).to("cuda:0")[:, :nsamples]


def _rows(torch, nb, nframes, bins, seed=7):
    """PSD-like rows: non-negative floats, a different scale and floor per stream."""
    g = torch.Generator(device="cuda:0").manual_seed(seed)
    x = torch.rand((nb, nframes, bins), generator=g, device="cuda:0", dtype=torch.float32)
    scale = torch.tensor([10.0 ** ((b * 37) % 7 - 3) for b in range(nb)], device="cuda:0", dtype=torch.float32)
    floor = torch.tensor([0.01 * ((b * 13) % 5) for b in range(nb)], device="cuda:0", dtype=torch.float32)
    return (x * x * scale[:, None, None] + floor[:, None, None]).contiguous()


def _avg_loop(lib, mode, rows, depth, minbin, maxbin, max0, n_out):
    outs = [lib.update_avg(mode, rows[b], depth, minbin, maxbin, max0=max0, n_out=n_out) for b in range(rows.size(0))]
    return outs


def _check_avg_batch(torch, lib, mode, rows, depth, minbin, maxbin, max0=0, n_out=None):
    avg, ret = lib.api.update_avg_batch(mode, rows, depth, minbin, maxbin, max0=max0, n_out=n_out)
    want = _avg_loop(lib, mode, rows, depth, minbin, maxbin, max0, n_out)
    torch.cuda.synchronize()
    for b, (wa, wr) in enumerate(want):
        assert torch.equal(avg[b], wa), b
        for c in range(4):
            assert torch.equal(ret[b, :, c], wr[:, c]), (b, c)
    return avg, ret


# ---- 1. glfer_hip_avg_batch_device against a loop of glfer_hip_avg_device

@pytest.mark.parametrize("depth", [1, 3, 4, 7, 20])          # 40 frames: 8-frame chunks, so depth 20 takes the two-pass form
@pytest.mark.parametrize("max0", [0, 1])
@pytest.mark.parametrize("mode", [1, 2, 3])
def test_avg_batch_modes_depths(torch_cuda, lib, mode, max0, depth):
    rows = _rows(torch_cuda, 3, 40, 513, seed=depth)
    _check_avg_batch(torch_cuda, lib, mode, rows, depth, 0, 513, max0=max0)


@pytest.mark.parametrize("nb", [1, 3, 37])
@pytest.mark.parametrize("band", ["full", "default", "wide"])
def test_avg_batch_bands_sizes(torch_cuda, lib, band, nb):
    if band == "full":
        bins, minbin, maxbin, n_out, nf = 2049, 0, 2049, None, 300
    elif band == "default":                                   # the reference's band, 34 .. 103, avgdata N wide
        bins, minbin, maxbin, n_out, nf = 513, 34, 103, 1024, 300
    else:                                                     # N = 32768 rows: more than 33 x 256 bins, the two-pass form
        bins, minbin, maxbin, n_out, nf = 16385, 0, 16385, None, 6
    rows = _rows(torch_cuda, nb, nf, bins, seed=nb)
    for mode in (1, 2, 3):
        _check_avg_batch(torch_cuda, lib, mode, rows, 4, minbin, maxbin, n_out=n_out)


@pytest.mark.parametrize("mode", [1, 2, 3])
def test_avg_batch_window_still_filling(torch_cuda, lib, mode):
    """nframes < depth: the effective depth grows to the end of every stream."""
    rows = _rows(torch_cuda, 5, 3, 257, seed=11)
    avg, ret = _check_avg_batch(torch_cuda, lib, mode, rows, 7, 0, 257)
    assert ret[:, :, 3].tolist() == [[1.0, 2.0, 3.0]] * 5


def test_avg_batch_long_streams_many_chunks(torch_cuda, lib):
    """Streams long enough for 128-frame chunks in both the ring and the no-ring forms, the chunk boundaries inside and at
    the ends of the streams."""
    rows = _rows(torch_cuda, 3, 131072 + 77, 129, seed=3)
    for depth in (4, 200):
        _check_avg_batch(torch_cuda, lib, 2, rows, depth, 0, 129)


# ---- 2. the averaging state restarts per stream

@pytest.mark.parametrize("depth", [4, 20])
@pytest.mark.parametrize("mode", [1, 2, 3])
def test_avg_state_restarts_per_stream(torch_cuda, lib, mode, depth):
    torch = torch_cuda
    rows = _rows(torch, 3, 40, 513, seed=5) * 1e3
    rows[1].zero_()
    avg, ret = lib.api.update_avg_batch(mode, rows.contiguous(), depth, 0, 513)
    z_avg, z_ret = lib.update_avg(mode, torch.zeros_like(rows[1]), depth, 0, 513)
    s2_avg, s2_ret = lib.update_avg(mode, rows[2].contiguous(), depth, 0, 513)
    torch.cuda.synchronize()
    same = lambda a, b: torch.equal(a.view(torch.int64), b.view(torch.int64))     # bit for bit: the all-zero stream's 0/0 is a NaN
    assert same(avg[1], z_avg) and same(ret[1], z_ret)
    assert same(avg[2], s2_avg) and same(ret[2], s2_ret)
    # what a call over the flattened rows gives instead: stream 1's windows start with stream 0's loud rows
    f_avg, _ = lib.update_avg(mode, rows.reshape(-1, 513), depth, 0, 513)
    torch.cuda.synchronize()
    assert not torch.equal(f_avg[40:80], z_avg)


# ---- 3. glfer_hip_spectrogram_avg_batch_device against a loop of glfer_hip_spectrogram_avg_device

C1 = lambda **k: dict(dict(kind="fft", n=1024, window_type=HANNING, overlap=0.5), **k)
C2 = lambda **k: dict(dict(kind="fft", n=4096, window_type=HANNING, overlap=0.75), **k)
C3 = lambda **k: dict(dict(kind="mtm", n=4096, overlap=0.0, w=2.5, kmax=4), **k)
C4 = lambda **k: dict(dict(kind="mtm", n=16384, overlap=0.0, w=4.5, kmax=8), **k)


def _params(lib, spec):
    spec = dict(spec)
    kind = spec.pop("kind")
    return {"fft": lib.FftParams, "mtm": lib.MtmParams, "lmp": lib.LmpParams}[kind](**spec)


def _check_run_avg_batch(torch, lib, params, nb, nframes, mode=2, depth=4, band=None, n_out=None, max0=0):
    sp = lib.Spectrogram(params)
    hop = sp.hop
    x = _streams(torch, lib, params.sample_format, nb, nframes * hop + hop // 3)
    minbin, maxbin = band or (0, sp.bins)
    total = sp.num_frames(x.size(1))
    for first, nf in ((0, total), (total // 3, total - total // 3 - 1)):
        for want_psd, want_ret in ((True, True), (False, False)):
            kw = dict(max0=max0, n_out=n_out, want_psd=want_psd, want_ret=want_ret, first_frame=first, nframes=nf)
            avg, ret, psd = sp.run_avg_batch(x, mode, depth, minbin, maxbin, **kw)
            want = [sp.run_avg(x[b].contiguous(), mode, depth, minbin, maxbin, **kw) for b in range(nb)]
            torch.cuda.synchronize()
            assert (ret is None) == (not want_ret) and (psd is None) == (not want_psd)
            for b, (wa, wr, wp) in enumerate(want):
                assert torch.equal(avg[b], wa), (b, first, want_psd)
                if want_ret:
                    assert torch.equal(ret[b], wr), (b, first)
                if want_psd:
                    assert torch.equal(psd[b], wp), (b, first)
    sp.close()


# (params, streams, frames per stream)
CASES = {
    "C1": (C1(), 3, 40), "C2": (C2(), 3, 24), "C2_sub1": (C2(sub_mean=1), 3, 24), "C2_sub2": (C2(sub_mean=2), 3, 24),
    "C3": (C3(), 3, 12), "C4": (C4(), 3, 5),
    "fft_128": (dict(kind="fft", n=128, window_type=HANNING, overlap=0.5), 3, 50),      # below 256: rows stream by stream
    "fft_32768": (dict(kind="fft", n=32768, window_type=HANNING, overlap=0.5), 3, 4),   # above 16384: rows stream by stream
    "lmp": (dict(kind="lmp", n=1024, overlap=0.5, avg=4), 3, 20),
    "s16": (C2(sample_format=1), 3, 24), "u8": (C2(sample_format=2), 3, 24),
    "zero_always": (C2(history_mode=1), 3, 24),
    "C1_37": (C1(), 37, 40),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_run_avg_batch_equals_loop(torch_cuda, lib, name):
    spec, nb, nframes = CASES[name]
    _check_run_avg_batch(torch_cuda, lib, _params(lib, spec), nb, nframes)


@pytest.mark.parametrize("mode", [1, 3])
def test_run_avg_batch_other_modes(torch_cuda, lib, mode):
    _check_run_avg_batch(torch_cuda, lib, _params(lib, C2(sub_mean=1)), 3, 24, mode=mode, depth=7, band=(34, 103), n_out=4096, max0=1)


@pytest.mark.parametrize("depth", [2, 4])
@pytest.mark.parametrize("sub_mean", [0, 1])
def test_run_avg_batch_inside_the_launch(torch_cuda, lib, sub_mean, depth):
    """C2-shaped streams long enough that the average is taken inside the estimator launch (b0 + 256 <= end)."""
    _check_run_avg_batch(torch_cuda, lib, _params(lib, C2(sub_mean=sub_mean)), 3, 400, depth=depth)


def test_run_avg_batch_inside_the_launch_default_band(torch_cuda, lib):
    _check_run_avg_batch(torch_cuda, lib, _params(lib, C2(sub_mean=1)), 5, 400, band=(34, 103), n_out=4096)


# ---- 4. against the oracle's averager

def test_run_avg_batch_oracle(torch_cuda, lib, oracle):
    torch = torch_cuda
    sp = lib.Spectrogram(_params(lib, C2(sub_mean=1)))
    x = _streams(torch, lib, 0, 2, 400 * sp.hop)
    depth, minbin, maxbin, n_out = 4, 34, 103, 4096
    avg, ret, psd = sp.run_avg_batch(x, lib.AVG_PLAIN, depth, minbin, maxbin, n_out=n_out, want_psd=True)
    torch.cuda.synchronize()
    for b in range(2):
        a = oracle.Averager(n_out, depth)
        rows_h, avg_h, ret_h = psd[b].cpu().numpy(), avg[b].cpu().numpy(), ret[b].cpu().numpy()
        for f in range(40):
            r, want, peak, _ = a.update("plain", rows_h[f], minbin, maxbin, n=n_out)
            assert np.array_equal(avg_h[f], want), (b, f)
            assert ret_h[f, 1] == peak and np.isclose(ret_h[f, 0], r, rtol=1e-12), (b, f)
    sp.close()


# ---- 5. argument errors, empty calls

def test_avg_batch_bad_arguments(torch_cuda, lib):
    torch = torch_cuda
    L = lib.api.lib()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    x = torch.zeros((4, 8 * 4096), dtype=torch.int16, device="cuda:0")
    avg = torch.full((4, 8, 2049), 3.0, dtype=torch.float64, device="cuda:0")
    ret = torch.full((4, 8, 4), 3.0, dtype=torch.float64, device="cuda:0")

    def call(sp, nb=3, pitch=8 * 4096, nframes=4, band=(0, 2049), n_out=2049, first=0):
        return L.glfer_hip_spectrogram_avg_batch_device(sp._h, C.c_void_p(x.data_ptr()), nb, pitch, 8 * 4096, first, nframes, 2, 4,
                                                        band[0], band[1], 0, n_out, None, C.c_void_p(avg.data_ptr()),
                                                        C.c_void_p(ret.data_ptr()), st)
    s16 = lib.Spectrogram(_params(lib, C2(sample_format=1)))
    assert call(s16, pitch=8 * 4096 - 1) == -1                                   # odd pitch with s16 samples
    assert call(s16, band=(10, 10)) == -1 and call(s16, band=(0, 2050)) == -1    # bad bands
    assert call(s16, n_out=2048) == -1                                           # n_out < bins
    assert call(s16, nframes=33) == -1                                           # frame past the stream
    hp = lib.Spectrogram(lib.HparmaParams(n=4096, overlap=0.0, t=128, p_e=32, sample_format=1))
    assert call(hp) == -1                                                        # HP-ARMA
    padded = lib.Spectrogram(_params(lib, C2(sample_format=1, psd_pitch=2112)))
    assert call(padded) == -1                                                    # rows not dense
    assert call(s16, nb=0) == 0 and call(s16, nframes=0) == 0
    rows = torch.zeros((4, 8, 2049), dtype=torch.float32, device="cuda:0")
    acall = lambda nb, nf, band=(0, 2049), depth=4: L.glfer_hip_avg_batch_device(2, rows.data_ptr(), nb, nf, 2049, 2049, depth, band[0], band[1], 0,
                                                                                  avg.data_ptr(), ret.data_ptr(), st)
    assert acall(3, 8, band=(5, 5)) == -1 and acall(3, 8, depth=0) == -1
    assert acall(0, 8) == 0 and acall(3, 0) == 0
    torch.cuda.synchronize()
    assert bool((avg == 3.0).all()) and bool((ret == 3.0).all())                 # nothing was launched
    for sp in (s16, hp, padded):
        sp.close()


# ---- 6. more streams than the grid's y limit

def test_avg_batch_crosses_grid_y_limit(torch_cuda, lib):
    torch = torch_cuda
    nb = 70000
    rows = _rows(torch, nb, 4, 129, seed=9)
    avg, ret = lib.api.update_avg_batch(2, rows, 3, 0, 129)
    torch.cuda.synchronize()
    probe = sorted(set([0, 1, 65533, 65534, 65535, 65536, 65537, nb - 1] + list(np.random.default_rng(4).integers(0, nb, 48))))
    for b in probe:
        wa, wr = lib.update_avg(2, rows[b], 3, 0, 129)
        torch.cuda.synchronize()
        assert torch.equal(avg[b], wa) and torch.equal(ret[b], wr), b


# ---- 7. bench scale

def test_run_avg_batch_long_c2_streams(torch_cuda, lib):
    """16 C2-shaped streams of 65 536 frames with the reference's mean removal: every averaged row equal to the loop's."""
    torch = torch_cuda
    sp = lib.Spectrogram(_params(lib, C2(sub_mean=1)))
    nb, nframes = 16, 65536
    nsamples = (nframes + 3) * sp.hop
    g = torch.Generator(device="cuda:0").manual_seed(17)
    x = torch.randn((nb, nsamples), generator=g, device="cuda:0", dtype=torch.float32)
    x *= torch.linspace(0.2, 1.0, nb, device="cuda:0")[:, None]
    x += torch.linspace(-0.3, 0.3, nb, device="cuda:0")[:, None]
    avg, ret, _ = sp.run_avg_batch(x, lib.AVG_PLAIN, 4, 0, sp.bins, nframes=nframes)
    for b in range(nb):
        wa, wr, _ = sp.run_avg(x[b].contiguous(), lib.AVG_PLAIN, 4, 0, sp.bins, nframes=nframes)
        torch.cuda.synchronize()
        assert torch.equal(avg[b], wa) and torch.equal(ret[b], wr), b
        del wa, wr
    sp.close()
