"""The moving average of streams of unequal length in one call (-m gpu): glfer_hip_avg_ragged_device / update_avg_ragged and
glfer_hip_spectrogram_avg_ragged_device / Spectrogram.run_avg_ragged against a loop of the single-stream entries over each
stream's rows -- every double bit for bit (compared as int64: the variance of a frame without a counted bin is a NaN).
"""
import ctypes as C

import numpy as np
import pytest

from _ragged_cols import avg_chunk, psd_rows, row_starts, swinging_rows

pytestmark = pytest.mark.gpu

# an empty stream, a stream shorter than the deeper windows, the chunk edge at 8, several chunks
LENGTHS = [0, 1, 7, 8, 9, 255, 257, 3000]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _bits(t):
    import torch
    return t.contiguous().view(torch.int64)


def _check(torch, lib, psd, starts, mode, depth, minbin, maxbin, max0=0, n_out=None):
    avg, ret, got_starts = lib.update_avg_ragged(mode, psd, starts, depth, minbin, maxbin, max0, n_out)
    assert list(got_starts) == list(starts)
    assert avg.shape == (int(starts[-1]), n_out or psd.size(1)) and ret.shape == (int(starts[-1]), 4)
    for b in range(len(starts) - 1):
        lo, hi = int(starts[b]), int(starts[b + 1])
        if lo == hi:
            continue
        w_avg, w_ret = lib.update_avg(mode, psd[lo:hi], depth, minbin, maxbin, max0, n_out)
        assert torch.equal(_bits(avg[lo:hi]), _bits(w_avg)), (b, hi - lo)
        assert torch.equal(_bits(ret[lo:hi]), _bits(w_ret)), (b, hi - lo)


_ROWS = {}


def _rows(torch, bins):
    if bins not in _ROWS:
        _ROWS[bins] = psd_rows(torch, LENGTHS, bins, seed=3 + bins)
    return _ROWS[bins]


@pytest.mark.parametrize("depth", [1, 4, 20])
@pytest.mark.parametrize("max0", [0, 1])
@pytest.mark.parametrize("mode", [1, 2, 3])
@pytest.mark.parametrize("bins", [65, 2049])
def test_avg_ragged_equals_single_calls(torch_cuda, lib, bins, mode, max0, depth):
    _check(torch_cuda, lib, _rows(torch_cuda, bins), row_starts(LENGTHS), mode, depth, 0, bins, max0)


@pytest.mark.parametrize("mode", [1, 2, 3])
@pytest.mark.parametrize("bins,minbin,maxbin,n_out", [(65, 5, 60, 80), (2049, 100, 2000, 2100)])
def test_avg_ragged_sub_band_and_wide_output(torch_cuda, lib, bins, minbin, maxbin, n_out, mode):
    for depth in (4, 20):
        _check(torch_cuda, lib, _rows(torch_cuda, bins), row_starts(LENGTHS), mode, depth, minbin, maxbin, 0, n_out)


def test_avg_ragged_8193_bins(torch_cuda, lib):
    lengths = [0, 9, 300]
    psd = psd_rows(torch_cuda, lengths, 8193, seed=5)
    _check(torch_cuda, lib, psd, row_starts(lengths), 2, 4, 0, 8193)
    _check(torch_cuda, lib, psd, row_starts(lengths), 1, 20, 3, 8190, 1)


@pytest.mark.parametrize("mode", [1, 2, 3])
def test_avg_ragged_two_classes_in_one_call(torch_cuda, lib, mode):
    """depth 20: streams under 16 384 frames have chunk 8 and take the two-pass form, streams from 16 384 have chunk 16 and
    take the fused one -- both in one call"""
    lengths = [100, 16383, 16384, 20000]
    assert [avg_chunk(n) for n in lengths] == [8, 8, 16, 16]
    psd = psd_rows(torch_cuda, lengths, 65, seed=9)
    _check(torch_cuda, lib, psd, row_starts(lengths), mode, 20, 0, 65)


@pytest.mark.parametrize("depth", [4, 6])
def test_avg_ragged_takes_each_streams_own_chunk(torch_cuda, lib, depth):
    """Rows that swing by more than 2^26 inside a window: the window sums are inexact, and where a chunk restarts shows in the
    last bits (tests/test_avg_ragged_host.py checks that on the CPU for this very input).  The three streams have
    single-entry chunks of 8, 16 and 32.  At depth 4 the fused kernel sums the window directly, whatever the chunk; depth 6
    is the recurrence with its restarts."""
    torch = torch_cuda
    lengths = [40, 16400, 40000]
    assert [avg_chunk(n) for n in lengths] == [8, 16, 32]
    psd = torch.from_numpy(swinging_rows(sum(lengths), 65, seed=21)).cuda()
    for mode in (2, 1):
        _check(torch, lib, psd, row_starts(lengths), mode, depth, 0, 65)


def _samples(torch, lib, fmt, total, seed):
    rng = np.random.default_rng(seed)
    if fmt == lib.SAMPLES_F32:
        return torch.from_numpy((rng.standard_normal(total) * 0.1 + 0.02).astype(np.float32)).cuda()
    return torch.from_numpy(rng.integers(-3000, 3000, total).astype(np.int16)).cuda()


@pytest.mark.parametrize("want_psd", [False, True])
@pytest.mark.parametrize("sub_mean", [0, 1])
@pytest.mark.parametrize("fmt", ["f32", "s16"])
@pytest.mark.parametrize("kind", ["fft", "mtm"])
def test_run_avg_ragged_equals_run_then_update_avg(torch_cuda, lib, kind, fmt, sub_mean, want_psd):
    torch = torch_cuda
    fmt = lib.SAMPLES_F32 if fmt == "f32" else lib.SAMPLES_S16
    if kind == "fft":
        params = lib.FftParams(n=1024, window_type=7, overlap=0.5, sub_mean=sub_mean, sample_format=fmt)
    else:
        params = lib.MtmParams(n=1024, sub_mean=sub_mean, sample_format=fmt)
    sp = lib.Spectrogram(params)
    # 0.3 .. 1.7 s at 48 kHz, some a whole number of hops and some not, and one shorter than a hop
    lens = [int(0.3 * 48000), (int(0.6 * 48000) // sp.hop) * sp.hop, sp.hop // 2, int(0.9 * 48000) | 1,
            (int(1.2 * 48000) // sp.hop) * sp.hop, int(1.7 * 48000)]
    offs, at = [], 6
    for n in lens:
        offs.append(at)
        at += n + 10 + (n & 1)                                             # even offsets (s16), gaps between the streams
    x = _samples(torch, lib, fmt, at, seed=31)
    for mode, depth, minbin, maxbin, max0, n_out in ((2, 4, 0, sp.bins, 0, None), (1, 3, 7, 500, 1, sp.bins + 30)):
        avg, ret, psd, starts = sp.run_avg_ragged(x, offs, lens, mode, depth, minbin, maxbin, max0, n_out, want_psd=want_psd)
        assert list(starts) == list(row_starts([n // sp.hop for n in lens]))
        assert (psd is not None) == want_psd
        for b, (o, n) in enumerate(zip(offs, lens)):
            lo, hi = int(starts[b]), int(starts[b + 1])
            if lo == hi:
                continue
            w_psd = sp.run(x[o:o + n])
            w_avg, w_ret = lib.update_avg(mode, w_psd, depth, minbin, maxbin, max0, n_out)
            assert torch.equal(_bits(avg[lo:hi]), _bits(w_avg)), (mode, b)
            assert torch.equal(_bits(ret[lo:hi]), _bits(w_ret)), (mode, b)
            if want_psd:
                assert torch.equal(psd[lo:hi], w_psd), (mode, b)
        avg2, ret2, _, _ = sp.run_avg_ragged(x, offs, lens, mode, depth, minbin, maxbin, max0, n_out, want_psd=want_psd,
                                             want_ret=False)
        assert ret2 is None and torch.equal(_bits(avg2), _bits(avg))


def test_avg_ragged_refusals(torch_cuda, lib):
    torch = torch_cuda
    L = lib.api.lib()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    lengths = [3, 0, 5]
    psd = psd_rows(torch, lengths, 65, seed=41)
    avg = torch.full((8, 65), -3.5, dtype=torch.float64, device="cuda:0")
    ret = torch.full((8, 4), -3.5, dtype=torch.float64, device="cuda:0")
    good = row_starts(lengths).astype(np.uint64)

    def call(starts, stream=st, nstreams=3, mode=2, depth=4, maxbin=65):
        return L.glfer_hip_avg_ragged_device(mode, psd.data_ptr(), nstreams, starts.ctypes.data if starts is not None else None, 65, 65,
                                             depth, 0, maxbin, 0, avg.data_ptr(), ret.data_ptr(), stream)

    assert call(np.array([0, 5, 3, 8], np.uint64)) == -1                   # decreasing
    assert call(None) == -1                                                # no table
    assert call(good, mode=0) == -1 and call(good, depth=0) == -1 and call(good, maxbin=66) == -1
    assert call(None, nstreams=0) == 0                                     # nothing to do
    assert call(np.zeros(4, np.uint64)) == 0                               # no rows at all
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        capturing = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        rc = call(good, stream=capturing)
    torch.cuda.synchronize()
    assert rc == -1
    assert bool((avg == -3.5).all()) and bool((ret == -3.5).all())
    assert call(good) == 0                                                 # outside a capture: as ever
    torch.cuda.synchronize()
    assert bool((avg[:3] != -3.5).all()) and bool((avg[3:] != -3.5).all())


def test_run_avg_ragged_refusals(torch_cuda, lib):
    torch = torch_cuda
    L = lib.api.lib()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    sp = lib.Spectrogram(lib.FftParams(n=1024, window_type=7, overlap=0.5, sample_format=lib.SAMPLES_S16))
    x = torch.zeros(80 * sp.hop, dtype=torch.int16, device="cuda:0")
    avg = torch.full((16, sp.bins), -3.5, dtype=torch.float64, device="cuda:0")
    lens = np.array([4 * sp.hop, 6 * sp.hop], np.uint64)
    starts = np.full(3, 99, np.uint64)

    def call(plan, offs, stream=st, n_out=None, depth=4):
        offs = np.asarray(offs, np.uint64)
        return L.glfer_hip_spectrogram_avg_ragged_device(plan._h, x.data_ptr(), 2, offs.ctypes.data, lens.ctypes.data, 2, depth, 0,
                                                         plan.bins, 0, n_out or plan.bins, None, avg.data_ptr(), None,
                                                         starts.ctypes.data, stream)

    assert call(sp, [0, 4 * sp.hop + 1]) == -1                             # an odd s16 offset
    assert call(sp, [0, 4 * sp.hop], n_out=sp.bins - 1) == -1 and call(sp, [0, 4 * sp.hop], depth=0) == -1
    hp = lib.Spectrogram(lib.HparmaParams(n=4096, overlap=0.0, t=128, p_e=32, sample_format=lib.SAMPLES_S16))
    assert call(hp, [0, 4 * hp.hop]) == -1                                 # HP-ARMA rows are not averaged
    pitched = lib.Spectrogram(lib.FftParams(n=1024, overlap=0.5, sample_format=lib.SAMPLES_S16, psd_pitch=576))
    assert call(pitched, [0, 4 * sp.hop]) == -1                            # dense rows only
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        rc = call(sp, [0, 4 * sp.hop], stream=C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == -1
    assert bool((avg == -3.5).all())
    zero_offs = np.zeros(2, np.uint64)
    null_avg = L.glfer_hip_spectrogram_avg_ragged_device(sp._h, x.data_ptr(), 2, zero_offs.ctypes.data, lens.ctypes.data, 2, 4,
                                                         0, sp.bins, 0, sp.bins, None, None, None, starts.ctypes.data, st)
    assert null_avg == -1
    assert list(starts) == [99, 99, 99]                                    # no refusal wrote row_starts
    assert call(sp, [0, 4 * sp.hop]) == 0
    torch.cuda.synchronize()
    assert list(starts) == [0, 4, 10] and bool((avg[:10] != -3.5).all()) and bool((avg[10:] == -3.5).all())
