"""The waterfall of streams of unequal length in one call (-m gpu): glfer_hip_waterfall_ragged_device / waterfall_ragged
against a loop of glfer_hip_waterfall_device / waterfall over each stream's rows with a copy of its incoming Display -- rgb,
levbuf and floor statistics with torch.equal, the carried state with ==.
"""
import ctypes as C

import numpy as np
import pytest

from _ragged_cols import psd_rows, row_starts

pytestmark = pytest.mark.gpu
STATE = ("first_buffer", "display_max_lvl", "display_min_lvl")
# the four scale types (lin, lin max0, log, log max0), each with autoscale on and off
_AUTO = dict(autoscale=1, overlap=0.5)
_FIXED = dict(autoscale=0, max_level_db=-20.0, min_level_db=-80.0)
SCALES = {"lin_auto": dict(scale_type=0, autoscale=1, overlap=0.75, palette=3, thr_level=10.0),
          "lin_fixed": dict(scale_type=0, palette=2, max_level_db=-3.0, min_level_db=-40.0, autoscale=0),
          "linmax0_auto": dict(scale_type=1, palette=4, thr_level=10.0, **_AUTO),
          "linmax0_fixed": dict(scale_type=1, autoscale=0, max_level_db=-3.0, min_level_db=-40.0, palette=1),
          "log_auto": dict(scale_type=2, autoscale=1, overlap=0.5, palette=0),
          "log_fixed": dict(scale_type=2, palette=6, **_FIXED),
          "logmax0_auto": dict(scale_type=3, palette=1, thr_level=5.0, **_AUTO),
          "logmax0_fixed": dict(scale_type=3, autoscale=0, max_level_db=-20.0, min_level_db=-80.0, thr_level=5.0, palette=5)}
# LEV_CHUNK is 256 and the seeded warm-up starts past 1 280 columns: one and several level chunks, and a seeded one
LENGTHS = [0, 1, 255, 256, 257, 1281, 3000]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _disps(lib, nb, **kw):
    """nb Displays with the same options and different incoming states: every third stream a first buffer"""
    out = []
    for b in range(nb):
        d = lib.Display(first_buffer=1 if b % 3 == 0 else 0, **kw)
        if b % 3:
            scale = 10.0 ** ((b * 37) % 7 - 3)
            d.display_max_lvl = scale * (0.05 + 0.01 * (b % 5))
            d.display_min_lvl = scale * (0.002 + 0.0005 * (b % 4))
        out.append(d)
    return out


def _copy(lib, disps):
    return [lib.Display.from_buffer_copy(d) for d in disps]


def _state(d):
    return tuple(getattr(d, k) for k in STATE)


def _check(torch, lib, rows, starts, disps, want_lev=True, want_stats=True, **av):
    """waterfall_ragged against the loop; returns the ragged call's outputs and displays"""
    loop_d, rag_d = _copy(lib, disps), _copy(lib, disps)
    rgb, lev, stats, got = lib.waterfall_ragged(rag_d, rows, starts, want_lev=want_lev, want_stats=want_stats, **av)
    assert list(got) == list(starts) and (lev is None) == (not want_lev) and (stats is None) == (not want_stats)
    for b in range(len(starts) - 1):
        lo, hi = int(starts[b]), int(starts[b + 1])
        if lo == hi:
            assert bytes(rag_d[b]) == bytes(disps[b]), b                       # a stream without rows: untouched
            continue
        w_rgb, w_lev, w_stats = lib.waterfall(loop_d[b], rows[lo:hi], want_stats=True, **av)
        assert torch.equal(rgb[lo:hi], w_rgb), (b, hi - lo)
        if want_lev:
            assert torch.equal(lev[lo:hi], w_lev), (b, hi - lo)
        if want_stats:
            assert torch.equal(stats[lo:hi].view(torch.int32), w_stats.view(torch.int32)), (b, hi - lo)
        assert _state(rag_d[b]) == _state(loop_d[b]), b
    return rgb, lev, stats, rag_d


def _av(mode, bins, depth=4):
    if mode == 0:
        return dict(avg_mode=0)
    return {1: dict(avg_mode=1, depth=depth, minbin=10, maxbin=bins - 13), 2: dict(avg_mode=2, depth=depth, minbin=0, maxbin=bins),
            3: dict(avg_mode=3, depth=depth + 3, minbin=3, maxbin=bins - 2)}[mode]


_ROWS = {}


def _rows(torch, bins):
    if bins not in _ROWS:
        _ROWS[bins] = psd_rows(torch, LENGTHS, bins, seed=7 + bins)
    return _ROWS[bins]


@pytest.mark.parametrize("scale", sorted(SCALES))
@pytest.mark.parametrize("mode", [0, 1, 2, 3])
@pytest.mark.parametrize("bins", [513, 2049])
def test_waterfall_ragged_modes_scales(torch_cuda, lib, bins, mode, scale):
    for max0 in ((0, 1) if mode else (0,)):
        _check(torch_cuda, lib, _rows(torch_cuda, bins), row_starts(LENGTHS), _disps(lib, len(LENGTHS), **SCALES[scale]),
               max0=max0, **_av(mode, bins))


@pytest.mark.parametrize("want_lev,want_stats", [(False, False), (True, False), (False, True)])
def test_waterfall_ragged_optional_outputs(torch_cuda, lib, want_lev, want_stats):
    for mode in (0, 2):
        _check(torch_cuda, lib, _rows(torch_cuda, 513), row_starts(LENGTHS), _disps(lib, len(LENGTHS), **SCALES["log_auto"]),
               want_lev=want_lev, want_stats=want_stats, **_av(mode, 513))


@pytest.mark.parametrize("scale", ["log_auto", "lin_auto", "log_fixed"])
def test_waterfall_ragged_continues_across_calls(torch_cuda, lib, scale):
    """two ragged calls in sequence with the carried state equal one single-stream call per stream over the concatenation"""
    torch = torch_cuda
    first, second = [300, 0, 1, 700], [400, 5, 0, 257]
    bins = 513
    a = psd_rows(torch, first, bins, seed=13)
    b = psd_rows(torch, second, bins, seed=14)
    sa, sb = row_starts(first), row_starts(second)
    disps = _disps(lib, 4, **SCALES[scale])
    one = _copy(lib, disps)
    ra = lib.waterfall_ragged(disps, a, sa)
    rb = lib.waterfall_ragged(disps, b, sb)
    torch.cuda.synchronize()
    for s in range(4):
        whole = torch.cat([a[sa[s]:sa[s + 1]], b[sb[s]:sb[s + 1]]]).contiguous()
        w_rgb, w_lev, _ = lib.waterfall(one[s], whole)
        assert torch.equal(torch.cat([ra[0][sa[s]:sa[s + 1]], rb[0][sb[s]:sb[s + 1]]]), w_rgb), s
        assert torch.equal(torch.cat([ra[1][sa[s]:sa[s + 1]], rb[1][sb[s]:sb[s + 1]]]), w_lev), s
        assert _state(disps[s]) == _state(one[s]), s


@pytest.mark.parametrize("mode", [1, 2, 3])
def test_waterfall_ragged_staged_route(torch_cuda, lib, monkeypatch, mode):
    monkeypatch.setenv("GLFER_WATERFALL_FUSED", "0")
    _check(torch_cuda, lib, _rows(torch_cuda, 513), row_starts(LENGTHS), _disps(lib, len(LENGTHS), **SCALES["log_auto"]),
           **_av(mode, 513))


@pytest.mark.parametrize("mode", [1, 2])
def test_waterfall_ragged_deep_window_two_classes(torch_cuda, lib, mode):
    """depth 40: the short streams (chunks of 8 and 16 frames) take the staged class, the long one (chunks of 32) the fused"""
    torch = torch_cuda
    lengths = [100, 0, 3000, 17000, 40000]
    rows = psd_rows(torch, lengths, 129, seed=23)
    _check(torch, lib, rows, row_starts(lengths), _disps(lib, len(lengths), **SCALES["log_auto"]), **_av(mode, 129, depth=40))


@pytest.mark.parametrize("mode", [0, 2])
@pytest.mark.parametrize("fused", ["1", "0"])
def test_waterfall_ragged_tiles_fall_back_stream_by_stream(torch_cuda, lib, monkeypatch, mode, fused):
    monkeypatch.setenv("GLFER_WATERFALL_FUSED", fused)
    monkeypatch.setenv("GLFER_WATERFALL_TILE", "64")
    torch = torch_cuda
    lengths = [300, 0, 20, 64]
    rows = psd_rows(torch, lengths, 513, seed=29)
    _check(torch, lib, rows, row_starts(lengths), _disps(lib, len(lengths), **SCALES["lin_auto"]), **_av(mode, 513))


def test_waterfall_ragged_pitched_rows(torch_cuda, lib):
    """psd_pitch 2112 at 2049 bins: the rows of a run_ragged call on a pitched plan, mapped where they lie"""
    torch = torch_cuda
    bins, pitch = 2049, 2112
    sp = lib.Spectrogram(lib.FftParams(n=4096, window_type=7, overlap=0.5, psd_pitch=pitch))
    assert sp.bins == bins and sp.pitch == pitch
    lens = [40 * sp.hop + 3, sp.hop - 1, 300 * sp.hop, 7 * sp.hop]
    offs, at = [], 0
    for n in lens:
        offs.append(at)
        at += n + 4
    g = torch.Generator(device="cuda:0").manual_seed(37)
    x = torch.randn(at, generator=g, device="cuda:0", dtype=torch.float32) * 0.05
    psd, starts = sp.run_ragged(x, offs, lens)
    assert psd.shape == (int(starts[-1]), pitch)
    psd[:, bins:] = -7.25                                                      # the padding is never read
    L = lib.api.lib()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rows = int(starts[-1])
    for mode in (0, 2, 1):
        av = _av(mode, bins)
        args = (av["avg_mode"], av.get("depth", 1), av.get("minbin", 0), av.get("maxbin", 1), 0)
        disps = _disps(lib, len(lens), psd_pitch=pitch, **SCALES["log_auto"])
        loop_d, rag_d = _copy(lib, disps), _copy(lib, disps)
        w_rgb = torch.empty((rows, bins, 3), dtype=torch.uint8, device="cuda:0")
        w_lev = torch.empty((rows, bins), dtype=torch.int16, device="cuda:0")
        for b in range(len(lens)):
            lo, hi = int(starts[b]), int(starts[b + 1])
            if hi > lo:
                assert L.glfer_hip_waterfall_device(C.byref(loop_d[b]), *args, psd[lo:].data_ptr(), hi - lo, bins, w_rgb[lo:].data_ptr(),
                                                    w_lev[lo:].data_ptr(), None, st) == 0
        rgb, lev, _, _ = lib.waterfall_ragged(rag_d, psd[:, :bins], starts, **av)
        torch.cuda.synchronize()
        assert torch.equal(rgb, w_rgb) and torch.equal(lev, w_lev), mode
        for b in range(len(lens)):
            assert _state(rag_d[b]) == _state(loop_d[b]), (mode, b)


def test_waterfall_ragged_argument_errors(torch_cuda, lib):
    torch = torch_cuda
    L = lib.api.lib()
    lengths = [4, 0, 6]
    rows = psd_rows(torch, lengths, 129, seed=19)
    good = row_starts(lengths).astype(np.uint64)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rgb = torch.full((10, 129, 3), 77, dtype=torch.uint8, device="cuda:0")
    sentinel = rgb.clone()

    def call(arr, starts=good, nstreams=3, av=(0, 1, 0, 1), bins=129, stream=st, out=rgb):
        return L.glfer_hip_waterfall_ragged_device(arr, nstreams, av[0], av[1], av[2], av[3], 0, rows.data_ptr(),
                                                   starts.ctypes.data if starts is not None else None, bins,
                                                   out.data_ptr() if out is not None else None, None, None, stream)

    for field, value in (("scale_type", 3), ("autoscale", 0), ("overlap", 0.25), ("max_level_db", -11.0), ("min_level_db", -61.0),
                         ("thr_level", 1.0), ("palette", 2), ("psd_pitch", 130)):
        disps = _disps(lib, 3, **SCALES["log_auto"])
        setattr(disps[2], field, value)
        arr = (lib.Display * 3)(*_copy(lib, disps))
        assert call(arr) == -1, field
        assert [bytes(d) for d in arr] == [bytes(d) for d in disps], field
    disps = _disps(lib, 3, **SCALES["log_auto"])
    arr = (lib.Display * 3)(*_copy(lib, disps))
    assert call(arr, nstreams=0) == 0
    assert call(arr, starts=np.zeros(4, np.uint64)) == 0                       # no rows at all
    assert call(None) == -1 and call(arr, starts=None) == -1 and call(arr, out=None) == -1
    assert call(arr, starts=np.array([0, 6, 4, 10], np.uint64)) == -1          # decreasing
    # the single-stream entry's rules: a bad band, mode or depth, no bins
    assert call(arr, av=(2, 4, 0, 130)) == -1 and call(arr, av=(4, 4, 0, 129)) == -1 and call(arr, av=(2, 0, 0, 129)) == -1
    assert call(arr, bins=0) == -1
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        rc = call(arr, stream=C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == -1
    assert torch.equal(rgb, sentinel)                                          # nothing launched
    assert [bytes(d) for d in arr] == [bytes(d) for d in disps]
    assert call(arr) == 0
    torch.cuda.synchronize()
    assert bytes(arr[1]) == bytes(disps[1]) and arr[0].first_buffer == 0 and arr[2].first_buffer == 0


def test_waterfall_ragged_wrapper_refusals(torch_cuda, lib):
    torch = torch_cuda
    rows = psd_rows(torch, [3, 5], 129, seed=43)
    two = _disps(lib, 2, **SCALES["log_auto"])
    with pytest.raises(ValueError):
        lib.waterfall_ragged(two, rows.double(), [0, 3, 8])
    with pytest.raises(ValueError):
        lib.waterfall_ragged(two, rows.reshape(-1), [0, 3, 8])
    with pytest.raises(ValueError):
        lib.waterfall_ragged(two[:1], rows, [0, 3, 8])
    with pytest.raises(ValueError):
        lib.waterfall_ragged(two, rows[:, :100], [0, 3, 8])                    # rows apart by more than their length, no psd_pitch
    with pytest.raises(ValueError):
        lib.update_avg_ragged(2, rows[:, :100], [0, 3, 8], 4, 0, 100)
    with pytest.raises(ValueError):
        lib.update_avg_ragged(2, rows, [0, 3, 9], 4, 0, 129)
    assert [_state(d) for d in two] == [_state(d) for d in _disps(lib, 2, **SCALES["log_auto"])]
