"""The waterfall of many streams per call (-m gpu): glfer_hip_waterfall_batch_device / waterfall_batch against a loop of
glfer_hip_waterfall_device / waterfall over the same streams, each with a copy of its incoming Display -- rgb, levbuf and
floor statistics with torch.equal, the carried state with ==.

The streams of a batch differ in scale, floor and seed, and their incoming states differ (first buffers and carried levels),
so that a column, a level or a state taken from the wrong stream cannot come out equal by accident.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
STATE = ("first_buffer", "display_max_lvl", "display_min_lvl")
SCALES = {"log_auto": dict(scale_type=2, autoscale=1, overlap=0.5, palette=0),
          "lin_auto": dict(scale_type=0, autoscale=1, overlap=0.75, palette=3, thr_level=10.0),
          "log_fixed": dict(scale_type=3, autoscale=0, max_level_db=-20.0, min_level_db=-80.0, thr_level=5.0, palette=5),
          "linmax0_fixed": dict(scale_type=1, autoscale=0, max_level_db=-3.0, min_level_db=-40.0, palette=1)}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _rows(torch, nb, nframes, bins, seed=7, pitch=None):
    """PSD-like rows: non-negative floats, a different scale and floor per stream; [nb][nframes][pitch or bins]."""
    width = pitch or bins
    g = torch.Generator(device="cuda:0").manual_seed(seed)
    x = torch.rand((nb, nframes, width), generator=g, device="cuda:0", dtype=torch.float32)
    scale = torch.tensor([10.0 ** ((b * 37) % 7 - 3) for b in range(nb)], device="cuda:0", dtype=torch.float32)
    floor = torch.tensor([1e-4 * ((b * 13) % 5) for b in range(nb)], device="cuda:0", dtype=torch.float32)
    return (x * x * x * x * scale[:, None, None] + floor[:, None, None]).contiguous()


def _disps(lib, nb, **kw):
    """nb Displays with the same options and different incoming states: every third stream a first buffer, the others
    carried levels of their own."""
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


def _check(torch, lib, rows, disps, **av):
    """waterfall_batch against the loop; returns the batch's outputs."""
    loop_d, batch_d = _copy(lib, disps), _copy(lib, disps)
    want = [lib.waterfall(loop_d[b], rows[b], want_stats=True, **av) for b in range(rows.size(0))]
    rgb, lev, stats = lib.waterfall_batch(batch_d, rows, want_stats=True, **av)
    torch.cuda.synchronize()
    for b, (w_rgb, w_lev, w_stats) in enumerate(want):
        assert torch.equal(rgb[b], w_rgb), b
        assert torch.equal(lev[b], w_lev), b
        assert torch.equal(stats[b].view(torch.int32), w_stats.view(torch.int32)), b
        assert _state(batch_d[b]) == _state(loop_d[b]), b
    return rgb, lev, stats, batch_d


AV = {0: dict(avg_mode=0), 1: dict(avg_mode=1, depth=4, minbin=10, maxbin=500), 2: dict(avg_mode=2, depth=4, minbin=0, maxbin=513),
      3: dict(avg_mode=3, depth=7, minbin=3, maxbin=511)}


# ---- 1. batch against loop

@pytest.mark.parametrize("scale", sorted(SCALES))
@pytest.mark.parametrize("max0", [0, 1])
@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_waterfall_batch_modes_scales(torch_cuda, lib, mode, max0, scale):
    rows = _rows(torch_cuda, 3, 300, 513, seed=mode * 10 + max0)          # 300 columns: two level chunks per stream
    _check(torch_cuda, lib, rows, _disps(lib, 3, **SCALES[scale]), max0=max0, **AV[mode])


@pytest.mark.parametrize("mode", [0, 2, 3])
@pytest.mark.parametrize("scale", ["log_auto", "lin_auto"])
def test_waterfall_batch_long_streams(torch_cuda, lib, scale, mode):
    """3 000 columns per stream: seeded warm-ups and the fix-up of every stream's own chunks."""
    rows = _rows(torch_cuda, 3, 3000, 257, seed=40 + mode)
    av = dict(AV[mode])
    if mode:
        av.update(minbin=5, maxbin=250)
    _check(torch_cuda, lib, rows, _disps(lib, 3, **SCALES[scale]), max0=1, **av)


@pytest.mark.parametrize("mode", [0, 2])
@pytest.mark.parametrize("nb", [1, 1000])
def test_waterfall_batch_many_short_streams(torch_cuda, lib, nb, mode):
    rows = _rows(torch_cuda, nb, 46, 129, seed=3)
    av = dict(avg_mode=mode, depth=4, minbin=2, maxbin=120) if mode else {}
    _check(torch_cuda, lib, rows, _disps(lib, nb, **SCALES["log_auto"]), **av)


def test_waterfall_batch_one_column(torch_cuda, lib):
    rows = _rows(torch_cuda, 4, 1, 65, seed=5)
    for av in (dict(avg_mode=0), dict(avg_mode=2, depth=3, minbin=0, maxbin=65)):
        _check(torch_cuda, lib, rows, _disps(lib, 4, **SCALES["lin_auto"]), **av)


# ---- 2. forced routes: staged average, tile starts inside each stream

@pytest.mark.parametrize("fused", ["1", "0"])
@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_waterfall_batch_tiles(torch_cuda, lib, monkeypatch, mode, fused):
    monkeypatch.setenv("GLFER_WATERFALL_FUSED", fused)
    monkeypatch.setenv("GLFER_WATERFALL_TILE", "100")                    # 300 columns: three tiles per stream
    rows = _rows(torch_cuda, 3, 300, 513, seed=60 + mode)
    _check(torch_cuda, lib, rows, _disps(lib, 3, **SCALES["log_auto"]), max0=1, **AV[mode])


@pytest.mark.parametrize("mode", [1, 2, 3])
def test_waterfall_batch_staged_route(torch_cuda, lib, monkeypatch, mode):
    monkeypatch.setenv("GLFER_WATERFALL_FUSED", "0")
    rows = _rows(torch_cuda, 5, 300, 513, seed=70 + mode)
    _check(torch_cuda, lib, rows, _disps(lib, 5, **SCALES["lin_auto"]), **AV[mode])


@pytest.mark.parametrize("mode", [1, 2, 3])
def test_waterfall_batch_deep_window_short_streams(torch_cuda, lib, mode):
    """46 columns: the avgmap chunk shrinks to 8, so a window of 20 rows (> 2 x chunk) takes the staged route."""
    rows = _rows(torch_cuda, 5, 46, 257, seed=80 + mode)
    _check(torch_cuda, lib, rows, _disps(lib, 5, **SCALES["log_auto"]), avg_mode=mode, depth=20, minbin=0, maxbin=257)


@pytest.mark.parametrize("bins", [8193, 16385])
def test_waterfall_batch_wide_bands(torch_cuda, lib, bins):
    """N = 16384 rows (fused) and N = 32768 rows: a band wider than 33 x 256 bins takes the staged route."""
    rows = _rows(torch_cuda, 2, 20, bins, seed=90)
    for mode in (2, 1):
        _check(torch_cuda, lib, rows, _disps(lib, 2, **SCALES["log_auto"]), avg_mode=mode, depth=4, minbin=0, maxbin=bins)


# ---- 3. rows at a pitch

def test_waterfall_batch_pitched_rows(torch_cuda, lib):
    """psd_pitch > bins: the batch reads stream b's rows where glfer_hip_waterfall_device reads them; with averaging the fused
    form is not taken (it walks dense rows) in either entry."""
    torch = torch_cuda
    L = lib.api.lib()
    nb, frames, bins, pitch = 3, 300, 513, 560
    rows = _rows(torch, nb, frames, bins, seed=11, pitch=pitch)
    rows[:, :, bins:] = -7.25                                              # the padding is never read
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for mode in (0, 2, 1):
        av = AV[mode] if mode == 0 else dict(avg_mode=mode, depth=4, minbin=10, maxbin=500)
        disps = _disps(lib, nb, psd_pitch=pitch, **SCALES["log_auto"])
        loop_d, batch_d = _copy(lib, disps), _copy(lib, disps)
        w_rgb = torch.empty((nb, frames, bins, 3), dtype=torch.uint8, device="cuda:0")
        w_lev = torch.empty((nb, frames, bins), dtype=torch.int16, device="cuda:0")
        for b in range(nb):
            assert L.glfer_hip_waterfall_device(C.byref(loop_d[b]), av["avg_mode"], av.get("depth", 1), av.get("minbin", 0),
                                                av.get("maxbin", 1), 0, rows[b].data_ptr(), frames, bins, w_rgb[b].data_ptr(),
                                                w_lev[b].data_ptr(), None, st) == 0
        arr = (lib.Display * nb)(*batch_d)
        rgb, lev = torch.empty_like(w_rgb), torch.empty_like(w_lev)
        assert L.glfer_hip_waterfall_batch_device(arr, nb, av["avg_mode"], av.get("depth", 1), av.get("minbin", 0), av.get("maxbin", 1),
                                                  0, rows.data_ptr(), frames, bins, rgb.data_ptr(), lev.data_ptr(), None, st) == 0
        torch.cuda.synchronize()
        assert torch.equal(rgb, w_rgb) and torch.equal(lev, w_lev), mode
        for b in range(nb):
            assert _state(arr[b]) == _state(loop_d[b]), (mode, b)


# ---- 4. continuity across calls

@pytest.mark.parametrize("scale", ["log_auto", "lin_auto"])
def test_waterfall_batch_continues_across_calls(torch_cuda, lib, scale):
    torch = torch_cuda
    rows = _rows(torch, 4, 700, 257, seed=13)
    one = _disps(lib, 4, **SCALES[scale])
    two = _copy(lib, one)
    rgb, lev, stats = lib.waterfall_batch(one, rows, want_stats=True)
    parts = [lib.waterfall_batch(two, rows[:, a:b].contiguous(), want_stats=True) for a, b in ((0, 1), (1, 300), (300, 700))]
    torch.cuda.synchronize()
    assert torch.equal(torch.cat([p[0] for p in parts], dim=1), rgb)
    assert torch.equal(torch.cat([p[1] for p in parts], dim=1), lev)
    assert torch.equal(torch.cat([p[2] for p in parts], dim=1), stats)
    for a, b in zip(one, two):
        assert _state(a) == _state(b)


# ---- 5. against the oracle, every stream with its own state

def test_waterfall_batch_oracle(torch_cuda, lib, oracle):
    torch = torch_cuda
    nb = 3
    rows = _rows(torch, nb, 300, 257, seed=17)
    kw = dict(scale_type=1, autoscale=1, overlap=0.5, palette=4, thr_level=10.0)
    disps = _disps(lib, nb, **kw)
    incoming = [_state(d) for d in disps]
    rgb, lev, stats = lib.waterfall_batch(disps, rows, want_stats=True)
    torch.cuda.synchronize()
    for b in range(nb):
        psd = rows[b].cpu().numpy()
        st_b = stats[b].cpu().numpy()
        w_st = np.array([oracle.floor_stats(r) for r in psd], np.float32)
        np.testing.assert_allclose(st_b[:, :2], w_st[:, :2], rtol=1e-6)
        fb, mx, mn = incoming[b]
        w_rgb, w_lev, _, w_state = oracle.display(psd, st_b, palette_id=4, scale_log=False, autoscale=True, overlap=0.5,
                                                  thr_level=10.0, first_buffer=bool(fb), state=(mx, mn))
        assert np.array_equal(rgb[b].cpu().numpy(), w_rgb), b                  # linear scale: no log10, every byte agrees
        bad = np.count_nonzero(lev[b].cpu().numpy() != w_lev)
        assert bad <= 1e-4 * w_lev.size, (b, bad)                              # tests/test_gpu_display.py's MISMATCH_MAX
        assert _state(disps[b]) == tuple(w_state), b


# ---- 6. argument errors

def test_waterfall_batch_argument_errors(torch_cuda, lib):
    torch = torch_cuda
    L = lib.api.lib()
    rows = _rows(torch, 3, 10, 129, seed=19)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rgb = torch.empty((3, 10, 129, 3), dtype=torch.uint8, device="cuda:0")
    sentinel = torch.full_like(rgb, 77)
    rgb.copy_(sentinel)
    for field, value in (("scale_type", 3), ("autoscale", 0), ("overlap", 0.25), ("max_level_db", -11.0), ("min_level_db", -61.0),
                         ("thr_level", 1.0), ("palette", 2), ("psd_pitch", 130)):
        disps = _disps(lib, 3, **SCALES["log_auto"])
        setattr(disps[2], field, value)
        arr = (lib.Display * 3)(*_copy(lib, disps))
        assert L.glfer_hip_waterfall_batch_device(arr, 3, 0, 1, 0, 1, 0, rows.data_ptr(), 10, 129, rgb.data_ptr(), None, None, st) == -1, field
        assert [_state(d) for d in arr] == [_state(d) for d in disps], field
    torch.cuda.synchronize()
    assert torch.equal(rgb, sentinel)                                          # nothing launched
    disps = _disps(lib, 3, **SCALES["log_auto"])
    arr = (lib.Display * 3)(*_copy(lib, disps))
    assert L.glfer_hip_waterfall_batch_device(arr, 0, 0, 1, 0, 1, 0, rows.data_ptr(), 10, 129, rgb.data_ptr(), None, None, st) == 0
    assert L.glfer_hip_waterfall_batch_device(arr, 3, 0, 1, 0, 1, 0, rows.data_ptr(), 0, 129, rgb.data_ptr(), None, None, st) == 0
    assert L.glfer_hip_waterfall_batch_device(None, 3, 0, 1, 0, 1, 0, rows.data_ptr(), 10, 129, rgb.data_ptr(), None, None, st) == -1
    # the single-stream entry's rules: a bad band, mode or depth, a pitch below bins
    assert L.glfer_hip_waterfall_batch_device(arr, 3, 2, 4, 0, 130, 0, rows.data_ptr(), 10, 129, rgb.data_ptr(), None, None, st) == -1
    assert L.glfer_hip_waterfall_batch_device(arr, 3, 4, 4, 0, 129, 0, rows.data_ptr(), 10, 129, rgb.data_ptr(), None, None, st) == -1
    assert L.glfer_hip_waterfall_batch_device(arr, 3, 2, 0, 0, 129, 0, rows.data_ptr(), 10, 129, rgb.data_ptr(), None, None, st) == -1
    torch.cuda.synchronize()
    assert torch.equal(rgb, sentinel)
    assert [_state(d) for d in arr] == [_state(d) for d in disps]
    empty = lib.waterfall_batch(disps, rows[:, :0].contiguous())
    assert empty[0].shape == (3, 0, 129, 3)
    assert [_state(d) for d in disps] == [_state(d) for d in _disps(lib, 3, **SCALES["log_auto"])]
