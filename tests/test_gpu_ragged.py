"""Streams of unequal length in one call (-m gpu): glfer_hip_spectrogram_ragged_device / Spectrogram.run_ragged against a
loop of the single-stream entry over the same memory, stream by stream with torch.equal.

The streams differ in seed, amplitude and DC level (as in test_gpu_batch.py), they lie shuffled in one buffer with gaps
between them that hold NaN (f32) or full-scale values (s16 / u8), and the output carries sentinel guard rows: a row taken
from the wrong stream, a read across a stream's start or end, a mean from the wrong table or a row written past a
stream's own frames cannot come out equal by accident.
"""
import ctypes as C

import numpy as np
import pytest

from _signals import synth

pytestmark = pytest.mark.gpu
HANNING = 0
SENTINEL = -7.25
GUARD = 3


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _layout(torch, lib, fmt, lengths, gap=5, seed=7):
    """One device buffer that holds streams of these lengths (samples) in a shuffled order, `gap` or gap + 1 fill samples
    in front of each (f32: odd and even offsets alike; s16 / u8: even offsets only).  Returns (tensor, offsets)."""
    order = np.random.RandomState(seed).permutation(len(lengths))
    offs, at = [0] * len(lengths), 0
    for b in order:
        at += gap + (b & 1)
        if fmt != lib.SAMPLES_F32:
            at += at & 1
        offs[b] = at
        at += lengths[b]
    at += gap
    if fmt == lib.SAMPLES_F32:
        buf = np.full(at, np.nan, np.float32)
    elif fmt == lib.SAMPLES_S16:
        buf = np.full(at, 32767, np.int16)
    else:
        buf = np.full(at, 255, np.uint8)
    for b, n in enumerate(lengths):
        amp = 0.4 + 0.6 * ((b * 7919) % 11) / 10.0
        dc = 0.05 * (((b * 104729) % 9) - 4)
        x = amp * synth(max(n, 1), seed=2000 + b)[:n] + dc
        if fmt == lib.SAMPLES_S16:
            x = np.clip(np.round(x * 20000.0), -32768, 32767)
        elif fmt == lib.SAMPLES_U8:
            x = np.clip(np.round(128.0 + x * 90.0), 0, 255)
        buf[offs[b]:offs[b] + n] = x.astype(buf.dtype)
    return torch.from_numpy(buf).to("cuda:0"), offs


def _lengths(n, hop, cap=None):
    """The issue's list, in samples: 0 frames (hop - 1 samples), 1, 2, 3, first_inside - 1, first_inside, first_inside + 1,
    7 (+ hop / 2 spare samples), 40, 41 frames -- shuffled by a fixed seed, the longest neither first nor last."""
    fi = -(-(n - hop) // hop)
    frames = [1, 2, 3, max(fi - 1, 0), fi, fi + 1, 40, 41]
    if cap is not None:
        frames = [min(f, cap) for f in frames]
    lens = [hop - 1] + [f * hop for f in frames] + [min(7, cap or 7) * hop + hop // 2]
    rs = np.random.RandomState(11)
    while True:
        lens = [lens[i] for i in rs.permutation(len(lens))]
        top = int(np.argmax(lens))
        if 0 < top < len(lens) - 1:
            return lens


def _check(torch, lib, sp, x, offs, lens):
    """run_ragged against run on the same views; guard rows, pitch padding and row_starts."""
    frames = [n // sp.hop for n in lens]
    total = sum(frames)
    got = torch.full((total + GUARD, sp.pitch), SENTINEL, dtype=torch.float32, device="cuda:0")
    _, starts = sp.run_ragged(x, offs, lens, out=got)
    torch.cuda.synchronize()
    assert starts.dtype == np.int64 and list(starts) == [0] + list(np.cumsum(frames))
    assert sp.ragged_frames(lens)[0] == total
    want = torch.full_like(got, SENTINEL)
    for b, (o, n) in enumerate(zip(offs, lens)):
        if frames[b]:
            sp.run(x[o:o + n], out=want[int(starts[b]):int(starts[b + 1])])
    torch.cuda.synchronize()
    assert torch.isfinite(got[:total, :sp.bins]).all()
    bad = [b for b in range(len(lens)) if not torch.equal(got[int(starts[b]):int(starts[b + 1])], want[int(starts[b]):int(starts[b + 1])])]
    assert not bad, (bad, [frames[b] for b in bad])
    assert bool((got[total:] == SENTINEL).all())                 # the guard rows
    if sp.pitch > sp.bins:
        assert bool((got[:, sp.bins:] == SENTINEL).all())
    return got, starts


C1 = lambda **k: dict(dict(kind="fft", n=1024, window_type=HANNING, overlap=0.5), **k)
C2 = lambda **k: dict(dict(kind="fft", n=4096, window_type=HANNING, overlap=0.75), **k)
C3 = lambda **k: dict(dict(kind="mtm", n=4096, overlap=0.0, w=2.5, kmax=4), **k)
C4 = lambda **k: dict(dict(kind="mtm", n=16384, overlap=0.0, w=4.5, kmax=8), **k)


def _params(lib, spec):
    spec = dict(spec)
    kind = spec.pop("kind")
    return {"fft": lib.FftParams, "mtm": lib.MtmParams, "hparma": lib.HparmaParams, "lmp": lib.LmpParams}[kind](**spec)


# params, frames cap per stream (None: the whole list)
CASES = {
    "C1": (C1(), None), "C1_sub1": (C1(sub_mean=1), None), "C1_sub2": (C1(sub_mean=2), None),
    "C2": (C2(), None), "C2_sub1": (C2(sub_mean=1), None), "C2_sub2": (C2(sub_mean=2), None),
    "C3": (C3(), None), "C3_sub1": (C3(sub_mean=1), None),
    "C3_zero_always": (C3(history_mode=1, overlap=0.5), None),
    "mtm_odd_512": (dict(kind="mtm", n=512, overlap=0.5, w=2.5, kmax=4), None),            # 5 tapers: spectro16x / xl
    "mtm_even_2048": (dict(kind="mtm", n=2048, overlap=0.5, w=2.5, kmax=3), None),         # 4 tapers: the packed kernel
    "mtm_8192": (dict(kind="mtm", n=8192, overlap=0.0, w=3.0, kmax=5), None),              # spectro16h's multitaper form
    "C4": (C4(), 6),
    "s16": (C2(sample_format=1), None), "u8": (C2(sample_format=2), None),
    "s16_mtm_odd": (dict(kind="mtm", n=1024, overlap=0.5, w=2.5, kmax=4, sample_format=1), None),
    "fft_ra9mb": (C1(a=0.3), None), "fft_limiter": (C1(limiter=1), None),
    "C2_pitch": (C2(psd_pitch=2112), None),
    # stream by stream inside the call
    "fft_128": (dict(kind="fft", n=128, window_type=HANNING, overlap=0.5), None),
    "fft_32768": (dict(kind="fft", n=32768, window_type=HANNING, overlap=0.5), 4),
    "lmp": (dict(kind="lmp", n=1024, overlap=0.5, avg=4), None),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_ragged_equals_loop(torch_cuda, lib, name):
    spec, cap = CASES[name]
    params = _params(lib, spec)
    sp = lib.Spectrogram(params)
    lens = _lengths(params.n, sp.hop, cap)
    x, offs = _layout(torch_cuda, lib, params.sample_format, lens)
    _check(torch_cuda, lib, sp, x, offs, lens)


def test_ragged_hparma_short_streams(torch_cuda, lib):
    params = lib.HparmaParams(n=4096, overlap=0.0, t=128, p_e=32)
    sp = lib.Spectrogram(params)
    lens = [2 * sp.hop, sp.hop - 1, 3 * sp.hop + 5]
    x, offs = _layout(torch_cuda, lib, params.sample_format, lens)
    _check(torch_cuda, lib, sp, x, offs, lens)


def test_ragged_one_stream_equals_run(torch_cuda, lib):
    for spec in (C1(sub_mean=1), C3()):
        sp = lib.Spectrogram(_params(lib, spec))
        lens = [9 * sp.hop + 3]
        x, offs = _layout(torch_cuda, lib, lib.SAMPLES_F32, lens)
        _check(torch_cuda, lib, sp, x, offs, lens)


def test_ragged_many_short_streams(torch_cuda, lib):
    """300 streams of 1 .. 3 frames at C1: many workgroups with nothing to do"""
    for sub in (0, 1):
        sp = lib.Spectrogram(_params(lib, C1(sub_mean=sub)))
        lens = [(1 + (b * 5) % 3) * sp.hop + (b % 7) for b in range(300)]
        x, offs = _layout(torch_cuda, lib, lib.SAMPLES_F32, lens, gap=2)
        _check(torch_cuda, lib, sp, x, offs, lens)


def test_ragged_one_long_stream_among_short(torch_cuda, lib):
    """one stream of 3000 frames among 36 of <= 4 at N = 256: the longest goes past one pass of the grid the streams share"""
    for sub in (0, 1):
        sp = lib.Spectrogram(_params(lib, dict(kind="fft", n=256, window_type=HANNING, overlap=0.5, sub_mean=sub)))
        lens = [(b % 5) * sp.hop + b for b in range(36)]
        lens.insert(17, 3000 * sp.hop + 11)
        x, offs = _layout(torch_cuda, lib, lib.SAMPLES_F32, lens)
        _check(torch_cuda, lib, sp, x, offs, lens)


def test_ragged_same_memory_and_overlaps(torch_cuda, lib):
    torch = torch_cuda
    for spec in (C1(sub_mean=1), C3()):
        sp = lib.Spectrogram(_params(lib, spec))
        x, _ = _layout(torch, lib, lib.SAMPLES_F32, [30 * sp.hop])
        base = 5                                                  # (_layout: the one stream starts after its gap)
        # streams 0 and 1 are the same memory; 2 .. 4 overlap them and one another
        offs = [base, base, base + sp.hop // 2 + 1, base + 3 * sp.hop, base + 7]
        lens = [12 * sp.hop, 12 * sp.hop, 20 * sp.hop + 9, 5 * sp.hop, 29 * sp.hop]
        got, starts = _check(torch, lib, sp, x, offs, lens)
        assert torch.equal(got[int(starts[0]):int(starts[1])], got[int(starts[1]):int(starts[2])])


def test_ragged_all_empty(torch_cuda, lib):
    torch = torch_cuda
    sp = lib.Spectrogram(_params(lib, C1()))
    lens = [sp.hop - 1, 0, 17]
    x, offs = _layout(torch, lib, lib.SAMPLES_F32, lens)
    got = torch.full((GUARD, sp.pitch), SENTINEL, dtype=torch.float32, device="cuda:0")
    _, starts = sp.run_ragged(x, offs, lens, out=got)
    torch.cuda.synchronize()
    assert list(starts) == [0, 0, 0, 0]
    assert bool((got == SENTINEL).all())


@pytest.mark.parametrize("name", ["C1", "C2_sub1", "C3", "s16"])
def test_ragged_equal_lengths_equal_run_batch(torch_cuda, lib, name):
    torch = torch_cuda
    params = _params(lib, CASES[name][0])
    sp = lib.Spectrogram(params)
    nb, n = 5, 13 * sp.hop + 2 * (sp.hop // 6)
    pitch = n + 6
    x, _ = _layout(torch, lib, params.sample_format, [nb * pitch], gap=0)
    streams = x[:nb * pitch].view(nb, pitch)[:, :n]
    want = sp.run_batch(streams)
    got, starts = sp.run_ragged(x, [b * pitch for b in range(nb)], [n] * nb)
    torch.cuda.synchronize()
    assert torch.equal(got.view(nb, -1, sp.pitch), want)


def test_ragged_above_the_grid_y_limit(torch_cuda, lib):
    """65 537 streams: two chunks, the second of one stream (which goes through the single-stream entry)"""
    torch = torch_cuda
    sp = lib.Spectrogram(_params(lib, dict(kind="fft", n=256, window_type=HANNING, overlap=0.5, sub_mean=1)))
    nb, n = 65537, 3 * sp.hop
    x = (torch.rand(nb * n, device="cuda:0", generator=torch.Generator(device="cuda:0").manual_seed(3)) - 0.3).contiguous()
    want = sp.run_batch(x.view(nb, n))
    got, starts = sp.run_ragged(x, np.arange(nb) * n, np.full(nb, n))
    torch.cuda.synchronize()
    assert int(starts[-1]) == nb * 3
    assert torch.equal(got.view(nb, 3, sp.pitch), want)


def test_ragged_long_stream_takes_the_short_ones_along(torch_cuda, lib):
    """One C2 stream of 4 000 frames among short ones: the launchers choose the kernel form and the grid from the LONGEST stream
    of a launch (spectro16h's register-reuse forms from work >= 4 x the resident workgroups), so the short streams run through a
    form their own single-stream calls do not pick -- and must come out equal all the same."""
    torch = torch_cuda
    for sub in (0, 1):
        sp = lib.Spectrogram(_params(lib, C2(sub_mean=sub)))
        lens = [3 * sp.hop, 41 * sp.hop + 7, 4000 * sp.hop + 5, sp.hop - 1, 7 * sp.hop + sp.hop // 2, 4 * sp.hop]
        gap, offs, at = 3, [], 0
        for n in lens:
            at += gap
            offs.append(at)
            at += n
        g = torch.Generator(device="cuda:0").manual_seed(5)
        x = torch.full((at + gap,), float("nan"), device="cuda:0")
        for b, (o, n) in enumerate(zip(offs, lens)):
            x[o:o + n] = torch.randn(n, device="cuda:0", generator=g) * (0.2 + 0.1 * b) + 0.03 * (b - 2)
        _check(torch, lib, sp, x, offs, lens)


@pytest.mark.parametrize("fmt", [1, 2])
@pytest.mark.parametrize("spec", [dict(history_mode=1, sub_mean=1), dict(sub_mean=1), dict(sub_mean=2), dict()],
                         ids=["zero_always_sub1", "sub1", "sub2", "plain"])
def test_ragged_integer_base_off_the_pair_alignment(torch_cuda, lib, fmt, spec):
    """s16 / u8 samples whose BUFFER starts one element off the pair alignment (a sliced tensor): the raw samples stay on the
    packed kernel, their corrected float copies do not -- the route is the one of the samples a launch reads, as in run."""
    torch = torch_cuda
    sp = lib.Spectrogram(_params(lib, C2(sample_format=fmt, **spec)))
    lens = _lengths(sp.n, sp.hop)
    x, offs = _layout(torch, lib, fmt, lens)
    y = torch.empty(x.numel() + 1, dtype=x.dtype, device="cuda:0")
    y[1:] = x
    assert y[1:].data_ptr() % (4 if fmt == 1 else 2) != 0
    _check(torch, lib, sp, y[1:], offs, lens)


def test_ragged_frames_and_argument_checks(torch_cuda, lib):
    """glfer_hip_ragged_frames' totals and prefix sums, and the entry's refusals that need a plan but no samples"""
    L = lib.api.lib()
    sp = lib.Spectrogram(_params(lib, C1()))
    h, hop = sp._h, sp.hop
    lens = np.array([0, hop - 1, hop, hop + 1, 7 * hop + hop // 2, 0, 40 * hop], np.uint64)
    starts = np.full(lens.size + 1, 2 ** 63, np.uint64)
    total = L.glfer_hip_ragged_frames(h, lens.size, lens.ctypes.data, starts.ctypes.data)
    frames = lens // np.uint64(hop)
    assert list(frames[:4]) == [0, 0, 1, 1]
    assert total == int(frames.sum())
    assert list(starts) == [0] + list(np.cumsum(frames))
    assert L.glfer_hip_ragged_frames(h, lens.size, lens.ctypes.data, None) == total      # row_starts is optional
    assert L.glfer_hip_ragged_frames(h, 0, None, None) == 0
    assert L.glfer_hip_ragged_frames(h, 2, None, None) == 0
    offs = np.zeros(lens.size, np.uint64)
    assert L.glfer_hip_spectrogram_ragged_device(h, None, lens.size, None, lens.ctypes.data, None, None, None) == -1
    assert L.glfer_hip_spectrogram_ragged_device(h, None, lens.size, offs.ctypes.data, None, None, None, None) == -1
    assert L.glfer_hip_spectrogram_ragged_device(h, None, lens.size, offs.ctypes.data, lens.ctypes.data, None, None, None) == -1
    none = np.array([hop - 1, 0, 3], np.uint64)
    st = np.full(4, 9, np.uint64)
    assert L.glfer_hip_spectrogram_ragged_device(h, None, 3, offs.ctypes.data, none.ctypes.data, None, st.ctypes.data, None) == 0
    assert list(st) == [0, 0, 0, 0]
    assert L.glfer_hip_spectrogram_ragged_device(h, None, 0, None, None, None, None, None) == 0


def test_ragged_refuses_a_capturing_stream(torch_cuda, lib):
    """the tables are uploaded from host memory that is gone after the call: a captured copy would read it at every replay"""
    torch = torch_cuda
    sp = lib.Spectrogram(_params(lib, C1()))
    x = torch.zeros(16 * sp.hop, device="cuda:0")
    out = torch.full((8 + GUARD, sp.pitch), SENTINEL, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    graph, refused = torch.cuda.CUDAGraph(), False
    with torch.cuda.graph(graph):
        try:
            sp.run_ragged(x, [0, 8 * sp.hop], [4 * sp.hop, 4 * sp.hop], out=out)
        except lib.GlferHipError:
            refused = True
    torch.cuda.synchronize()
    assert refused
    assert bool((out == SENTINEL).all())
    sp.run_ragged(x, [0, 8 * sp.hop], [4 * sp.hop, 4 * sp.hop], out=out)     # outside a capture: as ever
    torch.cuda.synchronize()
    assert bool((out[:8, :sp.bins] == out[0, :sp.bins]).all()) and bool((out[8:] == SENTINEL).all())


def test_ragged_run_list(torch_cuda, lib):
    torch = torch_cuda
    for fmt in (lib.SAMPLES_F32, lib.SAMPLES_S16):
        sp = lib.Spectrogram(_params(lib, C2(sample_format=fmt, sub_mean=1)))
        lens = [5 * sp.hop + 1, sp.hop - 1, 9 * sp.hop + 3, 2 * sp.hop + 1]      # odd lengths: run_list keeps the offsets even
        x, offs = _layout(torch, lib, fmt, lens)
        parts = [x[o:o + n].clone() for o, n in zip(offs, lens)]
        rows = sp.run_list(parts)
        torch.cuda.synchronize()
        assert [r.size(0) for r in rows] == [n // sp.hop for n in lens]
        for part, r in zip(parts, rows):
            if r.size(0):
                assert torch.equal(r, sp.run(part))


def test_ragged_refusals(torch_cuda, lib):
    torch = torch_cuda
    L = lib.api.lib()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    # an odd offset with s16
    sp = lib.Spectrogram(_params(lib, C2(sample_format=1)))
    x = torch.zeros(16 * sp.hop, dtype=torch.int16, device="cuda:0")
    with pytest.raises(lib.GlferHipError):
        sp.run_ragged(x, [0, 4 * sp.hop + 1], [4 * sp.hop, 4 * sp.hop])
    # a NULL d_psd when there are frames; a frame count over the limit, through `lengths` alone (no such memory exists:
    # the entry refuses before it touches the samples)
    sp = lib.Spectrogram(_params(lib, C1()))
    x = torch.zeros(8 * sp.hop, dtype=torch.float32, device="cuda:0")
    out = torch.full((8 + GUARD, sp.pitch), SENTINEL, dtype=torch.float32, device="cuda:0")
    offs = np.array([0, 0], np.uint64)
    lens = np.array([4 * sp.hop, 4 * sp.hop], np.uint64)
    assert L.glfer_hip_spectrogram_ragged_device(sp._h, C.c_void_p(x.data_ptr()), 2, offs.ctypes.data, lens.ctypes.data,
                                                 None, None, st) == -1
    big = np.array([4 * sp.hop, sp.hop * 2 ** 31], np.uint64)
    assert L.glfer_hip_spectrogram_ragged_device(sp._h, C.c_void_p(x.data_ptr()), 2, offs.ctypes.data, big.ctypes.data,
                                                 C.c_void_p(out.data_ptr()), None, st) == -1
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
