"""Many streams per call (-m gpu): glfer_hip_spectrogram_batch_device / Spectrogram.run_batch against a loop of the
single-stream entry over the same streams, row for row with torch.equal.

The streams of a batch differ in seed, amplitude and DC level, so that a row taken from the wrong stream, history read
across a stream boundary or a mean removed with the wrong stream's table cannot come out equal by accident.
"""
import ctypes as C

import numpy as np
import pytest

from _signals import rel_err, synth

pytestmark = pytest.mark.gpu
HANNING = 0


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _streams(torch, lib, fmt, nb, nsamples, pitch=None, gap=None):
    """[nb, nsamples] view of a [nb, pitch] buffer of the plan's sample type; the pitch - nsamples samples after each
    stream hold `gap`."""
    pitch = pitch or nsamples
    if fmt != lib.SAMPLES_F32:
        pitch += pitch & 1                             # integer samples: an even stream pitch (glfer_hip.h)
    out = np.zeros((nb, pitch), np.float64)
    for b in range(nb):
        amp = 0.4 + 0.6 * ((b * 7919) % 11) / 10.0
        dc = 0.05 * (((b * 104729) % 9) - 4)
        out[b, :nsamples] = amp * synth(nsamples, seed=1000 + b) + dc
    if fmt == lib.SAMPLES_F32:
        buf = out.astype(np.float32)
    elif fmt == lib.SAMPLES_S16:
        buf = np.clip(np.round(out * 20000.0), -32768, 32767).astype(np.int16)
    else:
        buf = np.clip(np.round(128.0 + out * 90.0), 0, 255).astype(np.uint8)
    if gap is not None and pitch > nsamples:
        buf[:, nsamples:] = gap
    t = torch.from_numpy(buf).to("cuda:0")
    return t[:, :nsamples]


def _loop(torch, sp, streams, first, nframes, out):
    for b in range(streams.size(0)):
        sp.run(streams[b], first_frame=first, nframes=nframes, out=out[b])
    torch.cuda.synchronize()
    return out


def _check_batch(torch, lib, params, nb, nsamples, first=0, nframes=None, pitch=None, gap=None, sentinel=None):
    sp = lib.Spectrogram(params)
    fmt = params.sample_format
    x = _streams(torch, lib, fmt, nb, nsamples, pitch=pitch, gap=gap)
    total = sp.num_frames(nsamples)
    nframes = total - first if nframes is None else nframes
    fill = 0.0 if sentinel is None else sentinel
    got = torch.full((nb, nframes, sp.pitch), fill, dtype=torch.float32, device="cuda:0")
    want = torch.full_like(got, fill)
    sp.run_batch(x, first_frame=first, nframes=nframes, out=got)
    torch.cuda.synchronize()
    _loop(torch, sp, x, first, nframes, want)
    assert torch.isfinite(got[:, :, :sp.bins]).all()
    assert torch.equal(got, want), [b for b in range(nb) if not torch.equal(got[b], want[b])][:8]
    if sentinel is not None:
        assert bool((got[:, :, sp.bins:] == sentinel).all())
    return got


C1 = lambda **k: dict(dict(kind="fft", n=1024, window_type=HANNING, overlap=0.5), **k)
C2 = lambda **k: dict(dict(kind="fft", n=4096, window_type=HANNING, overlap=0.75), **k)
C3 = lambda **k: dict(dict(kind="mtm", n=4096, overlap=0.0, w=2.5, kmax=4), **k)
C4 = lambda **k: dict(dict(kind="mtm", n=16384, overlap=0.0, w=4.5, kmax=8), **k)


def _params(lib, spec):
    spec = dict(spec)
    kind = spec.pop("kind")
    return {"fft": lib.FftParams, "mtm": lib.MtmParams, "hparma": lib.HparmaParams, "lmp": lib.LmpParams}[kind](**spec)


# (params, streams, frames per stream)
CASES = {
    "C1": (C1(), 37, 40), "C1_sub1": (C1(sub_mean=1), 3, 40), "C1_sub2": (C1(sub_mean=2), 3, 40),
    "C2": (C2(), 37, 24), "C2_sub1": (C2(sub_mean=1), 3, 24), "C2_sub2": (C2(sub_mean=2), 3, 24),
    "C3": (C3(), 37, 12), "C3_sub1": (C3(sub_mean=1), 3, 12), "C3_sub2": (C3(sub_mean=2), 3, 12),
    "C4": (C4(), 3, 5), "C4_sub1": (C4(sub_mean=1), 3, 5),
    "C5": (dict(kind="hparma", n=4096, overlap=0.0, t=128, p_e=32), 3, 3),
    "mtm_even_2048": (dict(kind="mtm", n=2048, overlap=0.5, w=2.5, kmax=3), 37, 20),      # 4 tapers: the packed kernel
    "mtm_odd_512": (dict(kind="mtm", n=512, overlap=0.5, w=2.5, kmax=4), 37, 40),         # 5 tapers: spectro16x / xl
    "mtm_odd_1024": (dict(kind="mtm", n=1024, overlap=0.75, w=2.5, kmax=4), 37, 40),
    "mtm_8192": (dict(kind="mtm", n=8192, overlap=0.0, w=3.0, kmax=5), 3, 6),             # spectro16h's multitaper form
    "fft_128": (dict(kind="fft", n=128, window_type=HANNING, overlap=0.5), 3, 50),       # below 256: stream by stream
    "fft_32768": (dict(kind="fft", n=32768, window_type=HANNING, overlap=0.5), 3, 4),    # above 16384: stream by stream
    "lmp": (dict(kind="lmp", n=1024, overlap=0.5, avg=4), 3, 20),
    "zero_always": (C2(history_mode=1), 37, 24),
    "zero_always_mtm": (C3(history_mode=1, overlap=0.5), 3, 12),
    "s16": (C2(sample_format=1), 3, 24), "u8": (C2(sample_format=2), 3, 24),
    "s16_mtm_odd": (dict(kind="mtm", n=1024, overlap=0.5, w=2.5, kmax=4, sample_format=1), 3, 40),
    "u8_c1": (C1(sample_format=2), 37, 40),
    # the packed kernel's general path (RA9MB, limiter), and mean removal in the other kernel forms
    "fft_limiter": (C1(limiter=1), 9, 40), "fft_ra9mb": (C1(a=0.3), 9, 40), "fft_ra9mb_sub1": (C1(a=0.3, sub_mean=1), 9, 40),
    "mtm_odd_512_sub1": (dict(kind="mtm", n=512, overlap=0.5, w=2.5, kmax=4, sub_mean=1), 37, 40),
    "mtm_odd_1024_sub2": (dict(kind="mtm", n=1024, overlap=0.75, w=2.5, kmax=4, sub_mean=2), 9, 40),
    "mtm_even_2048_sub1": (dict(kind="mtm", n=2048, overlap=0.5, w=2.5, kmax=3, sub_mean=1), 9, 20),
    "mtm_8192_sub1": (dict(kind="mtm", n=8192, overlap=0.0, w=3.0, kmax=5, sub_mean=1), 3, 6),
    "C4_sub2": (C4(sub_mean=2), 3, 5),
    "s16_sub1": (C2(sample_format=1, sub_mean=1), 9, 24), "u8_mtm_sub1": (C3(sample_format=2, sub_mean=1), 9, 12),
    "zero_always_sub1": (C2(history_mode=1, sub_mean=1), 9, 24),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_batch_equals_loop(torch_cuda, lib, name):
    spec, nb, nframes = CASES[name]
    params = _params(lib, spec)
    hop = int(params.n * (1.0 - params.overlap))
    _check_batch(torch_cuda, lib, params, nb, nframes * hop + hop // 3)


@pytest.mark.parametrize("nb", [1, 3, 37])
@pytest.mark.parametrize("shape", ["C1", "C3", "mtm_odd_512"])
def test_batch_sizes(torch_cuda, lib, shape, nb):
    spec, _, nframes = CASES[shape]
    params = _params(lib, spec)
    hop = int(params.n * (1.0 - params.overlap))
    _check_batch(torch_cuda, lib, params, nb, nframes * hop)


def test_psd_pitch_padding_survives(torch_cuda, lib):
    _check_batch(torch_cuda, lib, _params(lib, C2(psd_pitch=2112)), 5, 24 * 1024, sentinel=-7.25)
    _check_batch(torch_cuda, lib, _params(lib, C3(psd_pitch=2112)), 5, 12 * 4096, sentinel=-7.25)


@pytest.mark.parametrize("shape", ["C1", "C2", "C3", "mtm_odd_1024", "C2_sub1", "C3_sub1", "mtm_odd_1024_sub2"])
def test_first_frame_inside(torch_cuda, lib, shape):
    spec, nb, nframes = CASES[shape]
    params = _params(lib, spec)
    hop = int(params.n * (1.0 - params.overlap))
    _check_batch(torch_cuda, lib, params, min(nb, 7), nframes * hop, first=5, nframes=nframes - 9)


@pytest.mark.parametrize("fmt", [0, 1, 2])
@pytest.mark.parametrize("shape", ["C1", "C2", "C3", "mtm_odd_512", "C2_sub1", "C3_sub1", "C1_sub2"])
def test_gap_between_streams(torch_cuda, lib, shape, fmt):
    """The samples between streams are NaN (f32) or full scale (integers): history read from the previous stream or a
    read past a stream's end shows as a non-finite or unequal row."""
    spec, nb, nframes = CASES[shape]
    spec = dict(spec, sample_format=fmt)
    params = _params(lib, spec)
    hop = int(params.n * (1.0 - params.overlap))
    nsamples = nframes * hop
    gap = {0: np.float32(np.nan), 1: np.int16(32767), 2: np.uint8(255)}[fmt]
    _check_batch(torch_cuda, lib, params, min(nb, 9), nsamples, pitch=nsamples + 2 * params.n + 6, gap=gap)


def test_large_batch_crosses_grid_y_limit(torch_cuda, lib):
    """70 000 one-frame streams: more than one chunk of the grid's y limit."""
    torch = torch_cuda
    params = _params(lib, C1())
    sp = lib.Spectrogram(params)
    nb, hop = 70000, sp.hop
    x = (torch.rand((nb, hop), generator=torch.Generator().manual_seed(5), dtype=torch.float32) - 0.5)
    x = (x + torch.linspace(-0.3, 0.3, nb)[:, None]).to("cuda:0")
    got = sp.run_batch(x)
    torch.cuda.synchronize()
    assert got.shape == (nb, 1, sp.bins) and bool(torch.isfinite(got).all())
    probe = sorted(set([0, 1, 2, 65533, 65534, 65535, 65536, 65537, nb - 2, nb - 1] +
                       list(np.random.default_rng(3).integers(0, nb, 64))))
    for b in probe:
        want = sp.run(x[b])
        torch.cuda.synchronize()
        assert torch.equal(got[b], want), b


def test_stream_past_4gib(torch_cuda, lib):
    """The last stream of the batch starts beyond 4 GiB of the buffer: its first, middle and last frames."""
    torch = torch_cuda
    for spec in (C3(), C2()):
        params = _params(lib, spec)
        sp = lib.Spectrogram(params)
        nsamples = 64 * sp.hop
        pitch = (1 << 30) + 4096                       # floats: stream 1 at 4 GiB + 16 KiB
        buf = torch.empty(pitch + nsamples, dtype=torch.float32, device="cuda:0")
        buf[:nsamples] = torch.from_numpy(synth(nsamples, seed=21)).to("cuda:0")
        buf[pitch:] = torch.from_numpy(0.7 * synth(nsamples, seed=22) + 0.1).to("cuda:0")
        x = buf.as_strided((2, nsamples), (pitch, 1))
        got = sp.run_batch(x)
        want1 = sp.run(buf[pitch:])
        want0 = sp.run(buf[:nsamples])
        torch.cuda.synchronize()
        nf = sp.num_frames(nsamples)
        for f in (0, nf // 2, nf - 1):
            assert torch.equal(got[1, f], want1[f]), f
            assert torch.equal(got[0, f], want0[f]), f
        del buf, x, got
        torch.cuda.empty_cache()


def test_batch_oracle_parity(torch_cuda, lib, oracle):
    torch = torch_cuda
    params = _params(lib, C3())
    sp = lib.Spectrogram(params)
    nsamples = 12 * 4096
    x = _streams(torch, lib, 0, 4, nsamples)
    got = sp.run_batch(x).cpu().numpy()
    xs = x.cpu().numpy()
    for b in range(4):
        want = oracle.spectrogram_mtm(xs[b], 4096, 0.0, 2.5, 4)
        worst = max(max(rel_err(got[b, f], want[f])) for f in range(want.shape[0]))
        assert worst < 1e-5, (b, worst)


def test_empty_and_bad_arguments(torch_cuda, lib):
    torch = torch_cuda
    L = lib.api.lib()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    sp = lib.Spectrogram(_params(lib, C2(sample_format=1)))
    x = torch.zeros((4, 8 * 4096), dtype=torch.int16, device="cuda:0")
    out = torch.full((4, 8, sp.bins), 3.0, device="cuda:0")
    call = lambda nb, pitch, nframes, first=0: L.glfer_hip_spectrogram_batch_device(
        sp._h, C.c_void_p(x.data_ptr()), nb, pitch, 4 * 4096, first, nframes, C.c_void_p(out.data_ptr()), st)
    assert call(3, 8 * 4096 - 1, 4) == -1                      # odd pitch with s16 samples: GLFER_E_ARG
    assert call(0, 8 * 4096, 4) == 0 and call(3, 8 * 4096, 0) == 0
    assert call(3, 8 * 4096, 17) == -1                         # frame past the stream
    torch.cuda.synchronize()
    assert bool((out == 3.0).all())                            # nothing was launched
    assert call(3, 8 * 4096, 8) == 0                           # 3 x 8 rows: inside `out`
    torch.cuda.synchronize()
    assert not bool((out[:3] == 3.0).all())
