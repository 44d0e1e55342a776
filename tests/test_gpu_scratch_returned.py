"""GPU tests (-m gpu): every entry family gives its per-call scratch back.

A request of 16 MiB or more is served from a block the library keeps (glfer_amd/csrc/scratch.cpp, kBigMin).  A kept block that an
entry does not give back stays marked "out", and glfer_hip_scratch_trim(dev, 0) cannot free it.  So each case calls one entry once
at the smallest shape whose scratch is a kept block -- the size is worked out from the entry's code and asserted from the plan's
own hop and bins before the call --, asserts glfer_hip_scratch_held(dev) >= 16 MiB after it (the case is not vacuous: the call did
take a kept block), trims, and asserts that nothing is held.  What the entries compute is other tests' business."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
KEPT = 16 << 20                      # scratch.cpp kBigMin
N, FRAMES = 1024, 8200               # 8200 hops of 512 f32 samples: 16.0 MiB + 16 KiB


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


@pytest.fixture(autouse=True)
def nothing_kept(lib, torch_cuda):
    """Every case starts and ends with nothing kept, and the default cap."""
    L = lib.api.lib()
    dev = torch_cuda.cuda.current_device()
    torch_cuda.cuda.synchronize()
    L.glfer_hip_scratch_limit(16 << 30)
    L.glfer_hip_scratch_trim(dev, 0)
    assert L.glfer_hip_scratch_held(dev) == 0
    yield
    torch_cuda.cuda.synchronize()
    L.glfer_hip_scratch_limit(16 << 30)
    L.glfer_hip_scratch_trim(dev, 0)
    assert L.glfer_hip_scratch_held(dev) == 0


def _samples(torch, shape, seed):
    rng = np.random.default_rng(seed)
    return torch.from_numpy((0.25 * rng.standard_normal(shape)).astype(np.float32)).cuda()


def _returned(lib, torch, scratch_bytes, call):
    """`call` once; its scratch (scratch_bytes of it in one request, by the entry's code) was a kept block and has come back."""
    assert scratch_bytes >= KEPT, scratch_bytes
    L = lib.api.lib()
    dev = torch.cuda.current_device()
    call()
    held = L.glfer_hip_scratch_held(dev)
    assert held >= KEPT, held                            # the call took a kept block ...
    torch.cuda.synchronize()
    L.glfer_hip_scratch_trim(dev, 0)
    assert L.glfer_hip_scratch_held(dev) == 0            # ... and no block is still out


def _fft(lib, **kw):
    return lib.Spectrogram(lib.FftParams(n=N, window_type=lib.WINDOWS["hanning"], overlap=0.5, **kw))


def test_rows_through_the_corrected_copy(lib, torch_cuda, monkeypatch):
    """submean_scratch: the copy of every hop the frames read, hops x hop floats (GLFER_MEAN_PREPASS=1 keeps the pre-pass)."""
    monkeypatch.setenv("GLFER_MEAN_PREPASS", "1")
    sp = _fft(lib, sub_mean=lib.SUBMEAN_EXACT)
    x = _samples(torch_cuda, FRAMES * sp.hop, 1)
    _returned(lib, torch_cuda, FRAMES * sp.hop * 4, lambda: sp.run(x))
    sp.close()


def test_batch_rows_through_the_corrected_copies(lib, torch_cuda, monkeypatch):
    """submean_scratch over a batch: the streams' copies side by side in one block, 2 x hops x hop floats."""
    monkeypatch.setenv("GLFER_MEAN_PREPASS", "1")
    sp = _fft(lib, sub_mean=lib.SUBMEAN_EXACT)
    xs = _samples(torch_cuda, (2, FRAMES // 2 * sp.hop), 2)
    _returned(lib, torch_cuda, 2 * (FRAMES // 2) * sp.hop * 4, lambda: sp.run_batch(xs))
    sp.close()


def test_ragged_rows_through_the_corrected_copies(lib, torch_cuda, monkeypatch):
    """RaggedChunk::submean: hops [0, frames_b) of both streams in one block, (5000 + 3200) x hop floats."""
    monkeypatch.setenv("GLFER_MEAN_PREPASS", "1")
    sp = _fft(lib, sub_mean=lib.SUBMEAN_EXACT)
    frames = (5000, FRAMES - 5000)
    lengths = [f * sp.hop for f in frames]
    x = _samples(torch_cuda, sum(lengths), 3)
    _returned(lib, torch_cuda, sum(frames) * sp.hop * 4, lambda: sp.run_ragged(x, [0, lengths[0]], lengths))
    sp.close()


def test_lmp_rows(lib, torch_cuda):
    """glfer_run_device, LMP: the periodograms of the call's frames, frames x bins floats."""
    sp = lib.Spectrogram(lib.LmpParams(n=N, overlap=0.5, avg=4))
    x = _samples(torch_cuda, FRAMES * sp.hop, 4)
    _returned(lib, torch_cuda, FRAMES * sp.bins * 4, lambda: sp.run(x))
    sp.close()


def test_averaged_rows_without_psd(lib, torch_cuda):
    """glfer_hip_spectrogram_avg_device, two launches (a window of 5 frames: the average is not taken in the estimator launch):
    without want_psd the rows to average are scratch, frames x bins floats."""
    sp = _fft(lib)
    x = _samples(torch_cuda, FRAMES * sp.hop, 5)
    _returned(lib, torch_cuda, FRAMES * sp.bins * 4, lambda: sp.run_avg(x, lib.AVG_PLAIN, 5, 0, sp.bins, want_psd=False))
    sp.close()


def test_batch_averaged_rows_without_psd(lib, torch_cuda):
    """glfer_hip_spectrogram_avg_batch_device, two launches: the rows of both streams, 2 x frames x bins floats."""
    sp = _fft(lib)
    xs = _samples(torch_cuda, (2, FRAMES // 2 * sp.hop), 6)
    _returned(lib, torch_cuda, 2 * (FRAMES // 2) * sp.bins * 4,
              lambda: sp.run_avg_batch(xs, lib.AVG_PLAIN, 5, 0, sp.bins, want_psd=False))
    sp.close()


def test_ftest_spectra_in_scratch(lib, torch_cuda):
    """ftest_single below N = 256: the spectra of the 7 tapers and of hn for a group of frames, 8 x frames x N floats (4200
    frames are one group: a group holds 256 MiB of spectra, 65536 frames here, 32768 at the most)."""
    n, frames = 128, 4200
    sp = lib.Spectrogram(lib.MtmParams(n=n, overlap=0.0, w=4.0, kmax=7))
    x = _samples(torch_cuda, frames * sp.hop, 7)
    _returned(lib, torch_cuda, (sp.ntapers + 1) * frames * n * 4, lambda: sp.ftest(x))
    sp.close()


def test_staged_waterfall_with_averaging(lib, torch_cuda, monkeypatch):
    """waterfall_columns, staged (GLFER_WATERFALL_FUSED=0): a tile's averaged rows, (rows + depth) x bins doubles."""
    monkeypatch.setenv("GLFER_WATERFALL_FUSED", "0")
    torch = torch_cuda
    rows, bins, depth = 4200, 513, 4
    rng = np.random.default_rng(8)
    psd = torch.from_numpy(rng.random((rows, bins), dtype=np.float32) + np.float32(0.01)).cuda()
    disp = lib.Display()
    _returned(lib, torch, (rows + depth) * bins * 8, lambda: lib.waterfall(disp, psd, lib.AVG_PLAIN, depth, 0, bins))


def test_zoom_baseband(lib, torch_cuda):
    """glfer_hip_spectrogram_zoom_device: the down-converter's output for the call's frames, frames x N complex floats."""
    n, frames = 256, FRAMES
    sp = lib.Spectrogram(lib.FftParams(n=n, window_type=lib.WINDOWS["rectangular"], overlap=0.0))
    ddc = lib.Ddc(1, 0.1234567, taps=np.ones(1, np.float32))
    x = _samples(torch_cuda, frames * n + 1, 9)
    _returned(lib, torch_cuda, frames * n * 8, lambda: sp.run_zoom(ddc, x))
    ddc.close()
    sp.close()
