"""GPU tests (-m gpu): Spectrogram.run_zoom, the two-sided rows of the down-converter's output (glfer_hip_spectrogram_zoom_device).

Bit for bit (int32 views): run_zoom against run_iq(ddc.run(x)), frame ranges and centered included, for a periodogram plan and a
multitaper plan at N = 256.  Orientation: two real tones 3 / (D N) cycles apart around the zoom frequency land in columns N/2 and
N/2 + 3 of the centred rows.  Accuracy: every bin of those rows under the I/Q rule of tests/_rows_check.py against
_iq_exact.periodogram64 of the float64 down-converter output, tau_f32 from the float32 stand-ins of both stages in a row.
"""
import numpy as np
import pytest

import _ddc_exact as X
import _iq_exact as XC
from _rows_check import bound, check_rows, tau_of

pytestmark = pytest.mark.gpu
D, N = 16, 256


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _same(a, b):
    import torch
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("est", ["fft", "mtm"])
def test_zoom_equals_iq_rows_of_the_ddc_output(lib, torch_cuda, est):
    torch = torch_cuda
    if est == "fft":
        sp = lib.Spectrogram(lib.FftParams(n=N, window_type=lib.WINDOWS["hanning"], overlap=0.5))
    else:
        sp = lib.Spectrogram(lib.MtmParams(n=N, overlap=0.75, w=2.5, kmax=4))
    frames = 21
    rng = np.random.default_rng(5)
    x = torch.from_numpy((0.25 * rng.standard_normal(frames * sp.hop * D + D // 2 + 1)).astype(np.float32)).cuda()
    ddc = lib.Ddc(D, 0.1234567)
    base = ddc.run(x)
    assert base.shape == (frames * sp.hop,)
    want = sp.run_iq(base)
    assert want.shape == (frames, N)
    assert _same(sp.run_zoom(ddc, x), want)
    assert _same(sp.run_zoom(ddc, x, centered=True), sp.run_iq(base, centered=True))
    cuts = [0, 1, 3, 11, frames - 1, frames]
    for a, b in zip(cuts, cuts[1:]):
        assert _same(sp.run_zoom(ddc, x, first_frame=a, nframes=b - a), want[a:b]), (a, b)
        assert _same(sp.run_zoom(ddc, x, first_frame=a, nframes=b - a, centered=True), torch.roll(want[a:b], N // 2, dims=-1)), (a, b)
    pitched = torch.full((frames, N + 24), -7.25, dtype=torch.float32, device="cuda")
    sp.run_zoom(ddc, x, out=pitched[:, :N])
    assert _same(pitched[:, :N], want) and bool((pitched[:, N:] == -7.25).all())
    assert sp.run_zoom(ddc, x, first_frame=frames, nframes=0).shape == (0, N)
    with pytest.raises(lib.GlferHipError):
        sp.run_zoom(ddc, x, first_frame=frames, nframes=1)           # a frame past the baseband
    s16 = lib.Spectrogram(lib.FftParams(n=N, window_type=0, overlap=0.5, sample_format=lib.SAMPLES_S16))
    with pytest.raises(lib.GlferHipError):
        s16.run_zoom(ddc, x)                                         # the baseband is f32: the plan must be
    s16.close()
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    out = torch.empty((frames, N), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.graph(graph, stream=side):
        with pytest.raises(lib.GlferHipError):
            sp.run_zoom(ddc, x, out=out)                             # documented: a captured stream is refused
        base.add_(0)                                                 # (a capture must record something)
    torch.cuda.synchronize()
    ddc.close()
    sp.close()


def test_two_tones_land_in_their_own_columns(lib, torch_cuda):
    torch = torch_cuda
    frames, fc = 3, 0.1234567
    ns = frames * N * D
    t = np.arange(ns, dtype=np.float64)
    f1, f2 = fc, fc + 3.0 / (D * N)
    x = (0.4 * np.cos(2 * np.pi * f1 * t + 0.3) + 0.3 * np.cos(2 * np.pi * f2 * t + 1.1)).astype(np.float32)
    sp = lib.Spectrogram(lib.FftParams(n=N, window_type=lib.WINDOWS["rectangular"], overlap=0.0))
    ddc = lib.Ddc(D, fc)
    got = sp.run_zoom(ddc, torch.from_numpy(x).cuda(), centered=True).cpu().numpy()
    assert got.shape == (frames, N)
    top2 = np.sort(np.argsort(got, axis=1)[:, -2:], axis=1)
    assert (top2 == np.array([N // 2, N // 2 + 3])).all(), top2
    # every bin, against float64 all the way: the exact DDC output, its exact periodogram
    W = X.phase_word(fc)
    g = X.tables(W, ddc.taps)
    assert np.array_equal(g.view(np.int32), ddc.tables().view(np.int32))
    nout = ns // D
    y64, _ = X.exact(x.astype(np.complex64), g, W, D, 0, nout)
    y32 = X.standin32(x.astype(np.complex64), g, W, D, 0, nout)
    ones = np.ones(N, np.float32)
    exact = np.roll(XC.periodogram64(y64, N, 0.0, ones), N // 2, axis=1)
    f32 = np.roll(XC.periodogram32(y32, N, 0.0, ones), N // 2, axis=1)
    tau_f32 = tau_of(f32, exact)
    tau = bound(tau_f32)
    frac = check_rows(got, exact, tau, "zoom two tones")
    print("ddc-rows zoom D%d N%d two tones: fraction %.3f of the bound, tau_f32 %.3e" % (D, N, frac, tau_f32))
    ddc.close()
    sp.close()
