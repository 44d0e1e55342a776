"""Float64 'exact-arithmetic' auto-spectra, cross-spectrum and coherence of two interleaved real channels, their float32 stand-in,
and the inputs the cross tests share (tests only): tests/_iq_exact.py for Spectrogram.cross.

A stream is pairs (x[n], y[n]) whose values are float32 (the sample format's conversion is input preparation and exact).  Frame f
holds pairs [f H - (N - H), f H + H) with the history rules of real streams.  With the plan's tapers v_j and c_j = 1 / (N (1 + sig_j)):

    X_j = rfft(v_j x_f)   Y_j = rfft(v_j y_f)
    Sxx = sum_j c_j |X_j|^2   Syy = sum_j c_j |Y_j|^2   Sxy = sum_j c_j X_j conj(Y_j)   coh = |Sxy|^2 / (Sxx Syy), 0 where Sxx Syy = 0

in float64 (numpy.fft.rfft per channel and taper).  The stand-in keeps the same frames and goes float32: one float32 transform per
channel and taper, torch.fft.rfft on CPU tensors row by row (as _iq_exact._fft32: the batched transform is another algorithm at large
N), products, weights and the taper sums in float32; its quotient is formed in double from the float32 sums, as the kernel forms it.
"""
import collections

import numpy as np

from _iq_exact import frames64

Cross = collections.namedtuple("Cross", ("sxx", "syy", "sxy", "coh"))


def to_float32(xy, fmt_name):
    """The float32 values of a stream of the plan's sample format (wav_fmt.c:104-117), exact."""
    xy = np.asarray(xy)
    if fmt_name == "f32":
        return xy.astype(np.float32)
    if fmt_name == "s16":
        return (xy.astype(np.float32) / np.float32(32768.0)).astype(np.float32)
    return ((xy.astype(np.float32) - np.float32(128.0)) / np.float32(128.0)).astype(np.float32)


def quantise(xy32, fmt_name):
    """A float32 stream in [-1, 1) as the sample format's integers (f32: itself)."""
    if fmt_name == "f32":
        return np.ascontiguousarray(xy32, np.float32)
    if fmt_name == "s16":
        return np.clip(np.round(xy32 * 32768.0), -32768, 32767).astype(np.int16)
    return np.clip(np.round(xy32 * 128.0 + 128.0), 0, 255).astype(np.uint8)


def _coh(sxx, syy, sxy):
    den = sxx.astype(np.float64) * syy.astype(np.float64)
    num = sxy.real.astype(np.float64) ** 2 + sxy.imag.astype(np.float64) ** 2
    return np.where(den > 0, np.minimum(num / np.where(den > 0, den, 1.0), 1.0), 0.0)


def cross64(xy32, n, overlap, tapers, sig, history_mode=0, ntap=None, weights=None):
    """xy32: float32 [S, 2].  ntap: only the first ntap tapers; weights: c_j N instead of 1 / (1 + sig_j) (the criterion test's
    mutations).  Returns Cross of float64 / complex128 [frames][n/2+1]."""
    xy32 = np.asarray(xy32, np.float32)
    fr = frames64(xy32[:, 0] + 1j * xy32[:, 1].astype(np.complex64), n, overlap, history_mode)
    fx, fy = fr.real, fr.imag
    nt = len(sig) if ntap is None else ntap
    sxx = np.zeros((fr.shape[0], n // 2 + 1))
    syy = np.zeros_like(sxx)
    sxy = np.zeros(sxx.shape, np.complex128)
    for j in range(nt):
        c = (1.0 / (1.0 + sig[j]) if weights is None else weights[j]) / n
        X = np.fft.rfft(fx * tapers[j], axis=1)
        Y = np.fft.rfft(fy * tapers[j], axis=1)
        sxx += c * (X.real ** 2 + X.imag ** 2)
        syy += c * (Y.real ** 2 + Y.imag ** 2)
        sxy += c * X * np.conj(Y)
    return Cross(sxx, syy, sxy, _coh(sxx, syy, sxy))


def _rfft32(rows):
    import torch
    rows = np.ascontiguousarray(rows, np.float32)
    out = np.empty((rows.shape[0], rows.shape[1] // 2 + 1), np.complex64)
    for f in range(rows.shape[0]):
        out[f] = torch.fft.rfft(torch.from_numpy(rows[f])).numpy()
    return out


def cross32(xy32, n, overlap, tapers, sig, history_mode=0):
    """The float32 stand-in: Cross of float32 / complex64 rows (coh float64 from the float32 sums)."""
    xy32 = np.asarray(xy32, np.float32)
    fr = frames64(xy32[:, 0] + 1j * xy32[:, 1].astype(np.complex64), n, overlap, history_mode)
    fx, fy = fr.real.astype(np.float32), fr.imag.astype(np.float32)            # (exact: the values are float32)
    sxx = np.zeros((fr.shape[0], n // 2 + 1), np.float32)
    syy = np.zeros_like(sxx)
    sre = np.zeros_like(sxx)
    sim = np.zeros_like(sxx)
    for j in range(len(sig)):
        c = np.float32(1.0 / (n * (1.0 + sig[j])))
        v = np.asarray(tapers[j], np.float32)
        X, Y = _rfft32(fx * v), _rfft32(fy * v)
        sxx += c * (X.real * X.real + X.imag * X.imag)
        syy += c * (Y.real * Y.real + Y.imag * Y.imag)
        sre += c * (X.real * Y.real + X.imag * Y.imag)
        sim += c * (X.imag * Y.real - X.real * Y.imag)
    sxy = (sre + 1j * sim).astype(np.complex64)
    return Cross(sxx, syy, sxy, _coh(sxx, syy, sxy))


# ---- the inputs: float32 [S, 2] in [-1, 1)
INPUTS = ("noise", "same", "delay3", "line", "edge_tones", "impulses", "silence", "x_only", "apart40")
LINE_DB = -40.0


def line_bin(n):
    return n // 4 + 3


def make_input(name, n, nsamples, seed):
    rng = np.random.default_rng([seed, n, INPUTS.index(name)])
    t = np.arange(nsamples, dtype=np.float64)
    nx, ny = 0.2 * rng.standard_normal(nsamples), 0.2 * rng.standard_normal(nsamples)
    if name == "noise":
        x, y = nx, ny
    elif name == "same":
        x, y = nx, nx
    elif name == "delay3":                        # y lags x by three samples
        x, y = nx, np.concatenate([np.zeros(3), nx[:-3]])
    elif name == "line":                          # a common line 40 dB under the independent noise of each channel (total power)
        amp = 0.2 * np.sqrt(2.0) * 10.0 ** (LINE_DB / 20.0)
        x = nx + amp * np.sin(2 * np.pi * line_bin(n) * t / n + 0.3)
        y = ny + amp * np.sin(2 * np.pi * line_bin(n) * t / n + 1.1)
    elif name == "edge_tones":                    # a tone on bin 1 in x, one on bin N/2 - 1 in y, a little of each in the other
        a, b = np.sin(2 * np.pi * 1 * t / n + 0.2), np.sin(2 * np.pi * (n // 2 - 1) * t / n + 0.5)
        x, y = 0.6 * a + 0.05 * b, 0.1 * a + 0.5 * b
    elif name == "impulses":
        x, y = np.zeros(nsamples), np.zeros(nsamples)
        x[rng.integers(0, nsamples, 7)] = 0.9
        y[rng.integers(0, nsamples, 7)] = -0.8
        y[3] = 0.5
    elif name == "silence":
        x, y = np.zeros(nsamples), np.zeros(nsamples)
    elif name == "x_only":                        # one channel silent
        x, y = nx, np.zeros(nsamples)
    elif name == "apart40":                       # channels 40 dB apart
        x, y = 2.0 * nx, 0.02 * ny
    else:
        raise ValueError(name)
    return np.clip(np.stack([x, y], axis=1), -0.999, 0.999).astype(np.float32)


# ---- inputs keyed to the passes of a persistent grid (tests/_grid_passes.py): equal-level noise cannot show state that a block
# carries from one of its frame groups into the next, these can.  `stride` is the frames (Welch: rows) one pass of the grid
# covers; a sample belongs to the frame whose fresh hop it lies in, a frame to row frame // step, a row to pass row // stride.
#   x_late         independent noise; x exactly zero from the first sample of frame c on, c = stride * step (+ 1 when segments
#                  > 1: the first row of pass 1 then has x in its segment 0 alone).  Every frame of the later passes past c
#                  is silent in x; the frames before c that overlap into it keep the samples they have
#   x_early        x exactly zero up to the last sample of frame c = stride * step + segments - 2 (segments = 1: the last
#                  frame of pass 0): pass 0 is silent in x, and the first row of pass 1 has x in its LAST segment alone
#   apart_by_pass  the channels' levels are 1 and 1e-3 in the even passes and exchanged in the odd ones (two passes: 1 and 1e-3
#                  in pass 0, exchanged in the later one)
PASS_INPUTS = ("x_late", "x_early", "apart_by_pass")


def make_pass_input(name, n, hop, nframes, seed, stride, segments=1, step=1):
    nsamples = nframes * hop
    rng = np.random.default_rng([seed, n, 100 + PASS_INPUTS.index(name)])
    x, y = 0.2 * rng.standard_normal(nsamples), 0.2 * rng.standard_normal(nsamples)
    if name == "x_late":
        c = stride * step + (1 if segments > 1 else 0)
        x[max(c * hop - (n - hop), 0):] = 0.0
    elif name == "x_early":
        c = stride * step + segments - 2
        x[:(c + 1) * hop] = 0.0
    elif name == "apart_by_pass":
        odd = ((np.arange(nsamples) // hop) // step // stride) % 2 == 1
        x *= np.where(odd, 1e-3, 1.0)
        y *= np.where(odd, 1.0, 1e-3)
    else:
        raise ValueError(name)
    return np.clip(np.stack([x, y], axis=1), -0.999, 0.999).astype(np.float32)


def silence_bits(xy32, n, overlap, history_mode=0):
    """Per frame: bit 0 / bit 1 set where the frame's x / y samples are not all zero (what the kernel's epilogue decides by)."""
    xy32 = np.asarray(xy32, np.float32)
    fr = frames64(xy32[:, 0] + 1j * xy32[:, 1].astype(np.complex64), n, overlap, history_mode)
    return (fr.real != 0).any(axis=1) * 1 + (fr.imag != 0).any(axis=1) * 2


def _packed32(fx, fy, tapers, sig, n):
    """The float32 sums of frames through ONE packed transform per taper, Z = FFT(v (x + i y)), separated through the mirror
    bins as the kernel separates them: a silent channel's spectrum is then rounding, not zero.  Returns (sxx, syy, sre, sim)."""
    from _iq_exact import _fft32
    half = n // 2 + 1
    k = np.arange(half)
    out = [np.zeros((fx.shape[0], half), np.float32) for _ in range(4)]
    for j in range(len(sig)):
        c = np.float32(0.25 / (n * (1.0 + sig[j])))
        v = np.asarray(tapers[j], np.float32)
        Z = _fft32((fx * v) + 1j * (fy * v))
        Zk, Zm = Z[:, k], Z[:, (n - k) % n]
        ar, ai = Zk.real + Zm.real, Zk.imag - Zm.imag
        br, bi = Zk.imag + Zm.imag, Zm.real - Zk.real
        out[0] += c * (ar * ar + ai * ai)
        out[1] += c * (br * br + bi * bi)
        out[2] += c * (ar * br + ai * bi)
        out[3] += c * (ai * br - ar * bi)
    return out


def cross32_packed(xy32, n, overlap, tapers, sig, history_mode=0, bits=None):
    """A float32 stand-in that works as the kernel does: one packed transform per frame and taper, and the rows of a channel
    whose bit is clear stored as zeros.  bits: the per-frame silence bits it decides by (None: the frames' own) -- the criterion
    tests hand it the bits of another frame."""
    xy32 = np.asarray(xy32, np.float32)
    fr = frames64(xy32[:, 0] + 1j * xy32[:, 1].astype(np.complex64), n, overlap, history_mode)
    sxx, syy, sre, sim = _packed32(fr.real.astype(np.float32), fr.imag.astype(np.float32), tapers, sig, n)
    bits = silence_bits(xy32, n, overlap, history_mode) if bits is None else np.asarray(bits)
    sxx[(bits & 1) == 0] = 0
    syy[(bits & 2) == 0] = 0
    sre[bits != 3] = 0
    sim[bits != 3] = 0
    sxy = (sre + 1j * sim).astype(np.complex64)
    return Cross(sxx, syy, sxy, _coh(sxx, syy, sxy))


def one_pass_earlier(a, stride):
    """Per-frame (per-row) state a as a block that never refreshed it would hold it: that of the frame stride earlier."""
    a = np.asarray(a)
    out = a.copy()
    out[stride:] = a[:len(a) - stride]
    return out
