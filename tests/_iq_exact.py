"""Float64 'exact-arithmetic' two-sided rows of complex I/Q streams, and their float32 stand-in (tests only): tests/_exact.py for
complex input.

A stream is complex samples z[n] = I[n] + i Q[n] whose parts are float32 values (the sample format's conversion is input
preparation and exact).  Frame f holds samples [f H - (N - H), f H + H) with the history rules of real streams; the rows are

    periodogram   P[k] = |FFT(w z_f)[k]|^2 / N                              k = 0 .. N-1
    multitaper    P[k] = sum_j |FFT(v_j z_f)[k]|^2 / N / (1 + sig_j)

in float64 (numpy.fft.fft on complex128).  The stand-in keeps the same frames and goes float32 all the way: complex64 frame x
float32 table, torch.fft.fft on CPU complex64 tensors row by row (pocketfft, accurate twiddles), |Z|^2 / N, weights and the
taper sum in float32.
"""
import numpy as np

from _exact import hop_len


def frames64(z, n, overlap, history_mode=0):
    """The assembled frames as complex128 rows of the complex64 samples."""
    h = hop_len(n, overlap)
    z = np.asarray(z, np.complex64)
    nfr = len(z) // h
    out = np.zeros((nfr, n), np.complex128)
    for f in range(nfr):
        lo = f * h - (n - h)
        if history_mode:
            out[f, n - h:] = z[f * h:(f + 1) * h]
        else:
            a = max(lo, 0)
            out[f, a - lo:] = z[a:f * h + h]
    return out


def periodogram64(z, n, overlap, window32, history_mode=0):
    fr = frames64(z, n, overlap, history_mode)
    return np.abs(np.fft.fft(fr * np.asarray(window32, np.float64), axis=1)) ** 2 / n


def multitaper64(z, n, overlap, tapers, sig, history_mode=0):
    fr = frames64(z, n, overlap, history_mode)
    out = np.zeros((fr.shape[0], n))
    for j in range(len(sig)):
        out += np.abs(np.fft.fft(fr * tapers[j], axis=1)) ** 2 / n / (1.0 + sig[j])
    return out


def _fft32(rows):
    """Row by row, as tests/_exact.py's _rfft32: the batched transform is another algorithm at large N."""
    import torch
    rows = np.ascontiguousarray(rows, np.complex64)
    out = np.empty_like(rows)
    for f in range(rows.shape[0]):
        out[f] = torch.fft.fft(torch.from_numpy(rows[f])).numpy()
    return out


def _power32(Z, n):
    return (Z.real * Z.real + Z.imag * Z.imag) / np.float32(n)


def periodogram32(z, n, overlap, window32, history_mode=0):
    fr = frames64(z, n, overlap, history_mode).astype(np.complex64)                       # (exact: the parts are float32 values)
    return _power32(_fft32(fr * np.asarray(window32, np.float32)), n)


def multitaper32(z, n, overlap, tapers, sig, history_mode=0, ntap=None):
    """ntap: only the first ntap tapers (the criterion test's 'last taper dropped')."""
    fr = frames64(z, n, overlap, history_mode).astype(np.complex64)
    out = np.zeros((fr.shape[0], n), np.float32)
    for j in range(len(sig) if ntap is None else ntap):
        wj = np.float32(1.0 / (1.0 + sig[j]))
        out += _power32(_fft32(fr * np.asarray(tapers[j], np.float32)), n) * wj
    return out
