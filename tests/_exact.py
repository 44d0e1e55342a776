"""Float64 'exact-arithmetic' rows for the parity bounds at large N (tests only).

At N >= 8192 the reference's float32 transform with its recurrence twiddles (fft_radix2.c:127-141) is
itself ~1e-5 (peak-normalised) away from exact arithmetic on noise-like frames, so parity is stated as
err(device, oracle) <= max(1e-5, 1.1 x err(oracle, exact)).  'exact' here = the same frames -- the samples
as floats, each hop's mean removed EXACTLY as fft.c:88-95 does it (a float sum sample after sample, a float
quotient, a float subtraction: that is input preparation, reproduced bit for bit) -- then window / tapers,
transform, |X|^2 / N and the taper sum in float64.
"""
import numpy as np


def hop_len(n, overlap):
    return int(n * (1.0 - float(np.float32(overlap))))                       # fft.c:70


def remove_hop_means(x, h):
    """fft.c:86-96 on every whole hop of a float32 stream (a copy)."""
    x = np.array(x, np.float32, copy=True)
    for j in range(len(x) // h):
        seg = x[j * h:(j + 1) * h]
        s = np.cumsum(seg, dtype=np.float32)[-1]                             # sequential float sum
        mean = np.float32(s) / np.float32(h)
        seg -= mean
    return x


def frames64(x, n, overlap, sub_mean=0, history_mode=0):
    """The assembled frames (fft.c:98-113) as float64 rows of the float32 samples."""
    h = hop_len(n, overlap)
    x = remove_hop_means(x, h) if sub_mean else np.asarray(x, np.float32)
    nfr = len(x) // h
    out = np.zeros((nfr, n))
    for f in range(nfr):
        lo = f * h - (n - h)
        if history_mode:
            out[f, n - h:] = x[f * h:(f + 1) * h]
        else:
            a = max(lo, 0)
            out[f, a - lo:] = x[a:f * h + h]
    return out


def periodogram64(x, n, overlap, window32, sub_mean=0, history_mode=0):
    fr = frames64(x, n, overlap, sub_mean, history_mode)
    return np.abs(np.fft.rfft(fr * np.asarray(window32, np.float64), axis=1)) ** 2 / n      # fft.c:203-226


def ftest64(x, n, overlap, tapers, kmax, sub_mean=0, history_mode=0):
    """The harmonic F statistic's parts as mtm.c:165-233 defines them, per frame and bin in float64:
    (num, den, tot), each [frames][n/2+1].  num = kmax |mu|^2 sum(U0^2) with mu the spectrum of the frame under
    hn = sum_j U0_j v_j / sum(U0^2) (mtm.c:76-83, 124-136, 165-174), den = sum_j |y_j - mu U0_j|^2 (mtm.c:203-210; the
    reference never accumulates it at Nyquist, here it is the plain sum there too), tot = sum_j |y_j|^2."""
    fr = frames64(x, n, overlap, sub_mean, history_mode)
    v = np.asarray(tapers, np.float64)[:kmax + 1]
    U0 = v.sum(axis=1)
    s2 = (U0 * U0).sum()
    hn = (U0[:, None] * v).sum(axis=0) / s2
    mu = np.fft.rfft(fr * hn, axis=1)
    num = kmax * np.abs(mu) ** 2 * s2
    den = np.zeros_like(num)
    tot = np.zeros_like(num)
    for j in range(kmax + 1):
        y = np.fft.rfft(fr * v[j], axis=1)
        den += np.abs(y - mu * U0[j]) ** 2
        tot += np.abs(y) ** 2
    return num, den, tot


def multitaper64(x, n, overlap, tapers, sig, sub_mean=0, history_mode=0):
    fr = frames64(x, n, overlap, sub_mean, history_mode)
    out = np.zeros((fr.shape[0], n // 2 + 1))
    for j in range(len(sig)):                                                                # mtm.c:189-220
        out += np.abs(np.fft.rfft(fr * tapers[j], axis=1)) ** 2 / n / (1.0 + sig[j])
    return out


def spectrum64(x, n, overlap, window32, sub_mean=0, history_mode=0):
    """The unnormalised spectra X_k, k = 0 .. n/2, of the windowed frames: complex128 rows (P_k = |X_k|^2 / n)."""
    fr = frames64(x, n, overlap, sub_mean, history_mode)
    return np.fft.rfft(fr * np.asarray(window32, np.float64), axis=1)


# ---- the float32 stand-in: what a correct float32 kernel can reach (tests/_rows_check.py takes its bounds from it) ----
# The same frames (float32 samples, hop means removed as the reference does), then float32 all the way: the frame times the
# float32 window / taper, torch.fft.rfft on CPU tensors in float32 (pocketfft: accurate twiddles), |X|^2 / n, the taper
# weights and the taper sum in float32.  Independent of the device's and of the reference's transform.
def _rfft32(rows32):
    """Row by row: the batched transform of the same library is another algorithm at large N (measured at N = 1 048 576, three
    rows: 2.4e-6 of the row's norm against 7e-8 row by row) and would set the bounds by the batch's shape."""
    import torch
    rows32 = np.ascontiguousarray(rows32, np.float32)
    out = np.empty((rows32.shape[0], rows32.shape[1] // 2 + 1), np.complex64)
    for f in range(rows32.shape[0]):
        out[f] = torch.fft.rfft(torch.from_numpy(rows32[f])).numpy()
    return out


def spectrum32(x, n, overlap, window32, sub_mean=0, history_mode=0):
    fr = frames64(x, n, overlap, sub_mean, history_mode).astype(np.float32)              # (exact: they are float32 values)
    return _rfft32(fr * np.asarray(window32, np.float32))


def _power32(X, n):
    return (X.real * X.real + X.imag * X.imag) / np.float32(n)


def periodogram32(x, n, overlap, window32, sub_mean=0, history_mode=0):
    return _power32(spectrum32(x, n, overlap, window32, sub_mean, history_mode), n)


def multitaper32(x, n, overlap, tapers, sig, sub_mean=0, history_mode=0):
    fr = frames64(x, n, overlap, sub_mean, history_mode).astype(np.float32)
    out = np.zeros((fr.shape[0], n // 2 + 1), np.float32)
    for j in range(len(sig)):
        wj = np.float32(1.0 / (1.0 + sig[j]))
        out += _power32(_rfft32(fr * np.asarray(tapers[j], np.float32)), n) * wj
    return out
