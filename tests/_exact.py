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


def _half_exponent(power):
    """odd_taper.hpp's scale_exponent, from its comment: half the binary exponent of a float32 power (power = m 2^ex with
    0.5 <= m < 1), the exponent clamped to +-120; None for a power of exactly 0 (the kernels' kSilent)."""
    power = np.float32(power)
    if power == 0:
        return None
    ex = int(np.frexp(power)[1]) if np.isfinite(power) else 0
    return max(-120, min(120, ex)) >> 1


def multitaper32_paired(x, n, overlap, tapers, sig, sub_mean=0, history_mode=0, pairs=(), scales="own"):
    """multitaper32 with the LAST taper of the frame pairs (fa, fb) of `pairs` in ONE complex float32 transform, as
    odd_taper.hpp describes the kernels for odd taper counts (written from its comments, never from device output):
    tapers 0 ... T-2 go one frame at a time; then z = sA yA + i sB yB with y = frame x last taper / 2 and s = 2^-hx, hx half
    the binary exponent of the frame's float32 power over the tapers done so far (a power of exactly 0: scale 0); the mirror
    bins separate them, E = Z[k] + conj Z[N-k] = sA Y_A[k], O = Z[k] - conj Z[N-k] = i sB Y_B[k], and |E|^2 / sA^2, |O|^2 / sB^2
    join the frames' sums.  A frame in no pair keeps multitaper32's row.
    scales: 'own' as above; 'unit' both scales 1 (a silent frame's too); 'exchanged' frame A enters and leaves with B's scale and
    B with A's -- consistent, so exact arithmetic would not notice; only the rounding level each frame sees changes."""
    assert scales in ("own", "unit", "exchanged")
    fr = frames64(x, n, overlap, sub_mean, history_mode).astype(np.float32)
    T = len(sig)
    half = n // 2
    k = np.arange(half + 1)
    w = [np.float32(1.0 / (1.0 + sig[j])) for j in range(T)]
    paired = sorted({f for p in pairs for f in p})
    assert len(paired) == 2 * len(pairs) and all(0 <= f < fr.shape[0] for f in paired), "every frame in at most one pair"
    out = multitaper32(x, n, overlap, tapers, sig, sub_mean, history_mode)
    if not pairs:
        return out
    acc = np.zeros((len(paired), half + 1), np.float32)
    for j in range(T - 1):
        acc += _power32(_rfft32(fr[paired] * np.asarray(tapers[j], np.float32)), n) * w[j]
    slot = {f: i for i, f in enumerate(paired)}
    last = np.float32(0.5) * np.asarray(tapers[T - 1], np.float32)
    for fa, fb in pairs:
        hx = [_half_exponent(acc[slot[f]].sum(dtype=np.float32)) for f in (fa, fb)]
        if scales == "unit":
            hx = [0, 0]
        elif scales == "exchanged":
            hx = hx[::-1]
        s_in = [np.float32(0.0) if h is None else np.float32(2.0 ** -h) for h in hx]
        s_out = [np.float32(0.0) if h is None else np.float32(2.0 ** (2 * h)) for h in hx]
        z = np.empty((1, n), np.complex64)
        z.real = fr[fa] * last * s_in[0]
        z.imag = fr[fb] * last * s_in[1]
        Z = _fft32(z)[0]
        Zk, Zm = Z[k], Z[(n - k) % n]
        er, ei = Zk.real + Zm.real, Zk.imag - Zm.imag
        orr, oi = Zk.real - Zm.real, Zk.imag + Zm.imag
        with np.errstate(over="ignore", invalid="ignore"):
            out[fa] = acc[slot[fa]] + (er * er + ei * ei) / np.float32(n) * w[T - 1] * s_out[0]
            out[fb] = acc[slot[fb]] + (orr * orr + oi * oi) / np.float32(n) * w[T - 1] * s_out[1]
    assert out.dtype == np.float32
    return out


# ---- the harmonic F statistic in float32 (tests/_ftest_rows_check.py takes its bounds from these) ---------------------------
def _ftest32_tables(tapers, kmax):
    """The float32 tapers and, formed in double from them and rounded once, U0_j, sum(U0^2) and hn."""
    v32 = np.asarray(tapers, np.float32)[:kmax + 1]
    v = v32.astype(np.float64)
    U0 = v.sum(axis=1)
    s2 = (U0 * U0).sum()
    hn = (U0[:, None] * v).sum(axis=0) / s2
    return v32, U0.astype(np.float32), np.float32(s2), hn.astype(np.float32)


def _ftest32_quotient(mu, ys, U0, s2, kmax, order):
    """num, den and F in float32 from the float32 spectra: the residuals, their squares, the taper sum (in `order`) and
    the quotient each rounded to float32.  The Nyquist column is num / 0, as the reference leaves it (mtm.c:206)."""
    num = np.float32(kmax) * (mu.real * mu.real + mu.imag * mu.imag) * s2
    den = np.zeros_like(num)
    for j in order:
        rr = ys[j].real - mu.real * U0[j]
        ri = ys[j].imag - mu.imag * U0[j]
        den += rr * rr + ri * ri
    assert num.dtype == den.dtype == np.float32
    low = den.copy()
    low[:, -1] = 0.0
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        return num / low, num, den


def ftest32(x, n, overlap, tapers, kmax, sub_mean=0, history_mode=0, reverse=False):
    """ftest64's frames, one float32 transform (_rfft32) per sequence -- hn, then each taper --, float32 from there on:
    (F, num, den), each [frames][n/2+1] float32.  reverse: the taper sum taken from the last taper to the first."""
    fr = frames64(x, n, overlap, sub_mean, history_mode).astype(np.float32)
    v32, U0, s2, hn = _ftest32_tables(tapers, kmax)
    mu = _rfft32(fr * hn)
    ys = [_rfft32(fr * v32[j]) for j in range(kmax + 1)]
    order = range(kmax, -1, -1) if reverse else range(kmax + 1)
    return _ftest32_quotient(mu, ys, U0, s2, kmax, order)


def _fft32(rows):
    """Complex float32 transforms row by row (see _rfft32)."""
    import torch
    rows = np.ascontiguousarray(rows, np.complex64)
    out = np.empty_like(rows)
    for f in range(rows.shape[0]):
        out[f] = torch.fft.fft(torch.from_numpy(rows[f])).numpy()
    return out


def ftest32_paired(x, n, overlap, tapers, kmax, sub_mean=0, history_mode=0):
    """The same statistic with TWO real sequences per complex transform, separated through the mirror bins: the sequences hn
    (brought to a taper's size by a power of two, taken out of mu again), taper 0 ... kmax go two at a time as the real and the
    imaginary part of z, each halved, and X_a = Z[k] + conj Z[N-k], X_b = (Z[k] - conj Z[N-k]) / i, in float32.  An odd count
    leaves the last transform's imaginary part zero."""
    fr = frames64(x, n, overlap, sub_mean, history_mode).astype(np.float32)
    v32, U0, s2, hn = _ftest32_tables(tapers, kmax)
    ex = int(np.frexp(np.sqrt(s2))[1])
    scale = np.float32(2.0 ** (ex - 1)) if s2 > 0 and 0 < ex < 64 else np.float32(1.0)
    seqs = [hn * scale] + [v32[j] for j in range(kmax + 1)]
    if len(seqs) % 2:
        seqs.append(np.zeros(n, np.float32))
    half = n // 2
    k = np.arange(half + 1)
    spectra = []
    for i in range(0, len(seqs), 2):
        z = np.empty(fr.shape, np.complex64)
        z.real = fr * (np.float32(0.5) * seqs[i])
        z.imag = fr * (np.float32(0.5) * seqs[i + 1])
        Z = _fft32(z)
        Zk, Zm = Z[:, k], Z[:, (n - k) % n]
        xa = np.empty((fr.shape[0], half + 1), np.complex64)
        xb = np.empty_like(xa)
        xa.real, xa.imag = Zk.real + Zm.real, Zk.imag - Zm.imag
        xb.real, xb.imag = Zk.imag + Zm.imag, Zm.real - Zk.real
        spectra += [xa, xb]
    mu = np.empty_like(spectra[0])
    mu.real, mu.imag = spectra[0].real * (np.float32(1.0) / scale), spectra[0].imag * (np.float32(1.0) / scale)
    return _ftest32_quotient(mu, spectra[1:kmax + 2], U0, s2, kmax, range(kmax + 1))
