"""Float64 rows and the float32 stand-in of the periodogram's non-linear pre-processing (tests only).

prepare_audio (fft.c:127-156) after the frame is assembled: RA9MB x / (a + x^2) when a > 0 (fft.c:127-136), the window
(no multiply when it is rectangular, fft.c:132, 139), the limiter sign(y) |y|^0.1 (fft.c:151-156).  Built on tests/_exact.py:
the frames are its frames64() -- the float32 samples with each hop's mean removed as fft.c:86-96 does it, bit for bit.

  exact     float64 from the frames on: x / (a + x^2) with `a` the float32 value, times the plan's float32 window, the limiter
            as sign * exp(0.1 * log|y|) with no float temporary, `y > 0 ? + : -` as the reference writes it and y = 0 -> 0,
            np.fft.rfft, |X|^2 / n.
  stand-in  float32 from the frames on, no fused multiply-add (numpy rounds every operation): x / (a + x * x), times the
            window, the limiter exactly as the reference writes it -- ftmp = (float) log((double) |y|), exp(ftmp * 0.1) in
            double, rounded to float -- then tests/_exact.py's _rfft32 and _power32.

window32 = None stands for the rectangular window.
"""
import numpy as np

import _exact as X


def limiter64(y):
    """sign(y) |y|^0.1 in float64; y = 0 gives 0 (the reference: log 0 = -inf, exp(-inf) = 0, and -0 is 0)."""
    y = np.asarray(y, np.float64)
    mag = np.zeros_like(y)
    nz = y != 0
    mag[nz] = np.exp(0.1 * np.log(np.abs(y[nz])))
    return np.where(y > 0, mag, -mag) + 0.0                                   # (+ 0.0: -0 -> +0)


def limiter32(y):
    """fft.c:153-154 on float32 values: a float ftmp, the exponential in double, the store rounds to float."""
    y = np.asarray(y, np.float32)
    with np.errstate(divide="ignore"):
        ftmp = np.log(np.abs(y).astype(np.float64)).astype(np.float32)
    mag = np.exp(ftmp.astype(np.float64) * 0.1).astype(np.float32)
    return np.where(y > 0, mag, -mag).astype(np.float32)


def prepared64(x, n, overlap, window32, a=0.0, limiter=0, sub_mean=0, history_mode=0):
    """inbuf_fft of every frame in float64: [frames][n]."""
    y = X.frames64(x, n, overlap, sub_mean, history_mode)
    if a > 0:
        y = y / (float(np.float32(a)) + y * y)
    if window32 is not None:
        y = y * np.asarray(window32, np.float32).astype(np.float64)
    return limiter64(y) if limiter else y


def prepared32(x, n, overlap, window32, a=0.0, limiter=0, sub_mean=0, history_mode=0):
    """inbuf_fft of every frame the way the reference computes it, operation by operation in float32: [frames][n]."""
    y = X.frames64(x, n, overlap, sub_mean, history_mode).astype(np.float32)  # (exact: they are float32 values)
    if a > 0:
        y = y / (np.float32(a) + y * y)
    if window32 is not None:
        y = y * np.asarray(window32, np.float32)
    assert y.dtype == np.float32
    return limiter32(y) if limiter else y


def spectrum64(x, n, overlap, window32, a=0.0, limiter=0, sub_mean=0, history_mode=0):
    """The unnormalised spectra X_k, k = 0 .. n/2, of the prepared frames (what run(spectrum=True) returns): complex128."""
    return np.fft.rfft(prepared64(x, n, overlap, window32, a, limiter, sub_mean, history_mode), axis=1)


def periodogram64(x, n, overlap, window32, a=0.0, limiter=0, sub_mean=0, history_mode=0):
    return np.abs(spectrum64(x, n, overlap, window32, a, limiter, sub_mean, history_mode)) ** 2 / n      # fft.c:203-226


def spectrum32(x, n, overlap, window32, a=0.0, limiter=0, sub_mean=0, history_mode=0):
    return X._rfft32(prepared32(x, n, overlap, window32, a, limiter, sub_mean, history_mode))


def periodogram32(x, n, overlap, window32, a=0.0, limiter=0, sub_mean=0, history_mode=0):
    return X._power32(spectrum32(x, n, overlap, window32, a, limiter, sub_mean, history_mode), n)
