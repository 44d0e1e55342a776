"""The bin-by-bin acceptance rule for estimator rows (tests only).

For a row `got` (float32) and the same row `exact` in float64 (tests/_exact.py):

    | sqrt(got[k]) - sqrt(exact[k]) |  <=  tau * sqrt( sum_k exact[k] )        for EVERY bin k              (1)

The rounding model of a float32 transform: each spectrum value carries an error e of the size u sqrt(log N) ||frame||
whatever the bin's own size, and |dP| <= 2 sqrt(P) e + e^2 is exactly |sqrt(P + dP) - sqrt(P)| <= e.  For a weighted sum
of eigenspectra (the multitaper row, a moving average of rows) the same form holds by Cauchy-Schwarz.  No bin is left
out, no mask, no percentile.  A non-finite or negative value fails; a row whose exact sum is 0 must be 0 in every bin.

tau never comes from the device: per case it is  4 * max(tau_f32, 2**-24)  (bound()), tau_f32 = tau_of() of the float32
stand-in of tests/_exact.py.  2**-24: storing a PSD value in float32 alone moves the amplitude of a bin that holds the
whole row's power by u/2.  4: the device's transform is a third float32 algorithm with a few more roundings of size u per
value than pocketfft's (about 2x in rms), and the worst of ~1e5 bins of a near-Gaussian error differs by ~1.3x between
two draws.
"""
import numpy as np

FLOOR = 2.0 ** -24
MARGIN = 4.0


def bound(tau_f32):
    return MARGIN * max(float(tau_f32), FLOOR)


def _scale(exact):
    return np.sqrt(np.asarray(exact, np.float64).sum(axis=1))


def tau_of(rows, exact):
    """(1) solved for tau: the largest |sqrt(rows) - sqrt(exact)| / sqrt(sum exact) over the frames with power."""
    rows, exact = np.asarray(rows, np.float64), np.asarray(exact, np.float64)
    assert rows.shape == exact.shape and rows.ndim == 2
    if not (np.isfinite(rows).all() and (rows >= 0).all()):
        return np.inf
    s = _scale(exact)
    live = s > 0
    if not live.any():
        return 0.0
    dev = np.abs(np.sqrt(rows[live]) - np.sqrt(exact[live])).max(axis=1)
    return float((dev / s[live]).max())


def check_rows(got, exact, tau, what=""):
    """Asserts (1) for every frame and bin; returns the largest fraction of the bound used."""
    got, exact = np.asarray(got, np.float64), np.asarray(exact, np.float64)
    assert got.shape == exact.shape and got.ndim == 2, (what, got.shape, exact.shape)
    assert tau > 0
    bad = ~np.isfinite(got) | (got < 0)
    assert not bad.any(), "%s: %d non-finite or negative values, first at (frame, bin) %s" % (what, int(bad.sum()), tuple(np.argwhere(bad)[0]))
    s = _scale(exact)
    dead = s == 0
    if dead.any():
        f = np.flatnonzero(dead)
        nz = got[f] != 0
        assert not nz.any(), "%s: frame %d has no power and bin %d holds %g" % (what, f[np.argwhere(nz)[0][0]], np.argwhere(nz)[0][1], got[f][nz][0])
    if dead.all():
        return 0.0
    live = np.flatnonzero(~dead)
    frac = np.abs(np.sqrt(got[live]) - np.sqrt(exact[live])) / (tau * s[live, None])
    i, k = np.unravel_index(int(np.argmax(frac)), frac.shape)
    worst = float(frac[i, k])
    assert worst <= 1.0, "%s: frame %d bin %d is %.3f of the bound (tau %.3e): got %.9g exact %.9g, row sum %.6g" % (
        what, live[i], k, worst, tau, got[live[i], k], exact[live[i], k], s[live[i]] ** 2)
    return worst


# ---- halfcomplex spectra: X_k unnormalised, P_k = |X_k|^2 / N; the same units as (1), so phase errors count ----------
#     | got_X[k] - exact_X[k] | / sqrt(N)  <=  tau * sqrt( sum_k P_k )
def _scale_spec(exact_X, n):
    return np.sqrt((np.abs(exact_X) ** 2).sum(axis=1) / n)


def tau_of_spectrum(X, exact_X, n):
    X, exact_X = np.asarray(X, np.complex128), np.asarray(exact_X, np.complex128)
    assert X.shape == exact_X.shape == (X.shape[0], n // 2 + 1)
    if not np.isfinite(X.view(np.float64)).all():
        return np.inf
    s = _scale_spec(exact_X, n)
    live = s > 0
    if not live.any():
        return 0.0
    return float((np.abs(X[live] - exact_X[live]).max(axis=1) / np.sqrt(n) / s[live]).max())


def check_spectrum(got_X, exact_X, n, tau, what=""):
    got_X, exact_X = np.asarray(got_X, np.complex128), np.asarray(exact_X, np.complex128)
    assert got_X.shape == exact_X.shape == (got_X.shape[0], n // 2 + 1), (what, got_X.shape, exact_X.shape)
    assert tau > 0
    assert np.isfinite(got_X.view(np.float64)).all(), "%s: non-finite values" % what
    s = _scale_spec(exact_X, n)
    dead = s == 0
    assert not got_X[dead].any(), "%s: a frame without power has a non-zero spectrum" % what
    if dead.all():
        return 0.0
    live = np.flatnonzero(~dead)
    frac = np.abs(got_X[live] - exact_X[live]) / np.sqrt(n) / (tau * s[live, None])
    i, k = np.unravel_index(int(np.argmax(frac)), frac.shape)
    worst = float(frac[i, k])
    assert worst <= 1.0, "%s: frame %d bin %d is %.3f of the bound (tau %.3e): got %r exact %r" % (
        what, live[i], k, worst, tau, got_X[live[i], k], exact_X[live[i], k])
    return worst


def from_halfcomplex(hc):
    """[frames][N] floats in the layout of fft_radix2.c:75-177 (data[k] = Re X_k, data[N-k] = Im X_k) -> complex [frames][N/2+1]."""
    hc = np.asarray(hc, np.float64)
    n = hc.shape[1]
    X = np.zeros((hc.shape[0], n // 2 + 1), np.complex128)
    X.real = hc[:, :n // 2 + 1]
    X.imag[:, 1:n // 2] = hc[:, :n // 2:-1]
    return X
