"""The bin-by-bin acceptance rule for harmonic F rows (tests only).

tests/_ftest_check.py bounds an F value by the frame's LARGEST num and den: on tonal input the bound at a weak line is larger
than the line's F.  Here, per frame and bin k < N/2, with num, den, tot from tests/_exact.py::ftest64 in float64 and

    a = sqrt(num),  b = sqrt(den),  f = a / b,     A = sqrt(sum_k num),  T = sqrt(sum_k tot)   (sums over the bins below Nyquist)

    | sqrt(got[k]) - f[k] | * b[k]   <=   tau * ( A + f[k] * ( T + A / sqrt(kmax) ) )        for EVERY bin k < N/2          (1)

The rounding model of tests/_rows_check.py applied to a quotient.  The numerator's mu is one transform: its amplitude error is at
most tau A whatever the bin's own size.  Each residual y_j - mu U0_j is linear in transforms, |d r_j| <= tau (|y_j| + |U0_j| |mu|)
in row norms, so by the triangle inequality over the tapers sqrt(den) carries at most tau (T + |mu| sqrt(sum U0^2)) =
tau (T + A / sqrt(kmax)).  Then d(a / b) <= (da + f db) / b.  (First order in db / b: where a bin's den is itself rounding -- a
lone tone on a bin -- db is of b's size; tests/test_ftest_rows_criterion.py asserts on every case that the float32 stand-in needs no
more than its own transforms' error under (1), and such inputs are the ones that reach it.)

No bin below Nyquist is left out, no mask, no percentile, no median.  A negative value fails; a non-finite value below Nyquist
fails where den64 > 0.  The Nyquist column is non-finite in every row.  A frame with T = 0 (silence) must hold what the oracle's
row holds: its NaN / inf pattern.

tau never comes from the device or the oracle: per case 4 * max(tau_f32, 2**-24) (_rows_check.bound), tau_f32 = tau_of_ftest() of
a float32 stand-in (tests/_exact.py::ftest32).
"""
import numpy as np

from _rows_check import FLOOR, MARGIN, bound          # noqa: F401  (the margin and the floor are the rows rule's)


def _parts(num, den, tot, kmax):
    num, den, tot = (np.asarray(v, np.float64) for v in (num, den, tot))
    assert num.ndim == 2 and num.shape == den.shape == tot.shape and kmax >= 1
    half = num.shape[1] - 1
    num, den, tot = num[:, :half], den[:, :half], tot[:, :half]
    a, b = np.sqrt(num), np.sqrt(den)
    with np.errstate(divide="ignore", invalid="ignore"):
        f = a / b
    A = np.sqrt(num.sum(axis=1))[:, None]
    T = np.sqrt(tot.sum(axis=1))[:, None]
    with np.errstate(invalid="ignore", over="ignore"):
        weight = A + f * (T + A / np.sqrt(kmax))          # (1)'s right side over tau; inf or NaN where den64 = 0
    return half, a, b, f, T[:, 0], weight


def _distance(got, half, b, f):
    """(1)'s left side, and the (frame, bin) below Nyquist that fail whatever tau is."""
    g = np.asarray(got, np.float64)[:, :half]
    held = b > 0                                          # den64 = 0 in a frame with power: f is x / 0, nothing to hold a value to
    with np.errstate(invalid="ignore"):
        bad = (g < 0) | (~np.isfinite(g) & held)
        dist = np.abs(np.sqrt(np.where(bad | ~held, 0.0, g)) - np.where(held, f, 0.0)) * b
    return np.where(held, dist, 0.0), bad


def tau_of_ftest(rows, num, den, tot, kmax):
    """(1) solved for tau over the frames with power; inf where a value fails whatever tau is."""
    half, a, b, f, T, weight = _parts(num, den, tot, kmax)
    live = T > 0
    if not live.any():
        return 0.0
    dist, bad = _distance(rows, half, b, f)
    if bad[live].any():
        return np.inf
    with np.errstate(divide="ignore", invalid="ignore"):
        need = np.where(dist[live] > 0, dist[live] / weight[live], 0.0)
    return float(need.max())


def check_ftest_rows(got, want, num, den, tot, kmax, tau, what=""):
    """Asserts (1) for every frame and bin below Nyquist, the Nyquist column and the silent frames' pattern against the oracle's
    rows `want`; returns (the largest fraction of the bound used, its frame, its bin)."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.ndim == 2 and got.shape == want.shape == np.shape(num), (what, got.shape, want.shape, np.shape(num))
    assert tau > 0
    half, a, b, f, T, weight = _parts(num, den, tot, kmax)
    assert not np.isfinite(got[:, half]).any(), "%s: a finite value in the Nyquist column, first in frame %d" % (what, np.flatnonzero(np.isfinite(got[:, half]))[0])
    dead = T == 0
    for fr in np.flatnonzero(dead):
        for name, test in (("NaN", np.isnan), ("+inf", np.isposinf), ("-inf", np.isneginf)):
            assert np.array_equal(test(got[fr]), test(want[fr])), "%s: silent frame %d: the %s pattern is not the oracle's, first at bin %d" % (
                what, fr, name, np.flatnonzero(test(got[fr]) != test(want[fr]))[0])
        fin = np.isfinite(want[fr])
        assert np.array_equal(got[fr][fin], want[fr][fin]), "%s: silent frame %d: a finite value differs from the oracle's" % (what, fr)
    if dead.all():
        return 0.0, -1, -1
    live = np.flatnonzero(~dead)
    dist, bad = _distance(got, half, b, f)
    if bad[live].any():
        i, k = np.argwhere(bad[live])[0]
        raise AssertionError("%s: %d negative or non-finite values below Nyquist, first at frame %d bin %d: %r" % (
            what, int(bad[live].sum()), live[i], k, got[live[i], k]))
    with np.errstate(divide="ignore", invalid="ignore"):
        frac = np.where(dist[live] > 0, dist[live] / (tau * weight[live]), 0.0)
    i, k = np.unravel_index(int(np.argmax(frac)), frac.shape)
    worst = float(frac[i, k])
    assert worst <= 1.0, "%s: frame %d bin %d is %.3f of the bound (tau %.3e): F got %.9g, float64 %.9g (num %.6g den %.6g)" % (
        what, live[i], k, worst, tau, got[live[i], k], f[live[i], k] ** 2, a[live[i], k] ** 2, b[live[i], k] ** 2)
    return worst, int(live[i]), int(k)
