"""The bin-by-bin acceptance rule for HP-ARMA rows (tests only).

An HP-ARMA row is N / |A(f)|^2 below Nyquist and |A(f)|^2 / N at Nyquist (hparma.c:140-156), A(f) = sum_m a[m] z^m the
spectrum of the frame's AR vector a.  The suite's older tests hold |A|^2 / N to max(1e-5, 3 s) OF THE ROW'S LARGEST BIN; a
spectral line is a bin 1e4 ... 1e8 times below that, so the peaks of the rows -- what the estimator is for -- are free.
Here, per frame, with
    a       the ORACLE's AR vector (oracle.hparma_frames)
    q64[k]  | sum_m a[m] z_k^m |^2 / N in float64 at the exact angles, k = 0 ... N/2                     (q64())
    q_got   the row under test with the reciprocal undone below Nyquist, the Nyquist bin as it is         (undo())
every bin, DC and Nyquist included, must meet tests/_rows_check.py's rule (1)

    | sqrt(q_got[k]) - sqrt(q64[k]) |  <=  (tau_eval + tau_cond) * sqrt( sum_k q64[k] )

tau_eval = 4 max(tau_f32, 2^-24) (_rows_check.bound): tau_f32 is tau_of() of a plain float32 evaluation of the same a (q32():
the zero-padded float32 transform of tests/_exact.py).  The device evaluates a double Horner over a float32 unit-circle
table, which sits at 0.8 x 2^-24.
tau_cond = 3 s_amp: a is a noise-subspace direction of a nearly rank-deficient matrix, and an implementation that does not
replay the reference's every rounding lands on a neighbouring a.  s_amp (spread()) is the largest value of the same left-hand
side, over the stream's frames and the draws, between q64 of the oracle's a on the input and on its 1-ulp perturbations
(_spread.ulp_perturbations) -- two float64 evaluations, so the reference's own transform is not in it.  3 is the project's
factor for a sampled maximum (_spread.hparma_bound says why 1.1 fails for no defect).  The stream's maximum, not a frame's:
a frame's dozen draws are exceeded by the next dozen by up to 3.6 x.

The shape of a row is the oracle's: NaN where it is NaN (digital silence with p_e >= 5: every bin), inf where it is inf (A
has a zero on the unit circle at that bin).  Where the oracle's rank is p_e or more (white input; silence with p_e <= 4,
whose rank stays at its initial 4) a = e_0 and the row is N below Nyquist and 1 / N at Nyquist, powers of two: compared as
bits.

peak_figure() is the older tests' figure, kept beside the new one in every record.
"""
import functools

import numpy as np

import _exact as X
from _rows_check import bound, tau_of
from _signals import rel_err
from _spread import ulp_perturbations

COND = 3.0


@functools.lru_cache(maxsize=8)
def _circle(ncol, n):
    """z_k^m at the exact angles: m k is reduced mod n in integers before it becomes an angle."""
    m = np.arange(ncol, dtype=np.int64)[:, None]
    k = np.arange(n // 2 + 1, dtype=np.int64)[None, :]
    return np.exp(-2j * np.pi * ((m * k) % n) / n)


def q64(a, n):
    """|A(f_k)|^2 / N, k = 0 ... N/2, of the AR vectors a [frames][p_e + 1] in float64; a row of NaN for a vector that is not finite."""
    a = np.atleast_2d(np.asarray(a, np.float64))
    out = np.full((a.shape[0], n // 2 + 1), np.nan)
    fin = np.isfinite(a).all(axis=1)
    if fin.any():
        A = a[fin] @ _circle(a.shape[1], n)
        out[fin] = (A.real ** 2 + A.imag ** 2) / n
    return out


def q32(a, n):
    """The same by a plain float32 transform of the zero-padded vector (finite vectors only)."""
    a = np.atleast_2d(np.asarray(a, np.float32))
    padded = np.zeros((a.shape[0], n), np.float32)
    padded[:, :a.shape[1]] = a
    return X._power32(X._rfft32(padded), n)


def undo(rows, n):
    """Rows as the estimator writes them -> |A|^2 / N: the reciprocal undone below Nyquist (1 / inf = 0), float64."""
    q = np.array(rows, np.float64)
    with np.errstate(divide="ignore"):
        q[:, :n // 2] = 1.0 / q[:, :n // 2]
    return q


def rows_of(q, n):
    """|A|^2 / N in float64 -> rows as a float32 estimator stores them: the value in float, its reciprocal below Nyquist."""
    ps = np.asarray(q, np.float64).astype(np.float32)
    out = ps.copy()
    with np.errstate(divide="ignore"):
        out[:, :n // 2] = (1.0 / ps[:, :n // 2].astype(np.float64)).astype(np.float32)
    return out


def finite_frames(a):
    return np.isfinite(np.atleast_2d(np.asarray(a, np.float64))).all(axis=1)


def amp_tau(q, exact):
    """tau_of over the frames whose exact row is finite (0.0 if there is none)."""
    fin = np.isfinite(exact).all(axis=1)
    return tau_of(np.asarray(q)[fin], exact[fin]) if fin.any() else 0.0


def spread(frames_of, xf, ref, n, draws=12, seed=0):
    """(s_amp, s_peak): the largest amplitude movement of q64 and the largest peak-normalised movement of 1 / psd
    (_spread.hparma_spread's figure) of the oracle over the stream's frames under `draws` 1-ulp perturbations of xf.
    frames_of(x) -> oracle.hparma_frames' list; ref: that list for xf itself.  s_amp is NaN where no frame has a finite AR
    vector, inf where a perturbation changes which frames have one."""
    a = np.stack([r[1] for r in ref])
    exact = q64(a, n)
    fin = finite_frames(a)
    s_amp, s_peak = (0.0 if fin.any() else np.nan), 0.0
    for xp in ulp_perturbations(np.asarray(xf, np.float32), draws, seed=seed):
        got = frames_of(xp)
        ap = np.stack([g[1] for g in got])
        if not np.array_equal(finite_frames(ap), fin):
            return np.inf, np.inf
        if fin.any():
            s_amp = max(s_amp, tau_of(q64(ap[fin], n), exact[fin]))
        for f in np.flatnonzero(fin):
            with np.errstate(divide="ignore"):
                v, w = 1.0 / got[f][0].astype(np.float64)[:n // 2], 1.0 / ref[f][0].astype(np.float64)[:n // 2]
            ok = np.isfinite(v) & np.isfinite(w)
            s_peak = max(s_peak, rel_err(v[ok], w[ok])[0])
    return s_amp, s_peak


def peak_figure(rows, want, n):
    """The older tests' figure, the worst frame's: max(max-norm, 2-norm) error of |A|^2 / N below Nyquist against the oracle's,
    over the largest bin, and the Nyquist bin's error over the same (test_hparma_parity).  Frames that are not finite in
    the oracle are left out."""
    rows, want = np.asarray(rows, np.float64), np.asarray(want, np.float64)
    worst = 0.0
    for f in range(len(want)):
        if not np.isfinite(want[f]).all() or not np.isfinite(rows[f]).all():
            continue
        g, w = 1.0 / rows[f, :n // 2], 1.0 / want[f, :n // 2]
        worst = max(worst, max(rel_err(g, w)), abs(rows[f, n // 2] - want[f, n // 2]) / np.abs(w).max())
    return worst


def check(rows, want, a, rank, n, p_e, tau, what=""):
    """Asserts the rule on the rows of one stream: the oracle's finiteness pattern (want: its rows), the exact rows where
    rank >= p_e, and (1) with tau = tau_eval + tau_cond on every bin of every frame with a finite AR vector.  Returns the
    largest fraction of the bound used (0.0 where no frame has one)."""
    rows, want = np.asarray(rows), np.asarray(want)
    assert rows.shape == want.shape == (len(a), n // 2 + 1), (what, rows.shape, want.shape)
    fin = finite_frames(a)
    for f in range(len(want)):
        assert np.array_equal(np.isnan(rows[f]), np.isnan(want[f])), "%s: frame %d: %d NaN bins, the oracle's row has %d" % (
            what, f, int(np.isnan(rows[f]).sum()), int(np.isnan(want[f]).sum()))
        assert np.array_equal(np.isinf(rows[f]), np.isinf(want[f])), "%s: frame %d: inf at bins %s, the oracle's at %s" % (
            what, f, np.flatnonzero(np.isinf(rows[f]))[:8], np.flatnonzero(np.isinf(want[f]))[:8])
        if not fin[f]:
            assert np.isnan(want[f]).all(), (what, f)                   # (the oracle's row of a NaN vector: NaN in every bin)
        if rank[f] >= p_e:
            flat = np.full(n // 2 + 1, n, np.float32)
            flat[n // 2] = np.float32(1.0) / np.float32(n)
            assert np.array_equal(np.asarray(rows[f], np.float32).view(np.uint32), flat.view(np.uint32)), "%s: frame %d (rank %d): not N and 1 / N" % (what, f, rank[f])
    if not fin.any():
        return 0.0
    assert tau > 0 and np.isfinite(tau), (what, tau)
    q, exact = undo(rows[fin], n), q64(np.asarray(a)[fin], n)
    bad = ~np.isfinite(q) | (q < 0)
    assert not bad.any(), "%s: |A|^2 / N not finite or negative at (frame, bin) %s" % (what, tuple(np.argwhere(bad)[0]))
    s = np.sqrt(exact.sum(axis=1))
    frac = np.abs(np.sqrt(q) - np.sqrt(exact)) / (tau * s[:, None])
    i, k = np.unravel_index(int(np.argmax(frac)), frac.shape)
    worst = float(frac[i, k])
    assert worst <= 1.0, "%s: frame %d bin %d is %.3f of the bound (tau %.3e): |A|^2 / N %.9g, float64 %.9g, row sum %.6g" % (
        what, np.flatnonzero(fin)[i], k, worst, tau, q[i, k], exact[i, k], s[i] ** 2)
    return worst


def fraction(rows, a, n, tau):
    """The largest fraction of the bound without asserting it (inf for a row that is not finite where the vector is)."""
    fin = finite_frames(a)
    if not fin.any():
        return 0.0
    return amp_tau(undo(np.asarray(rows)[fin], n), q64(np.asarray(a)[fin], n)) / tau


def tau_eval(a, n):
    """(tau_f32, tau_eval) of the finite AR vectors of a stream."""
    fin = finite_frames(a)
    if not fin.any():
        return 0.0, bound(0.0)
    t32 = tau_of(q32(np.asarray(a)[fin], n), q64(np.asarray(a)[fin], n))
    return t32, bound(t32)
