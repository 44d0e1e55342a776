"""The bin-by-bin rule for Spectrogram.cross rows against tests/_cross_exact.py's float64 (tests only).

Per frame, with the float64 rows: a = sqrt(Sxx64), b = sqrt(Syy64), g = |Sxy64| / (a b) (0 where a b = 0) and
A = sqrt(sum_k (Sxx64 + Syy64)).  For EVERY bin of every frame, DC and Nyquist included:

    | sqrt(Sxx_got) - a |          <= tau A                                          (1; the same for Syy: 2)
    | Sxy_got - Sxy64 |            <= tau A (a + b) + tau^2 A^2                      (3)
    | sqrt(coh_got) - g | a b      <= tau A (a + b) (1 + g) + tau^2 A^2              (4; bins with a b = 0: coh_got == 0)

tau = 4 max(tau_f32, 2^-24), where tau_f32 is the smallest tau at which the float32 stand-in (_cross_exact.cross32) satisfies the
four lines on that case: computed on the CPU per case, never from device output.  4 is the margin of every bin-by-bin module here.

Where the lines come from.  Write a bin's weighted spectra as vectors over the tapers, X = (sqrt(c_j) X_j)_j, Y likewise: a = |X|,
b = |Y|, Sxy = <X, Y>.  Both channels ride ONE packed transform, so what an implementation in float32 owes is an error vector of
each channel bounded by the rounding of the pair: |dX|, |dY| <= u = tau' A.  Then
    (1, 2)  | |X + dX| - a | <= u
    (3)     | d<X, Y> | <= |dX| b + a |dY| + |dX| |dY| <= u (a + b) + u^2 =: E(u)
    (4)     with s = sqrt(coh_got) in [0, 1] and s a' b' = |Sxy'| (a' = |X + dX|, b' likewise; the clamp only lowers s):
            |s - g| a b <= s |a b - a' b'| + | |Sxy'| - |Sxy| | <= (1 + s) E(u) <= 2 E(u)
The issue's line 4 has (1 + g) on the first-order term alone -- (1 + s) E(u) to first order, tighter beyond it.  It is kept as
stated: an implementation whose error vectors stay within u = (tau / 4) A, the margin's premise, has 2 E(u) = tau A (a + b) / 2 +
tau^2 A^2 / 8, which is under the right side of line 4 whatever g is.  No constant here comes from device output.
"""
import numpy as np

FLOOR = 2.0 ** -24
MARGIN = 4.0


def _terms(got, ref):
    """Per bin: the four left sides e_i and the coefficients (c_i, q_i) of the right sides tau A c_i + q_i tau^2 A^2."""
    a, b = np.sqrt(ref.sxx), np.sqrt(ref.syy)
    ab = a * b
    g = np.where(ab > 0, np.abs(ref.sxy) / np.where(ab > 0, ab, 1.0), 0.0)
    A = np.sqrt((ref.sxx + ref.syy).sum(axis=1, keepdims=True)) + 0.0 * a
    one, zero = np.ones_like(a), np.zeros_like(a)
    gsxx, gsyy = np.asarray(got.sxx, np.float64), np.asarray(got.syy, np.float64)
    gcoh = np.asarray(got.coh, np.float64)
    e = [np.abs(np.sqrt(gsxx) - a), np.abs(np.sqrt(gsyy) - b), np.abs(np.asarray(got.sxy, np.complex128) - ref.sxy),
         np.abs(np.sqrt(gcoh) - g) * ab]
    c = [one, one, a + b, (a + b) * (1.0 + g)]
    q = [zero, zero, one, one]
    return e, c, q, A, ab


def needed_tau(got, ref):
    """The smallest tau at which `got` satisfies the four lines (the zero-product rule aside)."""
    e, c, q, A, _ = _terms(got, ref)
    worst = 0.0
    for ei, ci, qi in zip(e, c, q):
        # u = tau A:  qi u^2 + ci u - ei >= 0  <=>  u >= 2 ei / (ci + sqrt(ci^2 + 4 qi ei))
        den = ci + np.sqrt(ci * ci + 4.0 * qi * ei)
        with np.errstate(divide="ignore", invalid="ignore"):
            u = np.where(ei > 0, 2.0 * ei / den, 0.0)
            t = np.where(u > 0, u / A, 0.0)
        worst = max(worst, float(np.nanmax(t)) if t.size else 0.0)
    return worst


def tau_of(stand_in, ref):
    return MARGIN * max(needed_tau(stand_in, ref), FLOOR)


def fraction(got, ref, tau):
    """The largest left side over its right side, over the four lines and all bins (inf where a right side of 0 is exceeded, or
    coh_got != 0 on a bin with a b = 0, or anything is not finite)."""
    e, c, q, A, ab = _terms(got, ref)
    worst = 0.0
    for arr in (got.sxx, got.syy, got.coh, np.abs(np.asarray(got.sxy))):
        if not np.isfinite(np.asarray(arr, np.float64)).all():
            return np.inf
    if (np.asarray(got.coh)[ab == 0] != 0).any() or (np.asarray(got.coh) < 0).any() or (np.asarray(got.coh) > 1).any():
        return np.inf
    for ei, ci, qi in zip(e, c, q):
        rhs = tau * A * ci + qi * (tau * A) ** 2
        with np.errstate(divide="ignore", invalid="ignore"):
            f = np.where(ei > rhs, np.where(rhs > 0, ei / rhs, np.inf), np.where(rhs > 0, ei / rhs, 0.0))
        worst = max(worst, float(f.max()))
    return worst


def check(got, ref, tau, what=""):
    f = fraction(got, ref, tau)
    print("cross-rows %s tau=%.3e fraction=%.3f" % (what, tau, f))
    assert f <= 1.0, (what, tau, f)
    return f
