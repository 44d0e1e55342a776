"""The rule the jackknife row is held to, for every bin of every frame, DC and Nyquist included (tests only).

It is written for s = sqrt(logvar), the quantity Student's quantile multiplies.  With E64 the float64 eigenspectra of a case, w* the
reference weights, (S*, s*^2, min_i S*_(i)) = jackknife64(E64, w*), A = _adaptive_check.amplitude(E64) per frame and
tau = _adaptive_check.eigen_tau of the case (from the float32 stand-in's eigenspectra, never from device output):

    |s_got - s*| <= sqrt(K-1) ( -2 ln(1 - tau A / sqrt(min_i S*_(i))) + REL_LOG )

WHY.  s = sqrt((K-1)/K) |l - lbar|_2 over the K values l_i.  If every l_i moves by at most eps, the centred vector moves by at most
sqrt(K) eps in the 2-norm (centring is a projection), so s moves by at most sqrt(K-1) eps: the triangle inequality.  A delete-one
estimate is a weighted mean of eigenspectra, its square root a weighted 2-norm of the amplitudes sqrt(E_j), which the device knows
to tau A each: sqrt(S_(i)) moves by at most tau A, a relative r = tau A / sqrt(S*_(i)), and ln S_(i) by at most -2 ln(1 - r).
The reference point S cancels in the centring, so its own error does not enter.

REL_LOG covers what float32 adds for GIVEN eigenspectra, per l_i:
    the weights          each w_j is lambda_j u_j^2 from the given S and the frame's sigma2: about 32 roundings, delta <= 2^-19
                         (_adaptive_check's count); a weighted mean whose weights move by 1 +- delta each moves by at most
                         (1 + delta) / (1 - delta): 2 delta = 2^-18 in the logarithm.  (iters = 0: the weights are exact.)
    the two K-1 term sums  non-negative terms, one rounding each: 2 * 7 * 2^-24
    the two quotients    S_(i) and its ratio to S: 2 * 2^-24
    the logarithm        2 ulp of l_i.  A bin under the rule has min_i S*_(i) >= (8 tau A)^2, S is a convex combination of the
                         S_(i) and none exceeds A^2, so |l_i| <= 2 ln(1 / (8 tau)) <= 2 ln 2^19 = 26.4 < 32: an ulp is at most
                         2^-19, two of them 2^-18
    the deviation        l_i - lbar, one rounding of a value below 32: 2^-20.  (The error of lbar itself shifts every deviation
                         alike and enters s in second order only.)
  sum: 2^-18 + 2^-18 + 2^-20 + 2^-20 = 1.375 * 2^-17; with this project's factor 2 over, rounded up to a power of two:
    REL_LOG = 2^-15
(tests/test_jackknife_criterion.py holds the stand-in inside a quarter of it.)

THE REFERENCE WEIGHTS are chained as the adaptive rule is: for iters = m + 1 >= 2 those of weights64 from the device's own psd_m
(a second call with iters = m); for iters = 0 the float32 lambda_j taken as doubles.  iters = 1 is held only to bits and
finiteness: at m = 0 the weights inherit the start value's error (_adaptive_check.start_dof_widen).

BELOW THE FLOOR.  A bin with tau A / sqrt(min_i S*_(i)) >= 1/8 lies below the float32 floor of its frame: there only
"non-negative or +inf, never NaN" is asserted.  How many such bins a case may have is a condition on the CASE, decided from
float64 alone (excluded_share; the callers assert it).  A silent frame (A == 0) must give exactly 0.
"""
import numpy as np

from _adaptive_check import _ratio, amplitude
from _jackknife_exact import jackknife64

REL_LOG = 2.0 ** -15
FLOOR_R = 1.0 / 8.0
NOISE_SHARE = 1e-3


def floor_ratio(E64, w, tau):
    """(r = tau A / sqrt(min_i S*_(i)) per bin (inf where that minimum is 0, 0 in a silent frame), s*, S*)."""
    S, lv, smin = jackknife64(E64, w)
    A = amplitude(E64)[:, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(A > 0, tau * A / np.sqrt(np.where(smin > 0, smin, 1.0)), 0.0)
    r = np.where((A > 0) & (smin <= 0), np.inf, r)
    return r, np.sqrt(lv), S


def excluded_share(E64, w, tau):
    """The share of a case's bins that lie below the floor, and the mask; from float64 alone."""
    r = floor_ratio(E64, w, tau)[0]
    return float((r >= FLOOR_R).mean()), r >= FLOOR_R


def rule(logvar, E64, w, tau, rel=1.0):
    """The rule on one call's logvar row set against the reference weights w.  rel scales REL_LOG (the criterion test: 0.25).
    Returns (the largest fraction of the bound, the excluded share); asserts the rule."""
    K = E64.shape[1]
    got = np.asarray(logvar, np.float64)
    assert not np.isnan(got).any(), "a NaN logvar"
    assert (got >= 0).all(), "a negative logvar"
    r, s_ref, _ = floor_ratio(E64, w, tau)
    silent = amplitude(E64) == 0
    assert (got[silent] == 0).all(), "a silent frame's logvar is not 0"
    held = r < FLOOR_R
    with np.errstate(divide="ignore", invalid="ignore"):
        bound = np.sqrt(K - 1.0) * (-2.0 * np.log1p(-np.where(held, r, 0.0)) + rel * REL_LOG)
        err = np.abs(np.sqrt(got) - s_ref)                       # (inf - inf: a NaN, counted as a miss below)
    err = np.where(np.isnan(err), np.where(np.isinf(got) & np.isinf(s_ref), 0.0, np.inf), err)
    frac = _ratio(err[held], bound[held])
    assert frac <= 1.0, ("jackknife rule", frac)
    return frac, float((~held).mean())
