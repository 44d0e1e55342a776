"""The two rules the adaptive rows are held to, for every bin of every frame, DC and Nyquist included (tests only).

With E64 the float64 eigenspectra of a case and A = sqrt(sum_k mean_j E64_j[k]) per frame:

1. The CHAINED rule, on any input.  A single sweep from a given S is a weighted mean of the eigenspectra with weights summing to 1,
   so it needs no conditioning term: with (S*, nu*) = sweep64(psd_m as float64, E64, ...) the rows after m + 1 sweeps must obey
       |sqrt(psd_{m+1}) - sqrt(S*)| <= tau A + REL_AMP sqrt(S*)        |dof_{m+1} - nu*| <= REL_DOF nu*
   (m = 0: the start value (E_0 + E_1) / 2 in float64).  tau = 4 max(tau_f32, 2^-24), tau_f32 the smallest tau at which the
   float32 stand-in's EIGENSPECTRA obey |sqrt(E32_j) - sqrt(E64_j)| <= tau A for all j, k: computed per case on the CPU, never from
   device output; the 4 is this project's margin.  The relative terms cover the float32 weights and sigma2: about 32 roundings
   give delta <= 2^-19 per weight, 2 delta in amplitude and 4 delta in nu, each with a factor 2 over: REL_AMP = 2^-17,
   REL_DOF = 2^-15 (tests/test_adaptive_criterion.py holds the stand-in inside a quarter of each).  At m = 0 alone the dof term
   is widened by the factor the stand-in measures (start_dof_widen: the derivation's miss is written there).
   Also: every value finite, 2 <= dof <= 2 K up to REL_DOF, and sqrt(min_j E_j) - bound <= sqrt(psd) <= sqrt(max_j E_j) + bound.
2. The END-TO-END rule, on noise-like inputs only: |sqrt(psd) - sqrt(adaptive64)| <= tau' A, tau' = 4 max(tau'_f32, 2^-24) with
   tau'_f32 from the stand-in's final rows at the same sweep count -- valid where the float64 result moves by at most tau' A / 4
   when the stand-in's float32 eigenspectra replace the float64 ones, which end_to_end_tau asserts.  Tone inputs are not under
   it: on a carrier's skirts the fixed-point equation has several roots.
"""
import numpy as np

from _adaptive_exact import adaptive64, start64, sweep64

REL_AMP = 2.0 ** -17
REL_DOF = 2.0 ** -15
FLOOR = 2.0 ** -24
MARGIN = 4.0


def amplitude(E64):
    """A per frame."""
    return np.sqrt(E64.mean(axis=1).sum(axis=1))


def _ratio(err, bound):
    """max err / bound over a row set; a zero bound admits a zero error only."""
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err == 0, 0.0, np.inf))
    return float(r.max()) if r.size else 0.0


def eigen_tau(E32, E64):
    """tau of a case: 4 max(tau_f32, 2^-24)."""
    A = amplitude(E64)[:, None, None]
    d = np.abs(np.sqrt(E32.astype(np.float64)) - np.sqrt(E64))
    return MARGIN * max(_ratio(d, np.broadcast_to(A, d.shape)), FLOOR)


def start_dof_widen(dof32_1, E64, lam, beta, sigma2, n):
    """The factor the dof term is widened by at m = 0: max(1, 4 f0), f0 the stand-in's own fraction of REL_DOF after its first
    sweep.  THE DERIVATION'S MISS: REL_DOF covers the rounding of the weights for a GIVEN S, and at m >= 1 the given S is the
    device's own psd_m.  At m = 0 it is the float64 start value, while the device starts from its own float32 eigenspectra: their
    error (tau A in amplitude, large against a bin far below the frame's level) moves nu through S.  The stand-in stays at 1 % of
    the term for m >= 1 and reaches 0.03 - 2.2 of it at m = 0 on tone inputs (profiles/adaptive_rows.txt), so the m = 0 term is
    widened by the measured factor with this project's margin of 4 -- per case, from the stand-in, never from device output."""
    nus = sweep64(start64(E64), E64, lam, beta, sigma2, n)[1]
    f0 = _ratio(np.abs(np.asarray(dof32_1, np.float64) - nus), REL_DOF * nus)
    return max(1.0, MARGIN * f0)


def chained(psd_m, psd_m1, dof_m1, E64, lam, beta, sigma2, n, tau, rel=1.0, dof_widen=1.0):
    """The chained rule for one step: psd_m (None: the start value) -> psd_m1, dof_m1 (None: not checked).  rel scales the two
    relative terms (the criterion test: 0.25); dof_widen: start_dof_widen's factor, applied at m = 0 only.  Returns (amplitude
    fraction, dof fraction) of the bounds; asserts they hold."""
    K = E64.shape[1]
    dof_rel = rel * REL_DOF * (dof_widen if psd_m is None else 1.0)
    S0 = start64(E64) if psd_m is None else np.asarray(psd_m, np.float64)
    Ss, nus = sweep64(S0, E64, lam, beta, sigma2, n)
    A = amplitude(E64)[:, None]
    fa = fd = 0.0
    if psd_m1 is not None:
        got = np.asarray(psd_m1, np.float64)
        assert np.isfinite(got).all() and (got >= 0).all()
        bound = tau * A + rel * REL_AMP * np.sqrt(Ss)
        fa = _ratio(np.abs(np.sqrt(got) - np.sqrt(Ss)), bound)
        lo, hi = np.sqrt(E64.min(axis=1)), np.sqrt(E64.max(axis=1))
        fa = max(fa, _ratio(np.maximum(np.sqrt(got) - hi, 0.0), bound), _ratio(np.maximum(lo - np.sqrt(got), 0.0), bound))
    if dof_m1 is not None:
        d = np.asarray(dof_m1, np.float64)
        assert np.isfinite(d).all()
        fd = _ratio(np.abs(d - nus), dof_rel * nus)
        fd = max(fd, _ratio(np.maximum(d - 2.0 * K, 0.0), np.full(d.shape, rel * REL_DOF * 2.0 * K)),
                 _ratio(np.maximum(2.0 - d, 0.0), np.full(d.shape, rel * REL_DOF * 2.0)))
    assert fa <= 1.0, ("chained rule, amplitude", fa)
    assert fd <= 1.0, ("chained rule, dof", fd)
    return fa, fd


def end_to_end_tau(psd32, E32, E64, lam, beta, sigma2, n, iters):
    """tau' of a noise-like case from the stand-in's final rows, with the condition that makes the rule valid asserted."""
    want, _ = adaptive64(E64, lam, beta, sigma2, n, iters)
    A = amplitude(E64)[:, None]
    Ab = np.broadcast_to(A, want.shape)
    taup = MARGIN * max(_ratio(np.abs(np.sqrt(psd32.astype(np.float64)) - np.sqrt(want)), Ab), FLOOR)
    moved, _ = adaptive64(E32.astype(np.float64), lam, beta, sigma2, n, iters)
    cond = _ratio(np.abs(np.sqrt(moved) - np.sqrt(want)), taup * Ab / 4.0)
    assert cond <= 1.0, ("end-to-end rule not valid on this input", cond)
    return taup, want


def end_to_end(psd, want, E64, taup):
    A = amplitude(E64)[:, None]
    f = _ratio(np.abs(np.sqrt(np.asarray(psd, np.float64)) - np.sqrt(want)), np.broadcast_to(taup * A, want.shape))
    assert f <= 1.0, ("end-to-end rule", f)
    return f
