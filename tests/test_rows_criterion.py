"""The bin-by-bin acceptance rule (tests/_rows_check.py) tested on the CPU, no device involved.

1. What it must accept: the float32 stand-in (tests/_exact.py: float32 frame x float32 table, torch.fft.rfft in float32,
   float32 sums) on EVERY input of the GPU matrix (tests/_rows_cases.py) at the case's bound 4 max(tau_f32, 2^-24) -- true
   by construction at a quarter of the bound; the test guards the matrix (finite, positive bounds) and prints tau_f32 and
   the oracle's own tau.  And the oracle against float64 arithmetic under
   the suite's peak-normalised 1e-5 below N = 8192 (from there on round 4's rule, max(1e-5, 1.1 x err(oracle, exact)),
   is what the GPU module holds the device to): an input the reference alone cannot pass fails here, without a GPU.
2. What it must reject: float64 stand-ins for subtly wrong kernels (five tapers, NW = 2.5).  weakzero, nyquist, mirror and
   twiddle at N = 64, 1024, 4096, 16384 on 'weak' and on 'noise'; weight at those sizes on 'noise' and at N = 1024, 4096,
   16384 on 'weak'; floor at N = 4096 and 16384 on 'weak' -- the (mutant, input) pairs left out change no value (below), and
   the test asserts that they are these pairs and no others:
     floor    bins below 1e-6 of the row maximum scaled by 1.5
     weakzero the weak tone's bins zeroed
     weight   the last taper's 1 / (1 + sig_j) weight dropped in bins k % 9 == 4 away from the tones
     nyquist  Nyquist doubled
     mirror   bin k taking bin N/2 - k's value for k % 16 == 5 (a wrong mirror index)
     twiddle  the last pass's twiddle rotated by 1e-4 rad on one residue class of bins (k % 4)
   The first three are also asserted to be ACCEPTED by the peak-normalised 1e-5 on 'weak' at N = 4096 and 16384 -- that
   is the gap the rule closes -- and for every other one the module prints which norm sees it.  (At N = 64 and 1024 the
   leakage of the strong tone through five tapers keeps every bin within 50 dB of the maximum: 'floor' and 'weight' then
   touch no bin of a 'weak' row, and zeroing the weak tone's bins removes leakage the old norm sees.)  A mutation that
   changes no value of an input (also: no bin of a noise row lies 60 dB below its maximum) is printed as such, not counted.
A later edit that loosens the rule until one of these passes fails this module.
"""
import numpy as np
import pytest

import _exact as X
import _rows_cases as K
from _rows_check import FLOOR, bound, check_rows, check_spectrum, tau_of
from _signals import rel_err


@pytest.mark.parametrize("c", K.ALL_CASES, ids=K.case_id)
def test_stand_in_and_oracle_on_every_input_of_the_gpu_matrix(oracle, c):
    r = K.reference(oracle, c)
    assert np.isfinite(r.exact).all() and (r.exact >= 0).all()
    assert np.isfinite(r.tau_f32) and r.tau == bound(r.tau_f32) and r.tau >= 4 * FLOOR
    frac = check_rows(r.f32, r.exact, r.tau, K.case_id(c))
    assert frac <= 0.25 + 1e-12
    print("rows-criterion %-60s tau_f32 %.3e bound %.3e oracle tau %.3e (%.2f of the bound) oracle/float64 peak-normalised %.3e" % (
        K.case_id(c), r.tau_f32, r.tau, r.tau_oracle, r.tau_oracle / r.tau, r.e_ref))
    assert np.isfinite(r.tau_oracle)
    if c.n < 8192:
        assert r.e_ref <= K.TOL, (K.case_id(c), r.e_ref)
    if not r.exact.any():
        assert not r.want.any() and not r.f32.any()


def test_inputs_of_the_in_kernel_mean_cases_meet_the_headers_condition(oracle):
    assert len(K.MEAN2_CASES) >= 8 and {c.est for c in K.MEAN2_CASES} == {"fft", "mtm"}
    for c in K.MEAN2_CASES:
        assert c.sub_mean == 1 and K.mean2_condition(c, K.reference(oracle, c).xf), K.case_id(c)


@pytest.mark.parametrize("c", K.SPECTRUM_CASES, ids=K.case_id)
def test_stand_in_spectra_on_every_input_of_the_gpu_matrix(oracle, c):
    raw, xf, exact_X, t32, tau = K.spectrum_reference(oracle, c)
    assert np.isfinite(t32) and tau >= 4 * FLOOR
    assert check_spectrum(X.spectrum32(xf, c.n, c.ovl, K.window(oracle, c.n, c.window)), exact_X, c.n, tau) <= 0.25 + 1e-12
    # the two rules are one: |X|^2 / n of the exact spectra are the exact rows
    assert np.allclose(np.abs(exact_X) ** 2 / c.n, K.reference(oracle, c).exact, rtol=1e-12, atol=0)
    print("rows-criterion spectrum %-60s tau_f32 %.3e bound %.3e" % (K.case_id(c), t32, tau))


# ---- the mutants ---------------------------------------------------------------------------------------------------------
def _eigen(xf, c, v):
    """The tapered spectra: complex [tapers][frames][n/2+1]."""
    fr = X.frames64(xf, c.n, c.ovl)
    return np.stack([np.fft.rfft(fr * v[j], axis=1) for j in range(len(v))])


def _twiddle_rotated(xf, c, v, sig, cls):
    """The last radix-2 pass X[k] = E[k] + W^k O[k] with W^k turned by 1e-4 rad for k % 4 == cls."""
    n = c.n
    fr = X.frames64(xf, c.n, c.ovl)
    k = np.arange(n // 2 + 1)
    tw = np.exp(-2j * np.pi * k / n) * np.where(k % 4 == cls, np.exp(1e-4j), 1.0)
    out = np.zeros((fr.shape[0], n // 2 + 1))
    for j in range(len(sig)):
        y = fr * v[j]
        E, O = np.fft.fft(y[:, 0::2], axis=1), np.fft.fft(y[:, 1::2], axis=1)
        idx = k % (n // 2)
        out += np.abs(E[:, idx] + tw * O[:, idx]) ** 2 / n / (1.0 + sig[j])
    return out


def _mutants(xf, c, exact, v, sig):
    n, half = c.n, c.n // 2
    k = np.arange(half + 1)
    k0, k1 = 0.23 * n + 0.37, 0.37 * n + 0.21                        # the tones of 'weak'
    spread = max(3, int(np.ceil(c.nw)) + 1)
    out = {}
    m = exact.copy()
    low = m < 1e-6 * m.max(axis=1, keepdims=True)
    m[low] *= 1.5
    out["floor"] = m
    m = exact.copy()
    m[:, np.abs(k - k1) <= spread] = 0.0
    out["weakzero"] = m
    eig = np.abs(_eigen(xf, c, v)) ** 2 / n
    assert np.allclose((eig / (1.0 + sig)[:, None, None]).sum(axis=0), exact, rtol=1e-11, atol=0)
    # the last taper's weight 1 / (1 + sig_j) left out (the one furthest from 1); on 'weak' in the bins 50 dB and more below
    # the row's maximum, which is where "away from the tones" is for five tapers' leakage
    j = len(sig) - 1
    away = np.broadcast_to(k % 9 == 4, exact.shape)
    if c.signal == "weak":
        away = away & (exact < 1e-5 * exact.max(axis=1, keepdims=True))
    m = exact.copy()
    m[away] += (eig[j] * (1.0 - 1.0 / (1.0 + sig[j])))[away]
    out["weight"] = m
    m = exact.copy()
    m[:, half] *= 2.0
    out["nyquist"] = m
    m = exact.copy()
    sel = k[(k % 16 == 5) & (k < half)]
    m[:, sel] = exact[:, half - sel]
    out["mirror"] = m
    out["twiddle"] = _twiddle_rotated(xf, c, v, sig, int(round(k0)) % 4)
    return out


GAP = ("floor", "weakzero", "weight")


@pytest.mark.parametrize("signal", ["weak", "noise"])
@pytest.mark.parametrize("n,frames", [(64, 21), (1024, 9), (4096, 7), (16384, 3)])
def test_rule_rejects_subtly_wrong_rows(oracle, n, frames, signal):
    c = K.mtm(n, 0.5, 2.5, 4, frames, signal)
    r = K.reference(oracle, c)
    v, sig = K.tapers(oracle, n, 4, 2.5)
    assert check_rows(r.exact, r.exact, r.tau) == 0.0
    assert check_rows(r.f32, r.exact, r.tau) <= 0.25 + 1e-12
    assert np.allclose(_twiddle_rotated(r.xf, c, v, sig, -1), r.exact, rtol=1e-10, atol=1e-30)     # (no class turned: the rows themselves)
    for name, rows in _mutants(r.xf, c, r.exact, v, sig).items():
        changed = int((rows != r.exact).sum())
        old = max(max(rel_err(rows[f], r.exact[f])) for f in range(frames))
        new = tau_of(rows, r.exact) / r.tau
        print("rows-mutant N=%-5d %-5s %-8s %6d values changed: peak-normalised %.2e (%s by 1e-5), rule (1) %.1f of the bound" % (
            n, signal, name, changed, old, "accepted" if old < K.TOL else "seen", new))
        if not changed:
            # five tapers' leakage of the strong tone keeps every bin of a short row within 50 dB of its maximum, and no bin of
            # a noise row lies 60 dB below it
            assert (name == "floor" and (signal == "noise" or n <= 1024)) or (name == "weight" and signal == "weak" and n == 64), name
            continue
        with pytest.raises(AssertionError):
            check_rows(rows, r.exact, r.tau)
        assert new > 1.0
        if signal == "weak" and name in GAP and n >= 4096:
            assert old < K.TOL, (n, name, old)                  # the gap: today's norm lets it through


def test_rule_rejects_what_is_no_power_row(oracle):
    c = K.fft(1024, 0.5, "hanning", 5, "noise")
    r = K.reference(oracle, c)
    for spoil in ("nan", "inf", "negative"):
        rows = r.exact.copy()
        rows[3, 17] = {"nan": np.nan, "inf": np.inf, "negative": -1e-12}[spoil]
        with pytest.raises(AssertionError):
            check_rows(rows, r.exact, r.tau)
        assert tau_of(rows, r.exact) == np.inf
    silent = np.zeros_like(r.exact)
    assert check_rows(silent, silent, r.tau) == 0.0
    silent[2, 5] = 1e-30
    with pytest.raises(AssertionError):
        check_rows(silent, np.zeros_like(r.exact), r.tau)
    # the complex rule sees a phase error the power rule cannot
    raw, xf, exact_X, t32, tau = K.spectrum_reference(oracle, c)
    turned = exact_X * np.exp(1e-4j)
    assert check_rows(np.abs(turned) ** 2 / c.n, r.exact, r.tau) < 1e-3
    with pytest.raises(AssertionError):
        check_spectrum(turned, exact_X, c.n, tau)
