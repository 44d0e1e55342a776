"""The bin-by-bin acceptance rule (tests/_rows_check.py) on two-sided rows of complex I/Q input, tested on the CPU.

tests/test_gpu_iq.py holds the device's rows to  |sqrt(got[k]) - sqrt(exact[k])| <= tau sqrt(sum_k exact[k])  in every one of the N
bins, tau = bound(tau_f32), exact = the float64 rows of tests/_iq_exact.py and tau_f32 what its float32 stand-in reaches.  Here, without
a device: the rule accepts the stand-in on every input of the GPU matrix (true by construction at a quarter of the bound: the test
guards the matrix -- finite, positive bounds, silence that is silence), and on the 'crit' signal (unequal I and Q powers, a DC
level on Q only, a carrier on a positive bin and a tone 80 dB below it on a different negative bin) it rejects the rows a wrong
kernel would write:
  mirrored     bin k holds bin N - k (the spectrum of the conjugate)
  I alone      Q taken as zero
  swapped      I and Q exchanged
  shifted      every bin one column off
  taper lost   the last taper left out of the sum (multitaper cases)
  weak zeroed  the bins of the weak tone zeroed
Each of them is also asserted to differ from the right rows, so that a rejection is never vacuous.
"""
import numpy as np
import pytest

import _iq_cases as Q
from _rows_check import FLOOR, bound, check_rows, tau_of


@pytest.mark.parametrize("c", Q.CASES + Q.CRITERION_CASES, ids=Q.case_id)
def test_stand_in_on_every_input_of_the_gpu_matrix(oracle, c):
    r = Q.reference(oracle, c)
    assert np.isfinite(r.exact).all() and (r.exact >= 0).all()
    assert np.isfinite(r.tau_f32) and r.tau == bound(r.tau_f32) and r.tau >= 4 * FLOOR
    assert check_rows(r.f32, r.exact, r.tau, Q.case_id(c)) <= 0.25 + 1e-12
    print("iq-criterion %-52s tau_f32 %.3e bound %.3e" % (Q.case_id(c), r.tau_f32, r.tau))
    if c.signal == "zero":
        assert not r.exact.any() and not r.f32.any() and not r.z.any()
    else:
        assert r.exact.sum(axis=1).min() > 0


def test_inputs_tell_the_two_sides_apart(oracle):
    """The signals the orientation of a row hangs on: I and Q of unequal power, DC on Q only, the tones on the bins they claim."""
    for c in Q.CRITERION_CASES:
        r = Q.reference(oracle, c)
        assert r.z.real.std() != r.z.imag.std()
        kc, kw = Q.tone_bins(c.n)
        row = r.exact[-1]
        assert abs(int(np.argmax(row)) - kc) <= 1 + c.nw                        # (tapers spread a tone over 2 NW bins)
        weak = int(round(kw)) % c.n
        assert weak > c.n // 2
        if c.est == "fft":                                                       # (five tapers' leakage of the carrier covers a short row)
            assert row[weak] > 1e3 * row[(c.n - weak) % c.n]                      # the weak tone sits on the negative side alone
    n = Q.fft(1024, 0.5, "hanning", 5, "noise")
    z = Q.reference(oracle, n).z
    assert z.imag.mean() > 10 * abs(z.real.mean()) and z.real.std() > 2 * z.imag.std()


def _wrong_rows(oracle, c, r):
    n = c.n
    k = np.arange(n)
    out = {}
    out["mirrored"] = r.f32[:, (n - k) % n]
    out["I alone"] = Q.rows_of(oracle, c, (r.z.real + 0j).astype(np.complex64))[1]
    out["swapped"] = Q.rows_of(oracle, c, (r.z.imag + 1j * r.z.real).astype(np.complex64))[1]
    out["shifted"] = np.roll(r.f32, 1, axis=1)
    if c.est == "mtm":
        out["taper lost"] = Q.rows_of(oracle, c, r.z, ntap=c.kmax)[1]
    kw = Q.tone_bins(n)[1] % n
    spread = max(3, int(np.ceil(c.nw)) + 1)
    m = r.f32.copy()
    m[:, np.abs(k - kw) <= spread] = 0.0
    out["weak zeroed"] = m
    return out


@pytest.mark.parametrize("c", Q.CRITERION_CASES, ids=Q.case_id)
def test_rule_rejects_wrong_two_sided_rows(oracle, c):
    r = Q.reference(oracle, c)
    assert check_rows(r.exact, r.exact, r.tau) == 0.0
    assert check_rows(r.f32, r.exact, r.tau) <= 0.25 + 1e-12
    wrong = _wrong_rows(oracle, c, r)
    assert set(wrong) == {"mirrored", "I alone", "swapped", "shifted", "weak zeroed"} | ({"taper lost"} if c.est == "mtm" else set())
    for name, rows in wrong.items():
        assert rows.shape == r.exact.shape and (rows != r.f32).any(), name
        frac = tau_of(rows, r.exact) / r.tau
        print("iq-mutant %-44s %-12s %.1f of the bound" % (Q.case_id(c), name, frac))
        assert frac > 1.0, name
        with pytest.raises(AssertionError):
            check_rows(rows, r.exact, r.tau, name)
