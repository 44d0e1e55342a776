"""The F-test acceptance rule (tests/_ftest_check.py) tested on the CPU, no device involved.

1. What it must accept: float64 arithmetic (num / den of tests/_exact.py::ftest64) against the oracle, on EVERY input
   of the GPU matrix (tests/_ftest_cases.py) -- the oracle's own float32 transforms use 0.002 - 0.06 of the bound up
   to N = 4096 and on tonal input, 0.25 - 0.55 on plain noise at N = 8192 / 16384, where its recurrence twiddles
   (fft_radix2.c:127-141) are the error.  An input the reference alone cannot pass fails here, without a GPU.
2. What it must reject: two float64 stand-ins for a subtly wrong kernel -- one taper's residual dropped in one bin of
   nine (a register of the paired form that misses its last sequence), and one bin in sixteen taking its neighbour's
   residual for one taper (a wrong mirror index) -- at small, middle and large block sizes, on tones and on noise.
A later edit that loosens the rule until one of these passes fails this module.
"""
import numpy as np
import pytest

import _ftest_cases as K
from _exact import frames64
from _ftest_check import check_ftest


def _float64_rows(num, den):
    got = num / den
    got[:, -1] = np.inf                  # the reference never accumulates the Nyquist denominator: x / 0
    return got


@pytest.mark.parametrize("c", list(dict.fromkeys(K.ALL_CASES)), ids=K.case_id)
def test_oracle_passes_the_rule_on_every_input_of_the_gpu_matrix(oracle, c):
    _, _, want, num, den = K.reference(oracle, c)
    frac = check_ftest(_float64_rows(num, den), want, num, den, c.kmax)
    print("oracle against float64, %s: %.4f of the bound" % (K.case_id(c), frac))
    assert frac <= 1.0


def _residuals(xf, c, tapers):
    """|y_j - mu U0_j|^2 per taper: [kmax+1][frames][n/2+1] float64 (the terms of ftest64's den)."""
    fr = frames64(xf, c.n, c.ovl, 1 if c.sub_mean else 0, c.history_mode)
    v = np.asarray(tapers, np.float64)
    U0 = v.sum(axis=1)
    hn = (U0[:, None] * v).sum(axis=0) / (U0 * U0).sum()
    mu = np.fft.rfft(fr * hn, axis=1)
    return np.stack([np.abs(np.fft.rfft(fr * v[j], axis=1) - mu * U0[j]) ** 2 for j in range(c.kmax + 1)])


@pytest.mark.parametrize("signal", ["synth", "noise"])
@pytest.mark.parametrize("n,nw,kmax,frames", [(64, 2.5, 4, 21), (1024, 2.5, 4, 9), (2048, 4.0, 7, 7), (16384, 4.5, 8, 3)])
def test_rule_rejects_subtly_wrong_rows(oracle, n, nw, kmax, frames, signal):
    c = K.case(n, 0.5, nw, kmax, frames, signal)
    _, xf, want, num, den = K.reference(oracle, c)
    assert check_ftest(_float64_rows(num, den), want, num, den, kmax) <= 1.0
    res = _residuals(xf, c, K._tapers(oracle, n, kmax, nw))
    assert np.allclose(res.sum(axis=0), den, rtol=1e-12)
    bins = np.arange(n // 2 + 1)
    # one taper's residual dropped in one bin of nine
    dropped = den.copy()
    sel = bins % 9 == 4
    dropped[:, sel] -= res[1][:, sel]
    with pytest.raises(AssertionError):
        check_ftest(_float64_rows(num, dropped), want, num, den, kmax)
    # one bin in sixteen takes its neighbour's residual for one taper
    swapped = den.copy()
    sel = np.flatnonzero((bins % 16 == 5) & (bins + 1 < n // 2))
    swapped[:, sel] += res[0][:, sel + 1] - res[0][:, sel]
    with pytest.raises(AssertionError):
        check_ftest(_float64_rows(num, swapped), want, num, den, kmax)
    # and the rule's parts one by one: a finite Nyquist value, a NaN below Nyquist, a moved strongest bin
    good = _float64_rows(num, den)
    for spoil in ("nyquist", "nan", "argmax"):
        rows = good.copy()
        if spoil == "nyquist":
            rows[0, -1] = 1.0
        elif spoil == "nan":
            rows[frames - 1, 3] = np.nan
        else:
            k = 1 + int(np.argmax(rows[0, 1:n // 2]))
            other = k + 2 if k + 2 < n // 2 else k - 2
            rows[0, other] = rows[0, k] * (1.0 + 1e-6)      # another bin is now the strongest
        with pytest.raises(AssertionError):
            check_ftest(rows, want, num, den, kmax)
