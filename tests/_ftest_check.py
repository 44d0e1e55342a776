"""The acceptance rule for harmonic F-test rows (tests only): the rule test_ftest_vs_oracle has held since round 2,
as one function, so that every F-test case of the suite is judged by the same assertions.

F = num / den with num = kmax |mu|^2 sum(U0^2) and den = sum_j |y_j - mu U0_j|^2 (mtm.c:165-233), two spectrum-like
sums that each carry the PSD tolerance (max-normalised TOL), so per frame and bin below Nyquist

    |got - want| * den <= TOL * (max num + want * max den)                          (1)

with num and den in float64 (tests/_exact.py::ftest64): they weigh the bound, they are not what is compared.  Beside
it, per frame, the median of |got / want - 1| below 1e-4 (2) and the strongest bin of got and want the same (3).  At
Nyquist the reference never accumulates the denominator (mtm.c:206 stops below n/2): x / 0, non-finite in both (4).
No other bin is left out.  tests/test_ftest_criterion.py holds the rule itself to what it must accept and reject."""
import numpy as np

TOL = 1e-5              # the project's parity target
MEDIAN_TOL = 1e-4


def check_ftest(got, want, num, den, kmax, tol=TOL):
    """got, want: [frames][n/2+1] F rows (float32 or float64); num, den: the same shape in float64 (ftest64).
    Asserts (1)-(4) and returns the largest fraction of bound (1) used by any frame and bin."""
    got = np.asarray(got)
    want = np.asarray(want)
    assert got.ndim == 2 and got.shape == want.shape == np.shape(num) == np.shape(den), (got.shape, want.shape, np.shape(num), np.shape(den))
    frames, half = got.shape[0], got.shape[1] - 1
    assert frames > 0 and half >= 2
    assert np.all(~np.isfinite(got[:, half])), "kmax %d: a finite value in the Nyquist column of got" % kmax
    assert np.all(~np.isfinite(want[:, half])), "kmax %d: a finite value in the Nyquist column of want" % kmax
    g64 = got[:, :half].astype(np.float64)
    w64 = want[:, :half].astype(np.float64)
    num = np.asarray(num, np.float64)[:, :half]
    den = np.asarray(den, np.float64)[:, :half]
    dist = np.abs(g64 - w64) * den
    bound = tol * (num.max(axis=1, keepdims=True) + w64 * den.max(axis=1, keepdims=True))
    bad = np.argwhere(~(dist <= bound))                      # (a NaN or an infinity below Nyquist fails here)
    with np.errstate(divide="ignore", invalid="ignore"):
        used = dist / bound
    assert bad.size == 0, ("kmax %d: bound exceeded at %d (frame, bin), worst %.3g of it" % (kmax, len(bad), np.nanmax(used)), bad[:8].tolist())
    with np.errstate(divide="ignore", invalid="ignore"):
        med = np.median(np.abs(g64 / w64 - 1.0), axis=1)
    assert np.all(med < MEDIAN_TOL), ("kmax %d: median |got/want - 1| per frame" % kmax, float(np.max(med)), np.argwhere(~(med < MEDIAN_TOL))[:8].ravel().tolist())
    ag, aw = np.argmax(g64[:, 1:], axis=1), np.argmax(w64[:, 1:], axis=1)
    assert np.array_equal(ag, aw), ("kmax %d: strongest bin differs in frames" % kmax, np.argwhere(ag != aw)[:8].ravel().tolist())
    return float(used.max())
