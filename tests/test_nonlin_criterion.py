"""The bin-by-bin rule (tests/_rows_check.py) on the periodogram's non-linear pre-processing, on the CPU, no device involved.

1. Over every input of the GPU matrix (tests/_nonlin_cases.py): the float32 stand-in of tests/_nonlin_exact.py sits at a quarter
   of the case's bound 4 max(tau_f32, 2^-24) by construction -- the test guards the matrix (finite tau_f32, the two input
   conditions: limiter_condition() and, for the sub_mean = 2 cases, mean2_condition()) -- and below N = 8192 the oracle is
   within the suite's peak-normalised 1e-5 of the float64 rows: the float64 restatement and the oracle describe the same
   operation.  The matrix itself is checked too: every setting in every sample format and with mean removal, every route.
2. The rule rejects wrong rows.  Float64 stand-ins for a non-linear branch that has drifted, each built from the exact pipeline:
     window_first   the window applied before RA9MB instead of after it
     raw_ra9mb      one mid-frame sample that skips RA9MB
     raw_limiter    one mid-frame sample that skips the limiter
     scale_first    post_scale = sqrt(1 / (2 N)) applied before the limiter instead of after it
     ftmp           the limiter's temporary log|y| off by 2e-6 of its value (a float logarithm that is not the reference's
                    (float) log((double) |y|))
     a_off          `a` off by 3e-6 (at a = 0.3: N = 256 and 1024)
   tau_of(wrong, exact) > bound for each; under the limiter the last two are also ACCEPTED by the peak-normalised 1e-5 (ftmp at
   N = 1024 and 4096, a_off at N = 256 and 1024, a = 0.3) -- the limiter flattens a
   frame, its spectrum is broad, and 1e-5 of the largest bin is loose for every other one: that is the gap the rule closes.
"""
import numpy as np
import pytest

import _exact as X
import _nonlin_cases as N
import _nonlin_exact as NX
import _rows_cases as K
from _rows_check import FLOOR, bound, check_rows, check_spectrum, tau_of
from _signals import rel_err


@pytest.mark.parametrize("c", N.ALL_CASES, ids=N.case_id)
def test_stand_in_and_oracle_on_every_input_of_the_gpu_matrix(oracle, c):
    r = N.reference(oracle, c)
    assert np.isfinite(r.exact).all() and (r.exact >= 0).all()
    assert np.isfinite(r.tau_f32) and r.tau == bound(r.tau_f32) and r.tau >= 4 * FLOOR
    assert check_rows(r.f32, r.exact, r.tau, N.case_id(c)) <= 0.25 + 1e-12
    print("nonlin-criterion %-58s tau_f32 %.3e bound %.3e oracle tau %.3e (%.2f of the bound) oracle/float64 peak-normalised %.3e" % (
        N.case_id(c), r.tau_f32, r.tau, r.tau_oracle, r.tau_oracle / r.tau, r.e_ref))
    assert not (c.limiter and c.sub_mean == 2)
    assert N.limiter_condition(c, r.xf), N.case_id(c)
    if c in N.MEAN2_CASES:
        assert not c.limiter and c.sub_mean == 1 and K.mean2_condition(c, r.xf), N.case_id(c)
    assert np.isfinite(r.tau_oracle)
    if c.n < 8192:
        assert r.e_ref <= K.TOL, (N.case_id(c), r.e_ref)
    if not r.exact.any():
        assert not r.want.any() and not r.f32.any()


def test_limiter_condition_sees_a_sample_next_to_the_mean():
    c = N.nl(64, 0.0, "hanning", N.LIM, sub_mean=1)
    x = np.zeros(128, np.float32)
    x[:64] = np.tile(np.float32([0.5, -0.5]), 32)
    x[2:4] = 0.0
    assert N.limiter_condition(c, x)                                    # (hop 1: mean 0, two exact zeros; hop 2: silence)
    x[3] = np.float32(2.0 ** -25)                                       # lost in the float sum: mean 0, and 0 < |x - mean| < 8 * 2^-24 * 0.5
    assert not N.limiter_condition(c, x)
    assert N.limiter_condition(c._replace(sub_mean=0), x) and N.limiter_condition(c._replace(limiter=0, a=0.3), x)


def test_matrix_reaches_every_route_setting_and_format():
    assert {N.kernel_file(c) for c in N.ALL_CASES} == {"spectro_small.hip", "spectro16.hip", "spectro_big.hip"}
    assert {N.kernel_file(c, True) for c in N.SPECTRUM_CASES} == {"spectro_small.hip", "spectro16.hip", "spectro16w.hip"}
    assert {c.n for c in N.SIZE_CASES} == set(N.SIZES) and all(c.frames == K._frames_for(c.n) for c in N.SIZE_CASES)
    for s in ("limiter", "ra9mb", "both"):
        mine = [c for c in N.ALL_CASES if N.setting_of(c) == s]
        assert {c.n for c in mine} >= set(N.SIZES), s
        assert {c.fmt for c in mine} == {"f32", "s16", "u8"}, s
        assert {c.fmt for c in mine if c.sub_mean} == {"f32", "s16", "u8"}, s
    for group in (N.FORMAT_CASES, N.MEAN_CASES, N.HISTORY_CASES, [c for c, _ in N.RANGE_CASES], [c for c, _ in N.PITCH_CASES], N.SPECTRUM_CASES):
        assert {N.setting_of(c) for c in group} == {"limiter", "ra9mb", "both"}
        sizes = {c.n for c in group}
        assert min(sizes) < 256 and sizes & {256, 512, 1024, 4096}, sizes     # one small and one packed-range size at least
    assert {c.a for c in N.ALL_CASES} == {0.0, 0.001, 0.3}
    assert {c.window for c in N.ALL_CASES} >= {"hanning", "kaiser", "blackman", "rectangular"}
    assert {c.ovl for c in N.ALL_CASES} >= {0.0, 0.5, 0.75, 0.9, 0.33}
    assert {c.signal for c in N.ALL_CASES} >= {"weak", "noise", "synth", "bin", "impulse", "zero", "lsb1", "full", "tiny"}
    assert 32768 in {c.n for c in N.SPECTRUM_CASES}
    # spectro16w.hip's copy runs only for spectrum=True and under GLFER_FORM=w at N = 32768: W_CASES give it what the others get
    assert {N.kernel_file(c) for c in N.ALL_CASES if c.n == 32768} == {"spectro_big.hip"}
    assert {N.kernel_file(c, True) for c, _ in N.W_CASES} == {"spectro16w.hip"}
    for s in ("limiter", "ra9mb", "both"):
        mine = [(c, first) for c, first in N.W_CASES if N.setting_of(c) == s]
        assert {c.fmt for c, _ in mine} == {"f32", "s16", "u8"}, s
        assert any(c.sub_mean for c, _ in mine) and any(c.history_mode for c, _ in mine) and any(first for _, first in mine), s
    assert len(N.MEAN2_CASES) >= 4 and {N.kernel_file(c) for c in N.MEAN2_CASES} == {N.kernel_file(c) for c in N.ALL_CASES}


@pytest.mark.parametrize("c", N.SPECTRUM_CASES, ids=N.case_id)
def test_stand_in_spectra_on_every_input_of_the_gpu_matrix(oracle, c):
    raw, xf, exact_X, t32, tau = N.spectrum_reference(oracle, c)
    assert np.isfinite(t32) and tau >= 4 * FLOOR
    got = NX.spectrum32(xf, c.n, c.ovl, N.window(oracle, c), c.a, c.limiter, c.sub_mean, c.history_mode)
    assert check_spectrum(got, exact_X, c.n, tau) <= 0.25 + 1e-12
    assert np.allclose(np.abs(exact_X) ** 2 / c.n, N.reference(oracle, c).exact, rtol=1e-12, atol=0)
    print("nonlin-criterion spectrum %-58s tau_f32 %.3e bound %.3e" % (N.case_id(c), t32, tau))


# ---- the wrong rows --------------------------------------------------------------------------------------------------------
def _rows(y, n):
    return np.abs(np.fft.rfft(y, axis=1)) ** 2 / n


def _wrong_rows(c, xf, w):
    """name -> rows of a non-linear branch that differs from fft.c:127-156 in one thing; float64 throughout."""
    n = c.n
    fr = X.frames64(xf, n, c.ovl, c.sub_mean, c.history_mode)
    w64 = np.ones(n) if w is None else np.asarray(w, np.float64)
    a = float(np.float32(c.a))
    ra = (lambda v, aa=a: v / (aa + v * v)) if c.a > 0 else (lambda v: v)
    lim = NX.limiter64 if c.limiter else (lambda v: v)
    mid = n // 2 + 3
    out = {}
    if c.a > 0 and w is not None:
        out["window_first"] = _rows(lim(ra(fr * w64)), n)
    if c.a > 0:
        y = ra(fr)
        y[:, mid] = fr[:, mid]
        out["raw_ra9mb"] = _rows(lim(y * w64), n)
    if c.limiter:
        s = np.sqrt(1.0 / (2.0 * n))
        out["scale_first"] = _rows(lim(ra(fr) * w64 * s) / s, n)
        y = ra(fr) * w64
        z = lim(y)
        z[:, mid] = y[:, mid]
        out["raw_limiter"] = _rows(z, n)
        nz = y != 0
        mag = np.zeros_like(y)
        mag[nz] = np.exp(0.1 * (np.log(np.abs(y[nz])) * (1.0 + 2e-6)))
        out["ftmp"] = _rows(np.where(y > 0, mag, -mag), n)
    if c.a > 0:
        out["a_off"] = _rows(lim(ra(fr, a + 3e-6) * w64), n)
    return out


GAP = ("ftmp", "a_off")                 # under the limiter: accepted by the peak-normalised 1e-5, rejected by rule (1)
WRONG_CASES = [N.nl(256, 0.5, "hanning", N.RA_L, "synth", frames=9), N.nl(256, 0.5, "hanning", N.BOTH_L, "synth", frames=9), N.nl(1024, 0.5, "hanning", N.LIM, "weak", frames=9),
               N.nl(4096, 0.5, "hanning", N.LIM, "weak", frames=7), N.nl(1024, 0.75, "kaiser", N.BOTH_L, "synth", frames=9),
               N.nl(64, 0.5, "blackman", N.RA_S, "noise", frames=21)]


@pytest.mark.parametrize("c", WRONG_CASES, ids=N.case_id)
def test_rule_rejects_a_drifted_nonlinear_branch(oracle, c):
    r = N.reference(oracle, c)
    assert check_rows(r.exact, r.exact, r.tau) == 0.0
    wrong = _wrong_rows(c, r.xf, N.window(oracle, c))
    assert set(wrong) == ({"window_first", "raw_ra9mb", "a_off"} if c.a > 0 else set()) | ({"raw_limiter", "scale_first", "ftmp"} if c.limiter else set())
    for name, rows in wrong.items():
        old = max(max(rel_err(rows[f], r.exact[f])) for f in range(c.frames))
        new = tau_of(rows, r.exact) / r.tau
        print("nonlin-mutant %-52s %-12s peak-normalised %.2e (%s by 1e-5), rule (1) %.1f of the bound" % (
            N.case_id(c), name, old, "accepted" if old < K.TOL else "seen", new))
        with pytest.raises(AssertionError):
            check_rows(rows, r.exact, r.tau)
        assert new > 1.0, (name, new)
        if name in GAP and c.limiter:
            assert old < K.TOL, (name, c.n, old)                       # the gap: the suite's norm lets it through
