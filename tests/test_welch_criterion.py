"""The Welch rows' criterion without a GPU: tests/_cross_check.py's rule with tau = 4 max(tau_f32, 2^-24) from the float32
stand-in (tests/_welch_exact.py welch32), on inputs of tests/test_gpu_welch.py.  The rule rejects wrong rows that are close to
right ones -- a segment missing, segments one frame late, the wrong step, the mean of per-segment coherences, magnitudes averaged
with the phase dropped, the conjugate on the wrong channel, the 1/L on Sxy alone -- and accepts float64 rounded once to float32 and
the opposite segment order.  The float64 premise of the device's line10 assertion is checked here."""
import numpy as np
import pytest

import _cross_check as K
import _cross_exact as E
import _welch_exact as W

# the GPU module's cases with at least three rows on inputs whose two channels differ in phase, and line10
CASES = [c for c in W.cases() if c.name in ("noise", "line", "delay3") and c.fmt == "f32" and c.hist == 0 and c.n <= 1024 and c.rows >= 3
         and c.segments <= 8] + [W.line10_case(1024)]


def _ref(lib, c):
    p64, p32 = W.case_per_frame(lib, c)
    ref = W.welch64(p64, c.segments, c.step)
    return p64, p32, ref, K.tau_of(W.welch32(p32, c.segments, c.step), ref)


def _head(x, rows):
    return E.Cross(*(a[:rows] for a in x))


def test_the_cases_are_there():
    assert len(CASES) >= 6 and any(c.kind[0] == "mtm" for c in CASES) and any(c.kind[0] == "fft" for c in CASES)
    assert {c.step == c.segments for c in CASES} == {True, False}


@pytest.mark.parametrize("c", CASES, ids=W.case_id)
def test_accepts_float32_roundings(lib, c):
    p64, p32, ref, tau = _ref(lib, c)
    assert ref.sxx.shape == (c.rows, c.n // 2 + 1)
    assert K.FLOOR * K.MARGIN <= tau < 1e-5, tau
    K.check(ref, ref, tau, "float64 itself")
    once = E.Cross(ref.sxx.astype(np.float32), ref.syy.astype(np.float32), ref.sxy.astype(np.complex64), ref.coh.astype(np.float32))
    K.check(once, ref, tau, "float64 rounded once to float32")
    K.check(W.welch32(p32, c.segments, c.step, reverse=True), ref, tau, "the opposite segment order")
    # held-out draws: the stand-in of another seed's stream passes the tau of this one
    p64b, p32b = W.case_per_frame(lib, c, seed=1)
    K.check(W.welch32(p32b, c.segments, c.step), W.welch64(p64b, c.segments, c.step), tau, "held-out draw")


def _mutations(c, p64, ref):
    L, step, rows = c.segments, c.step, c.rows
    out = {}
    # a row with one segment missing (the last one), still divided by L; and divided by L - 1
    short = [o for o in W._rows(p64, L - 1, step, 0, rows, (np.float64, np.complex128), range)] if L > 1 else None
    if short is not None:
        sxx, syy, sxy = (o / L for o in short)
        out["one segment missing"] = (E.Cross(sxx, syy, sxy, E._coh(sxx, syy, sxy)), ref)
        sxx, syy, sxy = (o / (L - 1) for o in short)
        out["one segment missing, mean of the rest"] = (E.Cross(sxx, syy, sxy, E._coh(sxx, syy, sxy)), ref)
    out["segments one frame late"] = (W.welch64(p64, L, step, first=1, nrows=rows - 1), _head(ref, rows - 1))
    fit = W.rows_of(p64.sxx.shape[0], L, step + 1)
    assert fit >= 2
    out["rows taken at step + 1"] = (W.welch64(p64, L, step + 1, nrows=fit), _head(ref, fit))
    if L > 1:
        coh_mean = np.zeros_like(ref.coh)
        for r in range(rows):
            coh_mean[r] = p64.coh[r * step:r * step + L].mean(axis=0)
        out["mean of per-segment coherences"] = (ref._replace(coh=coh_mean), ref)
        mag = W._rows(E.Cross(p64.sxx, p64.syy, np.abs(p64.sxy) + 0j, None), L, step, 0, rows, (np.float64, np.complex128), range)[2] / L
        out["sxy averaged by magnitude"] = (ref._replace(sxy=mag, coh=E._coh(ref.sxx, ref.syy, mag)), ref)
        out["1/L on sxy alone"] = (E.Cross(ref.sxx * L, ref.syy * L, ref.sxy, E._coh(ref.sxx * L, ref.syy * L, ref.sxy)), ref)
    out["conj on the wrong channel"] = (ref._replace(sxy=np.conj(ref.sxy)), ref)
    return out


@pytest.mark.parametrize("c", CASES, ids=W.case_id)
def test_mutations_are_rejected(lib, c):
    p64, _, ref, tau = _ref(lib, c)
    muts = _mutations(c, p64, ref)
    assert len(muts) >= 3
    for what, (got, want) in muts.items():
        f = K.fraction(got, want, tau)
        print("welch mutation %-40s %s fraction of the bound %10.3g" % (what, W.case_id(c), f))
        assert f > 1.0, (what, W.case_id(c), f)


def test_float64_products_vanish_for_silence_only(lib):
    """The rule asks for coh == 0 exactly where the float64 Sxx Syy is 0, which a device can owe only where a channel is silent.
    So no accuracy case may have a float64 row with a zero product for any other reason (an exact cancellation in float64, as
    tones on odd bins under a rectangular window give it): in every case but the three that hold silent stretches, all are > 0."""
    for c in W.cases():
        if c.name in ("silence", "x_only", "impulses"):
            continue
        tapers, sig = W.tables_of(lib, c.n, c.kind)
        p64 = E.cross64(W.case_input(c)[1], c.n, c.ovl, tapers, sig, c.hist)
        ref = W.welch64(p64, c.segments, c.step)
        assert (ref.sxx * ref.syy > 0).all(), W.case_id(c)


def test_mean_of_per_segment_coherences_is_one_for_fft_plans(lib):
    """Why FFT plans need the average: one window's single-frame coherence is 1 wherever both spectra are not zero."""
    c = W.line10_case(1024)
    p64, _ = W.case_per_frame(lib, c)
    assert np.abs(p64.coh - 1.0).max() < 1e-9


@pytest.mark.parametrize("n", [1024, 8192])
def test_line_premise_in_float64(lib, n):
    """line10 (a common line 10 dB under each channel's noise; Hanning, 50 % overlap, L = step = 16, three rows): in float64 the
    line's bin has coherence >= 0.8 in every row and every bin more than two away has coherence <= 0.6, so the device's largest
    coherence of a row can be asked to sit at the line (tests/test_gpu_welch.py).  N = 256 is left out: 0.70 against 0.39 there."""
    c = W.line10_case(n)
    p64, _ = W.case_per_frame(lib, c)
    ref = W.welch64(p64, c.segments, c.step)
    kl = E.line_bin(n)
    assert ref.coh.shape == (3, n // 2 + 1)
    far = np.abs(np.arange(n // 2 + 1) - kl) > 2
    print("line10 n=%d coh at the line %s, largest elsewhere %s" % (n, ref.coh[:, kl], ref.coh[:, far].max(axis=1)))
    assert (ref.coh[:, kl] >= 0.8).all(), ref.coh[:, kl]
    assert (ref.coh[:, far] <= 0.6).all(), ref.coh[:, far].max()
