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


# ---- inputs keyed to the grid's passes: the GPU module's two-pass cases (the longest stream, N = 256 at step 5, left to the GPU)
PASS_CASES = [c for c in W.pass_cases() if c.name in E.PASS_INPUTS and not (c.n == 256 and c.step == 5)]


def pass_case_bits(c, xy32):
    """(per-row silence bits, the rows silent in x) of a case's stream."""
    bits = W.row_bits(E.silence_bits(xy32, c.n, c.ovl, c.hist), c.segments, c.step, c.rows)
    return bits, np.flatnonzero((bits & 1) == 0)


def test_the_pass_cases_cover_their_grid():
    import _grid_passes as G
    cs = W.pass_cases()
    assert {(c.n, c.kind, c.segments, c.step) for c in cs} == {(n,) + pl for n in W.PASS_SIZES for pl in W.PASS_PLANS}
    for n in W.PASS_SIZES:
        assert {c.name for c in cs if c.n == n} == set(W.PASS_NAMES)
    for pl in W.PASS_PLANS:
        assert {c.name for c in cs if (c.kind, c.segments, c.step) == pl} == set(W.PASS_NAMES)
    assert {c.fmt for c in cs} == set(W.FMTS) and {c.hist for c in cs} == {0, 1}
    assert all(G.passes("spectro16cx", c.n, c.rows).npasses == 2 for c in cs)


@pytest.mark.parametrize("c", PASS_CASES, ids=W.case_id)
def test_row_bits_of_the_row_one_pass_earlier_are_rejected(lib, c):
    """The float32 stand-ins pass the rule on the pass-keyed inputs and keep the exact zeros; a stand-in that stores a row by the
    silence bits of the row one grid pass earlier does not (tests/test_cross_criterion.py's test of the per-frame entry, with
    the OR over a row's segments).  x_late and x_early put a row into pass 1 that holds x in ONE of its segments: a stand-in that
    takes a row's bits from its last segment alone, or its first alone, zeroes or keeps the wrong rows there."""
    import _grid_passes as G
    p = G.passes("spectro16cx", c.n, c.rows)
    raw, xy32 = W.case_input(c)
    p64, p32 = W.case_per_frame(lib, c)
    ref = W.welch64(p64, c.segments, c.step)
    tau = K.tau_of(W.welch32(p32, c.segments, c.step), ref)
    assert K.FLOOR * K.MARGIN <= tau < 1e-5, tau
    tapers, sig = W.tables_of(lib, c.n, c.kind)
    fbits = E.silence_bits(xy32, c.n, c.ovl, c.hist)
    packed = E.cross32_packed(xy32, c.n, c.ovl, tapers, sig, c.hist, bits=np.full(len(fbits), 3))
    bits, quiet = pass_case_bits(c, xy32)
    honest = W.welch32_packed(packed, c.segments, c.step, bits)
    K.check(honest, ref, tau, W.case_id(c) + " packed stand-in")
    from test_cross_criterion import exact_zeros_hold
    assert exact_zeros_hold(honest, quiet) and exact_zeros_hold(ref, quiet)
    if c.name == "apart_by_pass":
        assert (bits == 3).all()
        moved = E.Cross(*(E.one_pass_earlier(a, p.stride) for a in honest))        # the samples of the row one pass earlier
        assert K.fraction(moved, ref, tau) > 100.0
        return
    assert len(quiet) >= p.fpb and len(set(p.pass_of[quiet])) == 1
    # the row of pass 1 that holds x in one segment only: its bits need the OR, taken in a later pass
    first = p.stride
    segs = [int(fbits[first * c.step + s] & 1) for s in range(c.segments)]
    assert sum(segs) == 1 and segs[0 if c.name == "x_late" else -1] == 1 and bits[first] == 3, segs
    stale = W.welch32_packed(packed, c.segments, c.step, E.one_pass_earlier(bits, p.stride))
    f = K.fraction(stale, ref, tau)
    print("stale row bits %s fraction of the bound %.3g, exact zeros %s" % (W.case_id(c), f, exact_zeros_hold(stale, quiet)))
    assert f > 1.0, f
    assert not exact_zeros_hold(stale, quiet) if c.name == "x_late" else (stale.sxx[first:] == 0).all()
    one_segment = fbits[(c.segments - 1 if c.name == "x_late" else 0):][:(c.rows - 1) * c.step + 1:c.step]
    assert K.fraction(W.welch32_packed(packed, c.segments, c.step, one_segment), ref, tau) > 1.0


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
