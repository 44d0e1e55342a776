"""The acceptance rule of the zoom rows, shown on the CPU: what it accepts, what its inputs are worth, and what it rejects.

tests/test_gpu_zoom.py holds every bin of every frame of Spectrogram.run_zoom to

    | sqrt(got[k]) - sqrt(exact[k]) |  <=  tau * sqrt( sum_k exact[k] ),    tau = 4 * max(tau_f32, 2**-24)

(tests/_rows_check.py, unchanged) with `exact` float64 through both stages and tau_f32 the LARGER of two float32 stand-ins of both
stages in a row: the down-converter's sum taken in tap order and in the row order ddc.hip documents.  On the `line` scene (a weak
line beside a strong carrier the filter removes) a row's partial sum holds the carrier aliased at stride D until the other rows
cancel it, and the row order is the worse one: the ratio is printed per case.  Here, for every case of tests/_zoom_cases.py:

  (a) both stand-ins are inside the bound by construction (a quarter of it at the most); a third order held out of the bound --
      taps descending -- stays inside it too.
  (b) `line` scenes show the line: in the float64 rows, in every frame past the filter's start-up, the line's peak stands 20 dB
      above every bin outside its own lobe (tests/_zoom_cases.py lobe(): a line off a bin centre fills its window's main lobe,
      so the neighbours inside it are not held to 20 dB).  NO_LINE lists the shapes whose filter cannot give that.
  (c) the rule rejects wrong rows, each built from the float32 stand-in with one change: rows mirrored k -> -k, rows rolled by one
      bin, frames taken one hop late, conjugated taps, a float32 phase (far into a stream), the last taper dropped (multitaper).
      A variant the rule cannot see on a scene is printed as unseen there (a hop's delay on stationary tones; anything on silence)
      and must be seen on another.  The rotation evaluated at n0 + 1 is the exception: W (n0 + 1) = W n0 + W, so it turns every
      output by the one angle -2 pi freq and NO power row of any scene holds it.  It is shown to be exactly that -- the right
      baseband times one unit constant -- and printed as unseen everywhere; the down-converter's own rule (tests/test_ddc_criterion.py)
      is the one that rejects it.

Lines starting with 'zoom-criterion' and 'zoom-mutant' (run with -s) are kept in profiles/zoom_rows.txt.
"""
import functools

import numpy as np
import pytest

import _ddc_exact as X
import _zoom_cases as Z
from _rows_check import FLOOR, bound, check_rows, tau_of

NO_LINE = [(1, 1), (5, 4)]                                            # (D, T) whose default filter leaves the carrier above the line


def test_the_matrix_holds_what_it_claims():
    ns = {c.n for c in Z.CASES}
    assert ns == {256, 512, 1024, 2048, 4096, 8192, 16384}
    for n in ns:
        assert any(c.n == n and c.scene == "line" for c in Z.CASES) and any(c.n == n and c.scene != "line" for c in Z.CASES), n
    assert {(c.D, c.T) for c in Z.CASES} == {(1, 1), (3, 17), (5, 4), (16, 129), (64, 513), (100, 401), (1024, 1025), (7, 8192)}
    assert all(c.n == 256 for c in Z.CASES if (c.D, c.T) in ((1024, 1025), (7, 8192)))
    kinds = [(c.cplx, c.fmt) for c in Z.CASES]
    assert all(kinds.count((cp, f)) >= 2 for cp in (0, 1) for f in ("f32", "s16", "u8"))
    assert {c.ovl for c in Z.CASES} == {0.0, 0.5, 0.75, 0.3} and {c.window for c in Z.CASES} == {"hanning", "kaiser", "rectangular"}
    assert {(c.n, c.kmax + 1) for c in Z.CASES if c.est == "mtm"} >= {(1024, 1), (1024, 4), (1024, 5), (4096, 1), (4096, 4), (4096, 5), (16384, 9)}
    assert sum(c.history_mode for c in Z.CASES) == 3
    assert {c.scene for c in Z.CASES} == {"line", "pair", "noise", "zero"}
    assert Z.fft(64, 513, Z.F1, 0, "f32", 16384, 0.5, "hanning", 3, "line") in Z.CASES
    far = [c for c in Z.CASES if c.first]
    assert [(c.D, c.T, c.n, c.cplx, c.fmt) for c in far] == [(16, 129, 1024, 0, "f32"), (3, 17, 4096, 1, "s16")]
    for c in far:
        dh = c.D * Z.hop(c)
        assert c.first == -(-(1 << 36) // dh) + 3 and Z.lo_hi(c)[0] * c.D > 1 << 32 and Z.base_of(c) == Z.lo_hi(c)[0] * c.D - (c.T - 1)
    for c in Z.CASES:
        assert c.frames == (37 if c.n <= 1024 else 7 if c.n == 2048 else 3 if c.n == 16384 else 5) or c.T == 8192
        assert not (c.scene == "line" and ((c.D, c.T) in NO_LINE or c.window == "rectangular" and c.est == "fft"))
        assert len(Z.make_input(c)[0]) == Z.nsamples_of(c) - Z.base_of(c)


def test_orders_of_the_sum():
    assert X.tap_order(3, 8, "taps") == [0, 1, 2, 3, 4, 5, 6, 7] and X.tap_order(3, 8, "rows") == [0, 3, 6, 1, 4, 7, 2, 5]
    assert X.tap_order(5, 4, "rows") == [0, 1, 2, 3] and X.tap_order(1, 3, "rows") == [0, 1, 2] and X.tap_order(3, 4, "down") == [3, 2, 1, 0]
    for D, T in ((16, 129), (100, 401), (7, 8192), (1024, 1025)):
        assert sorted(X.tap_order(D, T, "rows")) == list(range(T))


@pytest.mark.parametrize("c", Z.CASES, ids=Z.case_id)
def test_stand_ins_and_a_held_out_order(oracle, c):
    r = Z.reference(oracle, c)
    assert np.isfinite(r.exact).all() and (r.exact >= 0).all()
    assert np.isfinite(r.tau_f32) and r.tau_f32 == max(r.tau_taps, r.tau_rows) and r.tau == bound(r.tau_f32) and r.tau >= 4 * FLOOR
    for rows in (r.f32, r.f32_rows):
        assert check_rows(rows, r.exact, r.tau, Z.case_id(c)) <= 0.25 + 1e-12
    down = Z.rows32(oracle, c, Z.baseband32(c, r, order="down"))
    t_down = tau_of(down, r.exact)
    print("zoom-criterion %-64s tau_f32(taps) %.3e tau_f32(rows) %.3e rows/taps %.2f bound %.3e held-out (taps descending) %.3e = %.3f of the bound" % (
        Z.case_id(c), r.tau_taps, r.tau_rows, r.tau_rows / r.tau_taps if r.tau_taps else 1.0, r.tau, t_down, t_down / r.tau))
    check_rows(down, r.exact, r.tau, "held out: " + Z.case_id(c))
    if c.scene == "zero":
        assert not r.exact.any() and not r.f32.any() and not r.f32_rows.any() and not r.x.any()
    else:
        assert r.exact.sum(axis=1).min() > 0
        if c.cplx:
            assert r.x.real.std() != r.x.imag.std()


def _line_margin_db(c, exact):
    """The least, over the settled frames, of peak / largest bin outside the line's lobe, in dB; and whether the peak is the line's."""
    k = np.arange(c.n)
    d = np.abs((k - Z.line_bin(c) + c.n // 2) % c.n - c.n // 2)
    frames = Z.settled_frames(c)
    assert len(frames) >= 1, "a `line` case needs a frame past the filter's start-up"
    worst, on = np.inf, True
    for f in frames:
        row = exact[f]
        on = on and d[int(np.argmax(row))] <= (np.ceil(c.nw) if c.est == "mtm" else 0)
        worst = min(worst, 10 * np.log10(row.max() / row[d > Z.lobe(c)].max()))
    return worst, on


@pytest.mark.parametrize("c", [c for c in Z.CASES if c.scene == "line"], ids=Z.case_id)
def test_line_scenes_show_the_line(oracle, c):
    r = Z.reference(oracle, c)
    db, on = _line_margin_db(c, r.exact)
    print("zoom-criterion %-64s line bin %d stands %.1f dB above every bin outside its lobe (+-%d) in %d frames" % (
        Z.case_id(c), Z.line_bin(c), db, Z.lobe(c), len(Z.settled_frames(c))))
    assert on and db >= 20.0, (db, on)


@pytest.mark.parametrize("D,T", NO_LINE)
def test_shapes_that_cannot_show_the_line(oracle, D, T):
    """Why these shapes carry the other scenes: their default filter leaves the carrier within 20 dB of the line, or above it."""
    c = Z.fft(D, T, Z.F1, 1, "f32", 256, 0.5, "hanning", 37, "line")
    raw, x = Z.make_input(c)
    W = X.phase_word(c.freq)
    exact = Z.rows64(oracle, c, Z.exact_baseband(c, x, X.tables(W, X.design(D, T)), W))
    db, _ = _line_margin_db(c, exact)
    print("zoom-criterion D%d T%d cannot carry `line`: the line's bin stands %.1f dB above the rest" % (D, T, db))
    assert db < 20.0


# ---- (c) wrong rows ---------------------------------------------------------------------------------------------------------------------
VARIANTS = ["mirrored", "rolled one bin", "one hop late", "conjugated taps", "float32 phase", "taper dropped"]


@functools.lru_cache(maxsize=None)
def _verdicts(oracle, c):
    """{variant: fraction of the bound its rows reach} for the variants the case can build."""
    r = Z.reference(oracle, c)
    k = np.arange(c.n)
    wrong = {"mirrored": r.f32[:, (c.n - k) % c.n], "rolled one bin": np.roll(r.f32, 1, axis=1),
             "one hop late": np.concatenate([r.f32[1:], r.f32[-1:]]),
             "conjugated taps": Z.rows32(oracle, c, Z.baseband32(c, r, conj_taps=True))}
    if c.first:
        wrong["float32 phase"] = Z.rows32(oracle, c, Z.baseband32(c, r, float_phase=c.freq))
    if c.est == "mtm" and c.kmax > 0:
        wrong["taper dropped"] = Z.rows32(oracle, c, Z.baseband32(c, r), ntap=c.kmax)
    for name, rows in wrong.items():
        assert rows.shape == r.exact.shape, name
    return {name: tau_of(rows, r.exact) / r.tau for name, rows in wrong.items()}


@pytest.mark.parametrize("c", Z.CASES, ids=Z.case_id)
def test_rule_on_wrong_rows(oracle, c):
    r = Z.reference(oracle, c)
    assert check_rows(r.exact, r.exact, r.tau) == 0.0
    for name, frac in _verdicts(oracle, c).items():
        print("zoom-mutant %-64s %-16s %10.3g of the bound: %s" % (Z.case_id(c), name, frac, "rejected" if frac > 1.0 else "UNSEEN on this scene"))
    # the rotation at n0 + 1: the right baseband times one unit constant, which no power row holds
    if c.scene != "zero":
        y = Z.baseband32(c, r)
        turned = Z.baseband32(c, r, rot_at=1)
        unit = np.exp(-2j * np.pi * X.turns(r.W, 1))
        assert np.abs(turned - y * unit).max() <= 4 * 2.0 ** -24 * np.abs(y).max()
        frac = tau_of(Z.rows32(oracle, c, turned), r.exact) / r.tau
        print("zoom-mutant %-64s %-16s %10.3g of the bound: UNSEEN on every scene (one constant phase)" % (Z.case_id(c), "rotation at n0+1", frac))
        assert frac <= 1.0


def test_every_variant_is_rejected_on_some_scene(oracle):
    seen = {v: set() for v in VARIANTS}
    unseen = {v: set() for v in VARIANTS}
    for c in Z.CASES:
        for name, frac in _verdicts(oracle, c).items():
            (seen if frac > 1.0 else unseen)[name].add(c.scene)
    for v in VARIANTS:
        print("zoom-mutant %-16s rejected on %s; unseen on %s" % (v, sorted(seen[v]) or "-", sorted(unseen[v]) or "-"))
        assert seen[v], v
    # what zoom is for: on every `line` case the orientation, the bin and the filter's side are all under the rule
    for c in Z.CASES:
        if c.scene == "line":
            v = _verdicts(oracle, c)
            assert min(v["mirrored"], v["rolled one bin"], v["conjugated taps"]) > 1.0, (Z.case_id(c), v)
