"""The bin-by-bin rule of the harmonic F rows (tests/_ftest_rows_check.py), shown on the CPU: what it accepts, what its inputs are
worth, and what it rejects.  No device involved.

  (a) the matrix (tests/_ftest_rows_cases.py) holds what it claims, and every `line` input shows its line: in float64 the line's bin
      holds an F of at least 20 and the largest F outside the carrier's bins in every settled frame.
  (b) on every case the float32 stand-in (tests/_exact.py::ftest32) is inside the bound by construction, a quarter of it at the
      most; tau_f32 is finite and no larger than the stand-in's own transforms' error (the derivation's constants: mu and every
      y_j off by at most tau_spec of their row norms give an F off by at most tau_spec under the rule).  The paired stand-in
      (two sequences per transform, separated through the mirror bins) is printed beside it: it is NOT part of tau_f32 -- the
      device's paired form stays inside the one-sequence bound (profiles/ftest_rows.txt) -- and is itself inside the bound.
      The stand-in with its taper sum in the opposite order and ftest64 rounded to float32 are not rejected.
  (c) the oracle's fraction of the bound is recorded on every case and asserted at N <= 2048, where it is measured to pass (at
      most 0.65 on the hosts measured); at N = 4096 it uses up to 1.26 - 1.45 of the bound (`line_on` past it), at N = 8192 / 16384
      3.8 - 23 times the bound on `line` / `line_on`: its recurrence-twiddle transform (fft_radix2.c:127-141), as in the rows of
      tests/test_rows_criterion.py.
  (d) the rule rejects seven kinds of faulty rows, each built from float64 parts and rounded to float32, on every `line` and
      `line_on` case of the size matrix; for each, whether tests/_ftest_check.py::check_ftest accepts it is printed, and at least
      three kinds are accepted by it on some case.

Lines starting with 'ftest-rows-criterion' and 'ftest-rows-mutant' (run with -s) are kept in profiles/ftest_rows.txt.
"""
import functools

import numpy as np
import pytest

import _exact as X
import _ftest_rows_cases as K
from _ftest_check import check_ftest
from _ftest_rows_check import FLOOR, MARGIN, bound, check_ftest_rows, tau_of_ftest
from _rows_cases import mean2_condition

ORACLE_PASSES_UP_TO = 2048


def test_the_matrix_holds_what_it_claims():
    sizes = [8 << i for i in range(12)]
    assert {c.n for c in K.SIZE_CASES} == set(sizes) and sizes[-1] == 16384
    for n in sizes:
        mine = [c for c in K.SIZE_CASES if c.n == n]
        assert (n < 32) != any(c.signal == "line" for c in mine), n
        assert 2 <= sum(c.signal not in K.LINE_KINDS for c in mine), n
        if n >= 2048:
            assert {c.kmax % 2 for c in mine if c.signal == "line"} == {0, 1}, n
    assert {c.nw for c in K.SIZE_CASES} == {2.0, 2.5, 4.0, 4.5}
    assert {c.signal for c in K.SIZE_CASES} == {"line", "line_on", "bin_lo", "bin_hi", "noise", "impulse", "alt", "lsb1", "zero", "gap"}
    assert [(c.n, c.frames > 32768) for c in K.LONG_CASES] == [(16, True)]
    for group in (K.FORMAT_CASES, K.MEAN_CASES, K.HISTORY_CASES, [c for c, _ in K.RANGE_CASES]):
        assert {c.n for c in group} == {128, 2048, 16384} and all(c.signal in K.LINE_KINDS for c in group)
    assert {(c.fmt, c.n) for c in K.FORMAT_CASES} == {(f, n) for f in ("s16", "u8") for n in (128, 2048, 16384)} and K.FORMAT_OFFSET % 2 == 1
    assert {(c.signal, c.sub_mean) for c in K.MEAN_CASES} == {("line_dc", 1), ("line", 2)}
    assert all(c.history_mode == 1 and c.ovl > 0 for c in K.HISTORY_CASES)
    assert [c.signal for c in K.BATCH_MEMBERS] == [c.signal for c in K.RAGGED_MEMBERS] == ["line", "zero", "noise"]
    assert len({c.frames for c in K.RAGGED_MEMBERS}) == 3 and len({c.frames for c in K.BATCH_MEMBERS}) == 1
    for c in K.ALL_CASES:
        assert 5 <= c.frames <= (9 if c.n >= 8192 else 47) or c in K.LONG_CASES or (c, 3) in K.RANGE_CASES, c
        if c.signal in K.LINE_KINDS:
            assert 0.5 <= K.CARRIER <= 0.7 and 40.0 <= K.LINE_DB[(c.nw, c.kmax)] <= 60.0 and K.NOISE_UNDER_LINE_DB >= 30.0


@pytest.mark.parametrize("c", [c for c in K.ALL_CASES if c.signal in K.LINE_KINDS], ids=K.case_id)
def test_line_inputs_show_the_line(oracle, c):
    r = K.reference(oracle, c)
    settled = K.settled_frames(c)
    if c.history_mode:
        # the history zeroed in every frame at an overlap: every frame starts with N - H zeros, a step under every taper, and no
        # frame is settled -- the variation runs the rule on `line`, the line itself is held by the other cases
        assert not settled
        return
    assert len(settled) >= 5
    least, largest = K.line_conditions(c, r.num, r.den)
    print("ftest-rows-criterion %-48s line %g dB under the carrier, bin %d: least F64 %.4g in %d settled frames, the largest outside the carrier's bins: %s" % (
        K.case_id(c), K.LINE_DB[(c.nw, c.kmax)], K.line_bin(c.n), least, len(settled), largest))
    assert least >= 20.0 and largest
    if c.sub_mean == 2:
        assert mean2_condition(c, r.xf)


def _tau_spec(oracle, c, xf):
    """The stand-in's own transforms against float64: the largest |Y32[k] - Y64[k]| over the row's norm below Nyquist, over hn and the tapers."""
    m = 1 if c.sub_mean else 0
    fr = X.frames64(xf, c.n, c.ovl, m, c.history_mode)
    v32, _, _, hn = X._ftest32_tables(K.tapers(oracle, c.n, c.kmax, c.nw), c.kmax)
    worst = 0.0
    for s in [hn] + list(v32):
        e = np.fft.rfft(fr * s.astype(np.float64), axis=1)
        norm = np.sqrt((np.abs(e[:, :-1]) ** 2).sum(axis=1))
        live = norm > 0
        if live.any():
            g = X._rfft32(fr[live].astype(np.float32) * s)
            worst = max(worst, float((np.abs(g - e[live])[:, :-1].max(axis=1) / norm[live]).max()))
    return worst


@pytest.mark.parametrize("c", K.ALL_CASES, ids=K.case_id)
def test_stand_ins_oracle_and_float64(oracle, c):
    r = K.reference(oracle, c)
    what = K.case_id(c)
    m = 1 if c.sub_mean else 0
    v = K.tapers(oracle, c.n, c.kmax, c.nw)
    assert np.isfinite(r.tau_f32) and r.tau_f32 == r.tau_single and r.tau == bound(r.tau_f32) == MARGIN * max(r.tau_f32, FLOOR)
    silent = r.tot[:, :-1].sum(axis=1) == 0
    assert silent.all() == (c.signal == "zero") and silent.any() == (c.signal in ("zero", "gap"))
    assert np.isnan(r.want[silent]).all()                                # the oracle's silent rows: 0 / 0 in every bin
    assert not ((r.den[~silent, :-1] == 0).any())                       # (no bin of a frame with power is x / 0 in float64)
    with np.errstate(all="ignore"):
        # (b) the stand-in, its paired form, the opposite order of the taper sum, float64 rounded once
        assert check_ftest_rows(r.f32, r.want, r.num, r.den, r.tot, c.kmax, r.tau, what)[0] <= 1.0 / MARGIN + 1e-12
        paired = X.ftest32_paired(r.xf, c.n, c.ovl, v, c.kmax, m, c.history_mode)[0]
        rev = X.ftest32(r.xf, c.n, c.ovl, v, c.kmax, m, c.history_mode, reverse=True)[0]
        once = _rows(r.num, r.den)
        f_paired = check_ftest_rows(paired, r.want, r.num, r.den, r.tot, c.kmax, r.tau, "paired stand-in: " + what)[0]
        f_rev = check_ftest_rows(rev, r.want, r.num, r.den, r.tot, c.kmax, r.tau, "opposite order: " + what)[0]
        f_once = check_ftest_rows(once, r.want, r.num, r.den, r.tot, c.kmax, r.tau, "float64 rounded: " + what)[0]
    assert np.isfinite(r.tau_paired)
    # the derivation's constants: the stand-in needs no more than its own transforms' error (and the float32 arithmetic after them)
    spec = _tau_spec(oracle, c, r.xf) if c not in K.LONG_CASES else np.inf
    assert r.tau_f32 <= 1.01 * spec + FLOOR, (r.tau_f32, spec)
    # (c) the oracle
    t_oracle = tau_of_ftest(r.want, r.num, r.den, r.tot, c.kmax)
    print("ftest-rows-criterion %-48s tau_f32 %.3e (transforms %.3e, paired stand-in %.3e) tau %.3e | of the bound: paired %.3f opposite order %.3f "
          "float64 rounded %.3f oracle %.3f" % (what, r.tau_f32, spec, r.tau_paired, r.tau, f_paired, f_rev, f_once, t_oracle / r.tau))
    if c.n <= ORACLE_PASSES_UP_TO:
        with np.errstate(all="ignore"):
            check_ftest_rows(r.want, r.want, r.num, r.den, r.tot, c.kmax, r.tau, "oracle: " + what)


# ---- (d) faulty rows ----------------------------------------------------------------------------------------------------------------------
VARIANTS = ["line's F x 1.2", "floor under den", "mu from taper 0", "taper missing", "separation leak", "U0 in bfloat16", "frames exchanged"]
MUTANT_CASES = [c for c in K.SIZE_CASES if c.signal in ("line", "line_on")]


def _bfloat16(x):
    b = np.asarray(x, np.float32).view(np.uint32)
    return ((b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000).astype(np.uint32).view(np.float32).astype(np.float64)


def _rows(num, den):
    """num / den rounded once to float32, the Nyquist column x / 0 as the reference leaves it."""
    with np.errstate(all="ignore"):
        rows = (num / den).astype(np.float32)
        rows[:, -1] = (num[:, -1] / 0.0).astype(np.float32)
    return rows


@functools.lru_cache(maxsize=None)
def _verdicts(oracle, c):
    """{variant: (fraction of the new bound its rows reach, whether check_ftest accepts them)}"""
    r = K.reference(oracle, c)
    m = 1 if c.sub_mean else 0
    fr = X.frames64(r.xf, c.n, c.ovl, m, c.history_mode)
    v = np.asarray(K.tapers(oracle, c.n, c.kmax, c.nw), np.float64)[:c.kmax + 1]
    U0 = v.sum(axis=1)
    s2 = (U0 * U0).sum()
    mu = np.fft.rfft(fr * ((U0[:, None] * v).sum(axis=0) / s2), axis=1)
    ys = [np.fft.rfft(fr * v[j], axis=1) for j in range(c.kmax + 1)]

    def parts(mu, ys, U=U0, skip=()):
        return c.kmax * np.abs(mu) ** 2 * s2, sum(np.abs(ys[j] - mu * U[j]) ** 2 for j in range(c.kmax + 1) if j not in skip)

    num, den = parts(mu, ys)
    assert np.allclose(num, r.num, rtol=1e-9, atol=0) and np.allclose(den[:, :-1], r.den[:, :-1], rtol=1e-9, atol=0)
    settled = K.settled_frames(c)
    wrong = {}
    rows = _rows(num, den)
    rows[settled, K.line_bin(c.n)] *= np.float32(1.2)
    wrong["line's F x 1.2"] = rows
    wrong["floor under den"] = _rows(num, den + 1e-6 * den[:, :-1].max(axis=1, keepdims=True))
    wrong["mu from taper 0"] = _rows(*parts(ys[0] / U0[0], ys))
    wrong["taper missing"] = _rows(*parts(mu, ys, skip=(c.kmax,)))
    # the sequences hn, taper 0 ... kmax go two at a time: (hn, taper 0), (taper 1, taper 2) ...; the first of a pair takes 1e-5 of the second
    ex = int(np.frexp(np.sqrt(s2))[1])
    leaky = [y.copy() for y in ys]
    for j in range(1, c.kmax, 2):
        leaky[j] += 1e-5 * ys[j + 1]
    wrong["separation leak"] = _rows(*parts(mu + 1e-5 * ys[0] / 2.0 ** (ex - 1), leaky))
    wrong["U0 in bfloat16"] = _rows(*parts(mu, ys, U=_bfloat16(U0)))
    f = settled[len(settled) // 2]
    rows = _rows(num, den)
    rows[f] = _rows(num[f + 1:f + 2] if f + 1 < c.frames else num[f - 1:f], den[f:f + 1])[0]
    wrong["frames exchanged"] = rows
    out = {}
    for name, rows in wrong.items():
        try:
            with np.errstate(all="ignore"):
                check_ftest(rows, r.want, r.num, r.den, c.kmax)
            old = True
        except AssertionError:
            old = False
        out[name] = (tau_of_ftest(rows, r.num, r.den, r.tot, c.kmax) / r.tau, old)
    return out


@pytest.mark.parametrize("c", MUTANT_CASES, ids=K.case_id)
def test_rule_rejects_faulty_rows(oracle, c):
    got = _verdicts(oracle, c)
    assert list(got) == VARIANTS
    for name, (frac, old) in got.items():
        print("ftest-rows-mutant %-48s %-18s %10.3g of the bound: %s; check_ftest %s it" % (
            K.case_id(c), name, frac, "rejected" if frac > 1.0 else "NOT REJECTED", "accepts" if old else "rejects"))
    for name, (frac, _) in got.items():
        assert frac > 1.0, (name, frac)


def test_faulty_rows_the_present_rule_accepts(oracle):
    accepted = {v: [K.case_id(c) for c in MUTANT_CASES if _verdicts(oracle, c)[v][1]] for v in VARIANTS}
    for v in VARIANTS:
        print("ftest-rows-mutant %-18s check_ftest accepts it on %d of %d cases" % (v, len(accepted[v]), len(MUTANT_CASES)))
    assert sum(bool(ids) for ids in accepted.values()) >= 3, accepted
    assert len(accepted["line's F x 1.2"]) >= 1


def test_rule_parts_one_by_one(oracle):
    """A finite Nyquist value, a negative value, a NaN and an infinity below Nyquist, and a silent frame that is not the oracle's
    NaN row, each fail by themselves; the rows they were made from pass."""
    c = next(c for c in K.SIZE_CASES if c.signal == "gap" and c.n == 64)
    r = K.reference(oracle, c)
    silent = int(np.flatnonzero(r.tot[:, :-1].sum(axis=1) == 0)[0])
    loud = 0 if silent else 1
    good = _rows(r.num, r.den)

    def judge(rows):
        with np.errstate(all="ignore"):
            return check_ftest_rows(rows, r.want, r.num, r.den, r.tot, c.kmax, r.tau)[0]

    assert judge(good) <= 1.0
    for frame, k, value in ((loud, c.n // 2, 1.0), (loud, 3, -good[loud, 3]), (loud, 5, np.nan), (loud, 7, np.inf), (silent, 2, 0.0), (silent, 4, np.inf)):
        rows = good.copy()
        rows[frame, k] = value
        with pytest.raises(AssertionError):
            judge(rows)
        assert frame == silent or k == c.n // 2 or tau_of_ftest(rows, r.num, r.den, r.tot, c.kmax) == np.inf
