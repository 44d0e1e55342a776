"""What the drift tests rest on, shown without a GPU.

1. The detection premise, in float64: a line of constant power along k0 + o(d0, t) in unit-mean exponential noise is found by the
   search -- in every block the largest `best` lies at k0 with drift d0 and stands at least 1.25 times over the largest `best`
   outside k0 +- 2.  Fixed seeds (tests/_drift_cases.py); tests/test_gpu_drift.py runs the same inputs on the device.
2. The bit-for-bit comparison of tests/test_gpu_drift.py rejects wrong kernels: every mutation of the restatement below changes
   at least one output bit on each device case it is claimed for, so a kernel that made that mistake could not pass there."""
import numpy as np
import pytest

import _drift_cases as K
import _drift_exact as X


@pytest.mark.parametrize("c", K.DETECT, ids=lambda c: "T%d_b%d_A%g_d%d" % (c.T, c.bins, c.A, c.d0))
def test_a_drifting_line_is_found_in_float64(c):
    rows = K.detect_rows(c)
    r = c.T - 1
    _, best, drift = X.drift_all(rows, c.bins, c.T, c.T, -r, r, dtype=np.float64)
    assert best.shape == (K.DETECT_BLOCKS, c.bins)
    margins = K.detect_check(c, best, drift)
    print("margins", c, ["%.2f" % m for m in margins])
    # and the fixed-bin integration the library had before loses it: the zero-drift sum at k0 is not the row's largest
    zero = X.drift_sums(rows, c.bins, c.T, c.T, 0, 0, dtype=np.float64)[:, 0, :]
    assert all(zero[b].max() < best[b][K.detect_k0(c)] for b in range(K.DETECT_BLOCKS))


# ---- the mutations: name -> (which cases it is claimed for, the mutated outputs of a case)
def _outputs(case, order=None, **kw):
    s = X.drift_sums(K.make_rows(case), case.bins, case.T, case.step, case.dmin, case.dmax, **kw)
    return (s,) + X.best_drift(s, case.dmin, order)


def _noise(c):
    return c.kind == "noise"


def _has_tie(c, negative_only):
    """a (d, t) of the case at which d t / (T - 1) lies half way between two integers (and d < 0)"""
    return any((2 * abs(d) * t) % (2 * (c.T - 1)) == c.T - 1 for d in range(c.dmin, (0 if negative_only else c.dmax + 1)) for t in range(c.T))


MUTATIONS = {
    # half up: differs from half away from zero at the ties of negative drifts
    "round_half_up": (lambda c: _noise(c) and c.bins > 1 and _has_tie(c, True),
                      lambda c: _outputs(c, offs=X.offsets(c.T, c.dmin, c.dmax, "up"))),
    "round_half_even": (lambda c: _noise(c) and c.bins > 1 and _has_tie(c, False),
                        lambda c: _outputs(c, offs=X.offsets(c.T, c.dmin, c.dmax, "even"))),
    # (with one bin every line but the zero-drift one leaves the row at once, either way)
    "offset_sign_flipped": (lambda c: _noise(c) and c.bins > 1 and c.dmax - c.dmin > 0,
                            lambda c: _outputs(c, offs=-X.offsets(c.T, c.dmin, c.dmax))),
    # rows whose levels differ by decades frame to frame; two terms commute
    "summed_downwards": (lambda c: _noise(c) and c.T >= 3, lambda c: _outputs(c, downward=True)),
    "block_one_row_late": (lambda c: _noise(c) and c.F > (X.blocks(c.F, c.T, c.step) - 1) * c.step + c.T, lambda c: _outputs(c, late=1)),
    "one_term_short": (_noise, lambda c: _outputs(c, terms=c.T - 1)),
    # the padding (1e30) or the neighbouring row (loud) where the definition has zero
    "outside_read_from_memory": (lambda c: _noise(c) and c.dmax - c.dmin > 0, lambda c: _outputs(c, outside="flat")),
    "ties_to_the_lowest_index": (lambda c: c.kind in ("silence", "const", "cross"),
                                 lambda c: _outputs(c, order=range(c.dmin, c.dmax + 1))),
    # (on silence and on the constant plane drift 0 is never beaten: the two lines through one bin that tie above it are "cross")
    "minus_d_before_plus_d": (lambda c: c.kind == "cross", lambda c: _outputs(c, order=X.scan_order(c.dmin, c.dmax, neg_first=True))),
}
CLAIMS = [(m, c) for m, (claimed, _) in MUTATIONS.items() for c in K.CASES if claimed(c)]


def test_every_mutation_is_claimed_for_several_cases_and_every_case_by_some():
    for m in MUTATIONS:
        assert sum(1 for mm, _ in CLAIMS if mm == m) >= (1 if m == "minus_d_before_plus_d" else 3), m
    assert {c.name for _, c in CLAIMS} == {c.name for c in K.CASES if c.kind not in ("inf", "nan")}


@pytest.mark.parametrize("m,c", CLAIMS, ids=lambda v: v if isinstance(v, str) else v.name)
def test_mutation_changes_an_output_bit(m, c):
    want = K.reference(c)
    got = MUTATIONS[m][1](c)
    changed = [name for name, a, b in zip(("sums", "best", "drift"), got, want) if not X.same_bits(a, b)]
    assert changed, (m, c.name)


def test_the_special_cases_hold_what_they_are_for():
    s, best, drift = K.reference(K.BY_NAME["silence"])
    assert not s.any() and not best.any() and not drift.any() and not np.signbit(best).any()      # best = +0, drift = 0
    s, best, drift = K.reference(K.BY_NAME["const"])
    assert not drift.any() and np.all(best == np.float32(1.5 * 16))
    assert s[:, 0, :].min() < s[:, 15, :].min()                  # fewer terms at the edges: the term counts differ
    s, best, drift = K.reference(K.BY_NAME["cross"])
    assert np.all(s[:, 15 + 9, 32] == s[:, 15 - 9, 32]) and np.all(s[:, 15 + 9, 32] > s[:, 15, 32]) and np.all(drift[:, 32] == 9)
    s, best, drift = K.reference(K.BY_NAME["nan"])
    assert np.isnan(best[0, 30]) and drift[0, 30] == 0           # NaN on the zero-drift line: NaN with drift 0
    off = np.isnan(s[0]).any(axis=0) & ~np.isnan(s[0, 15])       # bins whose other lines cross the NaN
    assert off.sum() >= 5 and not np.isnan(best[0][off]).any()   # a NaN elsewhere never wins
    s, best, drift = K.reference(K.BY_NAME["inf"])
    assert np.isinf(best).any() and not np.isnan(s).any()
