"""The register-walk and second-unit cases (tests/_walk_cases.py) held to their own conditions on the CPU, no device involved.

1. The references pass: the float32 stand-in at a quarter of the case's bound by construction, the oracle within the suite's
   peak-normalised 1e-5 of float64 below N = 8192 (from there K.oracle_bound's round-4 rule holds the device); the oracle's own tau is
   printed beside the bound, as tests/test_rows_criterion.py does (the device is never held to the oracle bin by bin).
2. The inputs are adversarial where the kernels keep state: in every keyed walk case, at every place `it` of a slot's walk (so at
   every rotation phase it mod 16 / SHIFT and at both parities), the body of every call the GPU module makes holds a frame 10^6
   below its predecessor in float64 power, one 10^6 above, and a silent frame next to a loud one; in every second-unit case a
   workgroup's two units differ in level (tests/test_grid_passes_host.py), and with odd taper counts the second pass holds
   partners 10^6 apart in each order and a silent frame beside a live partner.
3. The rule rejects rows made with a wrong schedule (float32 stand-ins built in numpy from the restated schedule):
     landing_exchanged              the newest hop of one frame a slot taken from the following frame (the PF2 landing sets exchanged;
                                    PF2 is compiled out of this build -- spectro16h.hip:55-57 -- the stand-in stays as the guard)
     kept_hop_stale                 one kept hop at one rotation phase a frame stale
     slot_start_from_previous_slot  a slot's first frame keeping the previous slot's registers where they were
     unit_from_predecessor          a second-pass unit computed from its first-pass predecessor's samples (passes().prev)
     partners_scales_exchanged      odd tapers: the partners' scales exchanged in the second pass only
   and the module prints which of them the peak-normalised 1e-5 alone would accept ('walk-criterion ... old rule accepts').
"""
import numpy as np
import pytest

import _rows_cases as K
import _walk_cases as W
from _rows_check import FLOOR, bound, check_rows, tau_of


def _reference_passes(name, c, r):
    assert np.isfinite(r.exact).all() and (r.exact >= 0).all()
    assert np.isfinite(r.tau_f32) and r.tau == bound(r.tau_f32) and r.tau >= 4 * FLOOR
    assert check_rows(r.f32, r.exact, r.tau, name) <= 0.25 + 1e-12
    print("walk-criterion %-90s tau_f32 %.3e bound %.3e oracle tau %.3e (%.2f of the bound) oracle/float64 peak-normalised %.3e" % (
        name, r.tau_f32, r.tau, r.tau_oracle, r.tau_oracle / r.tau, r.e_ref))
    assert np.isfinite(r.tau_oracle)
    if c.n < 8192:
        assert r.e_ref <= K.TOL, (name, r.e_ref)


def _old_rule_accepts(rows, r, c):
    """Would the suite's peak-normalised rule against the oracle alone let these rows through?"""
    try:
        return K.peak_err(rows, r.want) <= K.oracle_bound(c, r.e_ref)
    except AssertionError:                                     # (a silent row that is not silent)
        return False


def _rejected(name, kind, rows, r, c):
    t = tau_of(rows, r.exact)
    print("walk-criterion %-90s %-30s tau %.3e = %.1f x the bound; old rule accepts: %s" % (name, kind, t, t / r.tau, _old_rule_accepts(rows, r, c)))
    assert t > r.tau, (name, kind, t, r.tau)
    with pytest.raises(AssertionError):
        check_rows(rows, r.exact, r.tau, name)


@pytest.mark.parametrize("c", W.WALK_CASES, ids=K.case_id)
def test_walk_cases(oracle, c):
    name = K.case_id(c)
    r = K.reference(oracle, c, W.seed_of(c))
    _reference_passes(name, c, r)
    power = r.exact.sum(axis=1)
    assert (power > 0).any()
    if W.is_keyed(c):
        ranges = [(0, None)] + ([W.range_of(c)] if c in W.RANGE_CASES else [])
        for lo, hi in ranges:
            ok, lines = W.walk_conditions(c, power, lo, hi)
            assert ok, (name, lo, hi, lines)
    for kind in W.WALK_STANDINS:
        rows, frames = W.walk_standin(oracle, c, r, kind)
        assert len(frames) >= 1 and not np.array_equal(rows[frames], r.f32[frames])
        _rejected(name, kind, rows, r, c)


@pytest.mark.parametrize("c", W.BELOW_CASES, ids=K.case_id)
def test_just_below_cases(oracle, c):
    _reference_passes(K.case_id(c), c, K.reference(oracle, c, W.seed_of(c)))


def test_walk_batch_and_ragged_members(oracle):
    """The second stream of the batch and of the ragged call: their own seeds' conditions."""
    c = W.BATCH_CASE
    r = K.reference(oracle, c, W.seed_of(c, 1))
    _reference_passes(K.case_id(c) + " slot 1", c, r)
    ok, lines = W.walk_conditions(c, r.exact.sum(axis=1))
    assert ok, lines
    c = W.RAGGED_CASE._replace(frames=W.RAGGED_CASE.frames + W.RAGGED_MORE)
    r = K.reference(oracle, c, W.seed_of(W.RAGGED_CASE, 1))
    _reference_passes(K.case_id(c) + " slot 1", c, r)
    ok, lines = W.walk_conditions(c, r.exact.sum(axis=1))
    assert ok, lines


@pytest.mark.parametrize("s", W.SECOND_CASES, ids=W.second_id)
def test_second_unit_cases(oracle, s):
    name = W.second_id(s)
    c = s.c
    r = W.second_reference(oracle, s)
    _reference_passes(name, c, r)
    b0, b1, p = W.second_passes(s)
    late = b0 + np.flatnonzero(p.pass_of >= 1)
    power = r.exact.sum(axis=1)
    if s.dev_mean == 2:
        assert K.mean2_condition(c, r.xf)
    if s.key == "pass":
        # silence in a second unit and in a first, live frames in both: the exact zeros and the rule's line 1 are both asked of either
        first = np.setdiff1d(np.arange(b0, b1), late)
        assert (power[late] > 0).any() and (power[first] > 0).any()
        if W.X.hop_len(c.n, c.ovl) == c.n:                       # (hop = frame: a frame is its hop, so whole frames are silent)
            assert (power[late] == 0).any() and (power[first] == 0).any()
    else:
        ok, cs = W.second_pairs_ok(s, power)
        assert ok, (name, cs)
        _rejected(name, "partners_scales_exchanged", W.second_standin(oracle, s, r, "partners_scales_exchanged"), r, c)
    _rejected(name, "unit_from_predecessor", W.second_standin(oracle, s, r, "unit_from_predecessor"), r, c)

