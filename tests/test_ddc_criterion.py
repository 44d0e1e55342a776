"""The down-converter's acceptance rule, shown on the CPU to accept a right float32 computation and to reject wrong ones.

    | got[m] - exact[m] |  <=  tau * A[m],   A[m] = sum_t |g[t]| |x[n0 - t]|,   tau = 4 * max(tau_f32, 2**-24)

tau_f32 is what the float32 stand-in of tests/_ddc_exact.py reaches on the case's own input; the same stand-in on an input of another
seed (held out) must pass under that bound, for every case tests/test_gpu_ddc.py holds the device to.  The wrong outputs:
conjugated taps, one sample of delay, the rotation taken at n0 + 1, reversed taps, freq off by 2^-40 at sample offset 2^36, and a
float32 phase freq * n -- at offset 0 (on noise and on a tone; on the weak-tone input its error stays under the bound, which is
why that variant is not shown there) and at offset 2^36.
"""
import numpy as np
import pytest

import _ddc_cases as Q
import _ddc_exact as X

FREQ = 0.1234567


@pytest.mark.parametrize("c", Q.CASES, ids=Q.case_id)
def test_standin_passes_on_a_held_out_seed(c):
    r = Q.reference(c)
    assert 0 < r.tau_f32 < 2e-6, r.tau_f32                                  # (a float32 sum of up to 8192 terms)
    _, x = Q.make_input(c, seed=Q.seed_of(c) + 101)
    ex, A = X.exact(x, r.g, r.W, c.D, c.first, c.nout, Q.base_of(c))
    y = X.standin32(x, r.g, r.W, c.D, c.first, c.nout, Q.base_of(c))
    frac = X.check(y, ex, A, r.tau, Q.case_id(c))
    print("ddc-criterion %-48s tau_f32 %.3e held-out fraction %.3f" % (Q.case_id(c), r.tau_f32, frac))


def _crit(D, T, signal, first=0, nout=200):
    return Q.Case(D, T, FREQ, 0, "f32", signal, nout, first)


def _worst(y, r):
    live = r.A > 0
    return float((np.abs(y[live] - r.exact[live]) / (r.tau * r.A[live])).max())


@pytest.mark.parametrize("signal", Q.SIGNALS)
@pytest.mark.parametrize("D,T", Q.CRITERION_SHAPES)
def test_wrong_outputs_are_rejected(D, T, signal):
    c = _crit(D, T, signal)
    r = Q.reference(c)
    args = (r.x, r.g, r.W, c.D, c.first, c.nout, Q.base_of(c))
    assert _worst(X.standin32(*args), r) <= 0.25 + 1e-9                      # (tau = 4 tau_f32: the stand-in itself)
    for name, kw in (("conjugated taps", {"conj_taps": True}), ("one sample of delay", {"delay": 1}),
                     ("rotation at n0 + 1", {"rot_at": 1}), ("reversed taps", {"reverse_taps": True})):
        f = _worst(X.standin32(*args, **kw), r)
        print("ddc-criterion D%d T%d %-6s %-22s %.3g of the bound" % (D, T, signal, name, f))
        assert f > 1.0, (name, f)
    if signal != "weak":
        f = _worst(X.standin32(*args, float_phase=FREQ), r)
        print("ddc-criterion D%d T%d %-6s %-22s %.3g of the bound" % (D, T, signal, "float32 phase, offset 0", f))
        assert f > 1.0, f


@pytest.mark.parametrize("signal", Q.SIGNALS)
@pytest.mark.parametrize("D,T", Q.CRITERION_SHAPES)
def test_wrong_phase_far_into_a_stream_is_rejected(D, T, signal):
    c = _crit(D, T, signal, first=(1 << 36) // D, nout=40)
    r = Q.reference(c)
    args = (r.x, r.g, r.W, c.D, c.first, c.nout, Q.base_of(c))
    off = X.phase_word(FREQ + 2.0 ** -40)
    assert off != r.W
    f = _worst(X.standin32(r.x, r.g, off, c.D, c.first, c.nout, Q.base_of(c)), r)
    print("ddc-criterion D%d T%d %-6s %-22s %.3g of the bound" % (D, T, signal, "freq off by 2^-40", f))
    assert f > 1.0, f
    f = _worst(X.standin32(*args, float_phase=FREQ), r)
    print("ddc-criterion D%d T%d %-6s %-22s %.3g of the bound" % (D, T, signal, "float32 phase, offset 2^36", f))
    assert f > 1.0, f
