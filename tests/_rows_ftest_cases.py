"""The case matrix of the rows-and-F entries (tests only): glfer_hip_mtm_rows_ftest_device / Spectrogram.rows_ftest and their
batch forms.  Shared by tests/test_gpu_rows_ftest.py and tests/test_rows_ftest_host.py, which holds the reference alone to
the rules the GPU file uses against it, on every input listed here, without a GPU.

A case is tests/_ftest_cases.py's (n, ovl, nw, kmax, frames, signal, fmt, sub_mean, history_mode); inputs come from its
make_input.  The three rules:
  F rows    bit for bit Spectrogram.ftest's (GPU file); the oracle's by tests/_ftest_check.py::check_ftest against ftest64
  PSD (2)   tests/_rows_check.py::check_rows against multitaper64 with tau = bound(tau_of(multitaper32, exact)): a device
            against float64 rule, never asserted for the oracle
  PSD (3)   per frame max|d|/max and ||d||2/||ref||2 <= max(1e-5, 1.1 err(oracle, exact)) against the oracle's psd of the pair
"""
import functools
from collections import namedtuple

import numpy as np

import _exact as X
import _ftest_cases as K
from _rows_check import bound, tau_of
from _signals import rel_err

TOL = 1e-5
FORMS = ("single", "paired")                      # GLFER_FTEST_PAIRED = 0 / 1

# the smallest shapes that reach each distinct path: (n, ovl, nw, kmax, frames)
SHAPES = {
    "n64": (64, 0.5, 2.5, 3, 29),                 # the epilogue route
    "n256": (256, 0.75, 2.0, 2, 39),              # the smallest in-launch size, several frames per block
    "n512": (512, 0.5, 4.5, 8, 19),
    "n2048_k3": (2048, 0.5, 2.5, 3, 9),           # the smallest default-paired size: five sequences with mu (odd) ...
    "n2048_k4": (2048, 0.0, 2.5, 4, 9),           # ... and six (even)
    "n4096": (4096, 0.0, 2.5, 4, 7),              # several wavefronts per frame
    "n16384": (16384, 0.0, 4.5, 8, 5),
}
SIGNALS = ("noise", "synth")


def shape_case(shape, signal="synth", **kw):
    n, ovl, nw, kmax, frames = SHAPES[shape]
    return K.case(n, ovl, nw, kmax, frames, signal, **kw)


SIZE_CASES = [shape_case(s, sig) for s in sorted(SHAPES) for sig in SIGNALS]

# (4) everything an F entry can be asked: one or two shapes each from N = 256, 2048, 4096
FORMAT_CASES = [shape_case(s, "synth", fmt=f) for f in ("s16", "u8") for s in ("n256", "n2048_k3")]
FORMAT_OFFSET = 3                                 # the stream starts this many samples into its allocation
MEAN_CASES = [shape_case(s, "noise", sub_mean=m) for m in (1, 2) for s in ("n256", "n4096")]
MEAN_CASES += [K.case(2048, 0.75, 2.5, 3, 13, "dc", "f32", 1)]          # the input on which the order of a hop's sum shows
HISTORY_CASES = [K.case(256, 0.75, 2.5, 4, 21, "synth", "f32", 0, 1), K.case(4096, 0.75, 2.5, 4, 9, "noise", "f32", 1, 1)]
# (case, first_frame): the launch ends 3 frames before the stream does
RANGE_CASES = [(K.case(256, 0.75, 2.5, 4, 45, "synth"), 5), (K.case(2048, 0.75, 2.5, 3, 47, "noise", "f32", 1), 32)]
# more frames than one pass of the grid holds (tests/_ftest_cases.py, (g)): N = 16 two epilogue groups, N = 256 and N = 2048
LONG_CASES = list(K.LONG_CASES)
LONG_TAU_FRAMES = 96
PITCH_CASE, PITCH = K.case(4096, 0.0, 2.5, 4, 7), 2112

ALL_CASES = SIZE_CASES + FORMAT_CASES + MEAN_CASES + HISTORY_CASES + [c for c, _ in RANGE_CASES] + LONG_CASES + [PITCH_CASE]

Ref = namedtuple("Ref", "raw xf want_psd want_ft exact tau_f32 tau num den e_ref")


def peak_err(got, want):
    """The worst frame's max(max-norm, 2-norm) error; a row of zeros must be met exactly."""
    worst = 0.0
    for f in range(len(want)):
        if np.asarray(want[f]).any():
            worst = max(worst, max(rel_err(got[f], want[f])))
        else:
            assert not np.asarray(got[f]).any(), "frame %d: the reference's row is 0 and this one is not" % f
    return worst


def oracle_bound(e_ref):
    return max(TOL, 1.1 * e_ref)


def check_against_oracle(got, r, rows=slice(None), what=""):
    """Rule (3), frame by frame; returns the largest fraction of the bound used."""
    want, exact = r.want_psd[rows], r.exact[rows]
    got = np.asarray(got)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    worst = 0.0
    for f in range(len(want)):
        if want[f].any():
            e_dev, b = max(rel_err(got[f], want[f])), oracle_bound(max(rel_err(want[f], exact[f])))
            assert e_dev <= b, (what, f, e_dev, b)
            worst = max(worst, e_dev / b)
        else:
            assert not got[f].any(), (what, f)
    return worst


@functools.lru_cache(maxsize=4)
def reference(oracle, c):
    """Everything the CPU knows of a case.  The reference's mean removal is one thing (fft.c:86-96) whichever way the device
    is asked to take the sums.  tau_f32 comes from the float32 stand-in of tests/_exact.py; on the long cases from its first
    LONG_TAU_FRAMES frames only (the stand-in transforms row by row), which can only make the bound tighter."""
    raw, xf = K.make_input(oracle, c)
    m = 1 if c.sub_mean else 0
    want_psd, want_ft = oracle.spectrogram_mtm_ftest(xf, c.n, c.ovl, c.nw, c.kmax, sub_mean=m, history_mode=c.history_mode, mu_live=1)
    v, sig = oracle.dpss(c.n, c.kmax, c.nw)
    exact = X.multitaper64(xf, c.n, c.ovl, v, sig, m, c.history_mode)
    nf = min(c.frames, LONG_TAU_FRAMES) if c.frames > 4 * LONG_TAU_FRAMES else c.frames
    h = X.hop_len(c.n, c.ovl)
    f32 = X.multitaper32(xf[:nf * h], c.n, c.ovl, v, sig, m, c.history_mode)
    t32 = tau_of(f32, exact[:nf])
    num, den, _ = X.ftest64(xf, c.n, c.ovl, v, c.kmax, sub_mean=m, history_mode=c.history_mode)
    assert want_psd.shape == want_ft.shape == exact.shape == num.shape == (c.frames, c.n // 2 + 1)
    return Ref(raw, xf, want_psd, want_ft, exact, t32, bound(t32), num, den, peak_err(want_psd, exact))
