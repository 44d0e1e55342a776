"""The bin-by-bin case matrix of the periodogram's non-linear pre-processing (tests only): RA9MB x / (a + x^2) (fft.c:127-136)
and the limiter sign(y) |y|^0.1 (fft.c:151-156), shared by tests/test_gpu_nonlin.py and tests/test_nonlin_criterion.py, which
runs the float32 stand-in and the oracle against float64 arithmetic on every input of the matrix without a GPU.

A case is tests/_rows_cases.py's Case (est is always 'fft') with `a` and `limiter` beside it; signal(), make_input() and
_frames_for() are that module's.  Every case is one of three settings: the limiter alone, RA9MB alone with a = 0.001 (most
samples in its x / a regime) or a = 0.3, or both together.  Two signals beside that module's: 'full', a +-0.99 tone (RA9MB's
1 / x regime), and 'tiny', 1e-4 in amplitude (x / a; the limiter's logarithm near -10).

The limiter jumps at 0: a sample whose x - mean is tiny comes out near +-0.2 with either sign, so a device mean one bit off
the reference's would move a row beyond any rounding bound.  Hence
  - limiter cases have sub_mean 0 or 1 (the device is asked for the reference-order mean, cfg.sub_mean = 1), never 2;
  - limiter_condition(): in a limiter case with mean removal no sample of any hop has 0 < |x - mean| < 8 * 2^-24 * max|hop|
    (asserted for every case by tests/test_nonlin_criterion.py; a seed that breaks it is changed, not the condition);
  - RA9MB alone is smooth: MEAN2_CASES are its sub_mean = 1 cases whose inputs meet tests/_rows_cases.py's mean2_condition().
Exact zeros are well defined on both sides (log 0 = -inf, exp(-inf) = 0) and wanted: zero history, silence, Hanning's end point.

Which case reaches which kernel file: kernel_file().  Up to N = 16384 glfer_hip.cpp's body_route sends every non-linear plan to
the packed kernel's general form whatever GLFER_FORM says (spectro_small.hip below N = 256).  From N = 32768 launch_wave_private
decides: N = 32768 runs spectro_big.hip by default and spectro16w.hip's general form only for run(spectrum=True) or under
GLFER_FORM=w; larger N run spectro_big.hip.  W_CASES are the N = 32768 cases that tests/test_gpu_nonlin.py runs under
GLFER_FORM=w so that spectro16w.hip's copy of the non-linear branch sees what every other copy sees.
"""
import functools
from collections import namedtuple

import numpy as np

import _exact as X
import _nonlin_exact as NX
import _rows_cases as K
from _rows_cases import _frames_for
from _rows_check import bound, tau_of, tau_of_spectrum

NCase = namedtuple("NCase", K.Case._fields + ("a", "limiter"))

LIM, RA_S, RA_L, BOTH_S, BOTH_L = (0.0, 1), (0.001, 0), (0.3, 0), (0.001, 1), (0.3, 1)


def nl(n, ovl, window, setting, signal="weak", fmt="f32", sub_mean=0, history_mode=0, frames=None):
    a, limiter = setting
    return NCase("fft", n, ovl, window, 0.0, 0, _frames_for(n) if frames is None else frames, signal, fmt, sub_mean, history_mode, a, limiter)


def case_id(c):
    return "n%d-o%g-%s-a%g-l%d-f%d-%s-%s-m%d-h%d" % (c.n, c.ovl, c.window, c.a, c.limiter, c.frames, c.signal, c.fmt, c.sub_mean, c.history_mode)


def setting_of(c):
    return "both" if c.a > 0 and c.limiter else "limiter" if c.limiter else "ra9mb"


def kernel_file(c, w_form=False):
    """w_form: the launch asks for the halfcomplex spectrum or runs under GLFER_FORM=w (glfer_hip.cpp launch_wave_private)."""
    return ("spectro_small.hip" if c.n < 256 else "spectro16.hip" if c.n <= 16384 else "spectro16w.hip" if c.n == 32768 and w_form
            else "spectro_big.hip")


# (a) every size of every route under the three settings; windows, overlaps and signals go round
SIZES = [8, 64, 128, 256, 512, 1024, 4096, 8192, 16384, 32768, 65536, 131072]
_WIN = ["hanning", "kaiser", "blackman", "rectangular"]
_OVL = [0.5, 0.0, 0.75, 0.9, 0.33]
_SIG = ["weak", "noise", "full", "synth", "tiny"]
SIZE_CASES = []
for _i, _n in enumerate(SIZES):
    for _s, _set in enumerate((LIM, RA_S if _i % 2 == 0 else RA_L, BOTH_L if _i % 2 == 0 else BOTH_S)):
        _j = 3 * _i + _s
        _o = _OVL[_j % 5]
        if X.hop_len(_n, _o) < 2:                                 # (N = 8 at 90 %: no whole sample in a hop)
            _o = 0.75
        SIZE_CASES.append(nl(_n, _o, _WIN[_j % 4], _set, _SIG[_j % 5]))

# (b) one sample, one bin, dither and silence: exact zeros through the limiter's log, 0 / (a + 0), rows that must stay 0
EDGE_CASES = [nl(64, 0.0, "rectangular", RA_S, "impulse"), nl(1024, 0.0, "rectangular", LIM, "impulse"), nl(65536, 0.0, "rectangular", BOTH_S, "impulse"),
              nl(256, 0.0, "rectangular", LIM, "bin"), nl(4096, 0.0, "rectangular", BOTH_L, "bin"), nl(32768, 0.0, "rectangular", RA_L, "bin"),
              nl(1024, 0.5, "hanning", LIM, "zero"), nl(4096, 0.75, "hanning", BOTH_S, "zero", "s16"), nl(64, 0.0, "hanning", RA_L, "zero", "u8"),
              nl(32768, 0.5, "kaiser", BOTH_L, "zero"), nl(65536, 0.5, "hanning", LIM, "zero"),
              nl(1024, 0.5, "hanning", BOTH_S, "lsb1", "s16"), nl(256, 0.75, "hanning", LIM, "lsb1", "u8"), nl(4096, 0.0, "kaiser", RA_S, "lsb1", "s16")]

# (c) 16-bit and 8-bit samples under every setting at a small and a packed-range size, and on the two large routes; some
#     streams start 3 samples into their allocation
FORMAT_CASES = [c for fmt in ("s16", "u8") for c in (
    nl(64, 0.5, "hanning", LIM, "weak", fmt), nl(64, 0.75, "kaiser", RA_S, "noise", fmt), nl(128, 0.33, "blackman", BOTH_L, "full", fmt),
    nl(1024, 0.75, "hanning", LIM, "noise", fmt), nl(1024, 0.5, "kaiser", RA_L, "weak", fmt), nl(4096, 0.9, "blackman", BOTH_S, "synth", fmt))]
FORMAT_CASES += [nl(32768, 0.5, "hanning", BOTH_S, "weak", "s16"), nl(32768, 0.0, "kaiser", RA_S, "noise", "u8"),
                 nl(65536, 0.0, "kaiser", LIM, "noise", "u8"), nl(131072, 0.5, "hanning", RA_L, "weak", "s16")]
FORMAT_OFFSETS = {case_id(c): 3 for c in FORMAT_CASES if (c.fmt, c.n) in (("s16", 64), ("u8", 128), ("s16", 1024), ("u8", 4096), ("s16", 32768), ("u8", 65536))}

# (d) per-hop mean removal in the reference's order (the device: cfg.sub_mean = 1) under every setting, in the three formats
MEAN_CASES = [nl(128, 0.5, "hanning", LIM, "weak", "f32", 1), nl(128, 0.75, "kaiser", RA_S, "weak", "f32", 1), nl(64, 0.5, "blackman", BOTH_L, "noise", "f32", 1),
              nl(1024, 0.75, "hanning", LIM, "noise", "f32", 1), nl(1024, 0.5, "kaiser", RA_L, "weak", "f32", 1), nl(4096, 0.5, "hanning", BOTH_S, "synth", "f32", 1),
              nl(4096, 0.9, "blackman", RA_S, "weak", "f32", 1), nl(16384, 0.75, "blackman", LIM, "weak", "f32", 1),
              nl(32768, 0.5, "hanning", BOTH_L, "noise", "f32", 1), nl(32768, 0.75, "kaiser", RA_S, "weak", "f32", 1),
              nl(65536, 0.5, "hanning", RA_L, "weak", "f32", 1), nl(65536, 0.0, "kaiser", LIM, "synth", "f32", 1),
              nl(1024, 0.5, "hanning", LIM, "weak", "s16", 1), nl(1024, 0.33, "hanning", RA_S, "noise", "s16", 1), nl(128, 0.5, "hanning", BOTH_L, "weak", "s16", 1),
              nl(256, 0.0, "kaiser", LIM, "noise", "u8", 1), nl(64, 0.5, "hanning", RA_L, "weak", "u8", 1), nl(4096, 0.75, "kaiser", BOTH_S, "noise", "u8", 1)]
#     RA9MB alone with the in-kernel sums (cfg.sub_mean = 2) where include/glfer_hip.h gives it the reference's rows
MEAN2_CASES = [c for c in MEAN_CASES if not c.limiter and c.fmt == "f32" and c.signal in ("weak", "synth")]

# (e) history zeroed in every frame; launches that start and end inside the stream (first frame; they end 3 frames early)
HISTORY_CASES = [nl(64, 0.75, "hanning", LIM, "weak", "f32", 0, 1), nl(1024, 0.5, "hanning", BOTH_S, "noise", "f32", 0, 1),
                 nl(4096, 0.75, "kaiser", RA_L, "weak", "f32", 1, 1), nl(32768, 0.5, "hanning", LIM, "weak", "f32", 0, 1),
                 nl(65536, 0.5, "hanning", RA_S, "noise", "f32", 0, 1)]
RANGE_CASES = [(nl(128, 0.5, "hanning", LIM, frames=45), 1), (nl(1024, 0.75, "hanning", RA_S, "noise", frames=41), 5),
               (nl(4096, 0.75, "kaiser", BOTH_L, frames=47), 2), (nl(32768, 0.5, "hanning", BOTH_S, frames=11), 3),
               (nl(65536, 0.5, "blackman", LIM, "noise", frames=9), 2)]

# (f) rows on a pitch; halfcomplex spectra (run(spectrum=True): spectro_small.hip, the packed kernel up to N = 16384, spectro16w.hip at 32768)
PITCH_CASES = [(nl(64, 0.5, "hanning", BOTH_S), 48), (nl(1024, 0.5, "kaiser", RA_L, "noise"), 528), (nl(4096, 0.75, "hanning", LIM), 2112),
               (nl(65536, 0.5, "hanning", RA_S), 32800)]
SPECTRUM_CASES = [nl(8, 0.5, "hanning", LIM), nl(64, 0.0, "kaiser", BOTH_L, "noise"), nl(256, 0.75, "hanning", RA_S), nl(1024, 0.5, "blackman", LIM, "noise"),
                  nl(4096, 0.0, "rectangular", BOTH_S, "impulse"), nl(4096, 0.5, "hanning", RA_L, "full"), nl(16384, 0.5, "hanning", LIM),
                  nl(32768, 0.0, "hanning", BOTH_S), nl(32768, 0.5, "kaiser", RA_L, "noise"), nl(32768, 0.75, "blackman", LIM, "synth")]

# (g) N = 32768 under GLFER_FORM=w, spectro16w.hip's general form: (case, first frame of a launch inside the stream or None).  The
#     three settings in f32, with 16-bit and 8-bit samples (some 3 samples into their allocation), with the reference-order mean,
#     with zeroed history and on a frame range
W_CASES = [(c, None) for c in SIZE_CASES if c.n == 32768]
W_CASES += [(nl(32768, 0.75, "hanning", LIM, "weak", "s16"), None), (nl(32768, 0.0, "blackman", RA_L, "noise", "s16"), None),
            (nl(32768, 0.5, "hanning", BOTH_S, "weak", "s16"), None), (nl(32768, 0.33, "kaiser", LIM, "noise", "u8"), None),
            (nl(32768, 0.0, "kaiser", RA_S, "noise", "u8"), None), (nl(32768, 0.5, "blackman", BOTH_L, "full", "u8"), None),
            (nl(32768, 0.5, "hanning", LIM, "weak", "f32", 1), None), (nl(32768, 0.75, "kaiser", RA_S, "weak", "f32", 1), None),
            (nl(32768, 0.5, "hanning", BOTH_L, "noise", "f32", 1), None), (nl(32768, 0.5, "hanning", BOTH_S, "weak", "s16", 1), None),
            (nl(32768, 0.5, "hanning", LIM, "weak", "f32", 0, 1), None), (nl(32768, 0.75, "blackman", RA_L, "noise", "f32", 0, 1), None),
            (nl(32768, 0.5, "kaiser", BOTH_S, "weak", "u8", 0, 1), None),
            (nl(32768, 0.75, "kaiser", LIM, "noise", frames=11), 2), (nl(32768, 0.9, "hanning", RA_L, "weak", frames=11), 4),
            (nl(32768, 0.5, "hanning", BOTH_S, frames=11), 3)]
W_OFFSETS = {case_id(c): 3 for c, _ in W_CASES if (c.fmt, setting_of(c)) in (("s16", "limiter"), ("s16", "both"), ("u8", "both")) and not c.history_mode}

# a seed of its own where tests/_rows_cases.py's seed_of() draws a hop that breaks limiter_condition()
SEEDS = {"n32768-o0.5-hanning-a0.3-l1-f5-noise-f32-m1-h0": 1}

ALL_CASES = list(dict.fromkeys(SIZE_CASES + EDGE_CASES + FORMAT_CASES + MEAN_CASES + HISTORY_CASES + [c for c, _ in RANGE_CASES]
                               + [c for c, _ in PITCH_CASES] + SPECTRUM_CASES + [c for c, _ in W_CASES]))


def make_input(oracle, c):
    return K.make_input(oracle, c, SEEDS.get(case_id(c)))


def window(oracle, c):
    """The plan's float32 window, None for the rectangular one (fft.c:132, 139: no multiply)."""
    return None if c.window == "rectangular" else K.window(oracle, c.n, c.window)


def limiter_condition(c, xf):
    """A limiter case with mean removal: no sample of any whole hop has 0 < |x - mean| < 8 * 2^-24 * max|hop|."""
    if not (c.limiter and c.sub_mean):
        return True
    h = X.hop_len(c.n, c.ovl)
    whole = len(xf) // h * h
    hops = np.asarray(xf[:whole], np.float32).reshape(-1, h)
    d = np.abs(X.remove_hop_means(xf, h)[:whole].reshape(-1, h)).astype(np.float64)
    thr = 8 * 2.0 ** -24 * np.abs(hops).max(axis=1, keepdims=True).astype(np.float64)
    return not bool(((d > 0) & (d < thr)).any())


def rows_of(oracle, c, xf):
    """(exact float64 rows, float32 stand-in rows, oracle rows) of the float stream xf under the case's plan."""
    m = 1 if c.sub_mean else 0
    args = (xf, c.n, c.ovl, window(oracle, c), c.a, c.limiter, m, c.history_mode)
    exact, f32 = NX.periodogram64(*args), NX.periodogram32(*args)
    want = oracle.spectrogram_fft(xf, c.n, c.ovl, oracle.WINDOWS[c.window], c.a, c.limiter, m, c.history_mode)
    assert exact.shape == f32.shape == want.shape == (c.frames, c.n // 2 + 1), (exact.shape, f32.shape, want.shape)
    return exact, f32, want


@functools.lru_cache(maxsize=4)
def reference(oracle, c):
    """tests/_rows_cases.py's Ref of a case: its samples, the three kinds of rows, tau_f32, the bound 4 max(tau_f32, 2^-24),
    the oracle's own tau and its peak-normalised distance from float64."""
    raw, xf = make_input(oracle, c)
    exact, f32, want = rows_of(oracle, c, xf)
    t32 = tau_of(f32, exact)
    return K.Ref(raw, xf, exact, f32, want, t32, bound(t32), tau_of(want, exact), K.peak_err(want, exact))


def spectrum_reference(oracle, c):
    """(raw, xf, exact_X, tau_f32, tau): the complex rule's parts."""
    raw, xf = make_input(oracle, c)
    args = (xf, c.n, c.ovl, window(oracle, c), c.a, c.limiter, 1 if c.sub_mean else 0, c.history_mode)
    exact_X = NX.spectrum64(*args)
    t32 = tau_of_spectrum(NX.spectrum32(*args), exact_X, c.n)
    return raw, xf, exact_X, t32, bound(t32)
