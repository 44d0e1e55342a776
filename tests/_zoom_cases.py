"""The case matrix of the zoom rows (tests only), shared by tests/test_zoom_criterion.py (CPU) and tests/test_gpu_zoom.py:
Spectrogram.run_zoom / glfer_hip_spectrogram_zoom_device, the two-sided rows of the down-converter's output.

A case is (D, T, freq, cplx, fmt | est, n, ovl, window, nw, kmax, history_mode | frames, scene, first): the converter (the default
design for D with T taps, the frequency moved to 0 Hz, real or complex input, sample format), the plan (as tests/_iq_cases.py: 'fft'
with a window name, or 'mtm' with NW and kmax + 1 tapers) and the frames [first, first + frames) of the rows.  first > 0: a piece far
into a stream, holding the input samples from lo D - (T - 1) on (lo: the first baseband sample the frames read) and passed by its
virtual base.  The input ends D/2 + 1 samples past the last frame's last sample: a ragged tail.

Scenes (seeded; clipped and converted by _ddc_cases.convert; real input: the real part; complex input: Q at 0.8 of its size, so I
and Q never have the same power):
  line    a 0.7 carrier at freq + 0.37 (out of band), a line 60 dB below it at freq + 0.0731 / D, noise 120 dB below the carrier
  pair    a 0.6 tone at freq + 0.0731 / D, a second 80 dB below it at freq - 0.1313 / D (a negative baseband bin), noise 100 dB below
  noise   Gaussian, sigma 0.25 (complex: 0.25 and 0.1 on I and Q, a DC level on Q), as tests/_ddc_cases.py
  zero    silence: every row exactly 0

Frame counts fill and overrun a workgroup's frame group: 37 up to N = 1024, 7 at 2048, 5 from 4096, 3 at 16384 (the 8192-tap shape:
21, its float64 side is the slowest of the matrix).  Every N = 256 .. 16384 has a `line` case and a case of another scene.  `line`
goes where the float64 rows show the line 20 dB above everything outside its own lobe (tests/test_zoom_criterion.py): the shapes
whose default filter takes the carrier that far down -- all but (1,1) and (5,4) -- under Hanning, Kaiser or tapers (a rectangular
window does not keep a line off a bin centre within a lobe), f32 or s16 input (a u8 carrier's quantisation spurs stand 10 dB under
the line), history_mode 0 (one hop under a whole window is a truncated window) and without NW = 4.5's ninth taper.  `line`
frequencies are 0.1234567 and 0.25 + 2^-40: at 0 and -0.49 the image of a real (or unequal I/Q) input falls into the band.

reference(oracle, c) is everything the CPU knows of a case; nothing in it comes from a device.  The float64 rows are
_iq_exact.periodogram64 / multitaper64 of the float64 baseband (which those functions take as complex64 samples: a relative 2^-25 a
sample, under 2^-25 / sqrt(N) of a row's amplitude scale, against a bound of 2^-22 at the least).
"""
import functools
from collections import namedtuple

import numpy as np

import _ddc_cases as DQ
import _ddc_exact as X
import _iq_exact as XC
import _rows_cases as K
from _exact import hop_len
from _rows_check import bound, tau_of

Case = namedtuple("Case", "D T freq cplx fmt est n ovl window nw kmax history_mode frames scene first")
F1, F2 = 0.1234567, 0.25 + 2.0 ** -40
LINE_AT, PAIR_AT = 0.0731, -0.1313                               # baseband frequencies, cycles per baseband sample


def fft(D, T, freq, cplx, fmt, n, ovl, window, frames, scene, history_mode=0, first=0):
    return Case(D, T, freq, cplx, fmt, "fft", n, ovl, window, 0.0, 0, history_mode, frames, scene, first)


def mtm(D, T, freq, cplx, fmt, n, ovl, nw, kmax, frames, scene, history_mode=0, first=0):
    return Case(D, T, freq, cplx, fmt, "mtm", n, ovl, "rectangular", nw, kmax, history_mode, frames, scene, first)


def far_first(D, n, ovl):
    """The first frame of a case far into a stream: ceil(2^36 / (D H)) + 3."""
    dh = D * hop_len(n, ovl)
    return -((-(1 << 36)) // dh) + 3


def case_id(c):
    return "D%d-T%d-f%.7g-%s-%s-%s-n%d-o%g-%s-nw%g-k%d-h%d-f%d-%s-at%d" % (
        c.D, c.T, c.freq, "cplx" if c.cplx else "real", c.fmt, c.est, c.n, c.ovl, c.window, c.nw, c.kmax, c.history_mode, c.frames,
        c.scene, c.first)


CASES = [
    # every N once with `line` ...
    fft(1024, 1025, F1, 0, "s16", 256, 0.5, "hanning", 37, "line"),
    fft(16, 129, F2, 1, "f32", 512, 0.75, "kaiser", 37, "line"),
    mtm(64, 513, F1, 0, "s16", 1024, 0.0, 2.0, 0, 37, "line"),
    fft(100, 401, F2, 1, "s16", 2048, 0.3, "hanning", 7, "line"),
    mtm(16, 129, F1, 0, "f32", 4096, 0.5, 2.5, 3, 5, "line"),
    fft(3, 17, F1, 0, "f32", 8192, 0.5, "hanning", 5, "line"),
    fft(16, 129, F2, 0, "s16", 16384, 0.0, "kaiser", 3, "line"),
    fft(7, 8192, F1, 1, "f32", 256, 0.3, "hanning", 21, "line"),
    # ... and once with another scene
    fft(7, 8192, -0.49, 0, "s16", 256, 0.0, "rectangular", 21, "pair"),
    fft(1, 1, F1, 1, "u8", 512, 0.3, "rectangular", 37, "noise", 1),
    mtm(3, 17, F2, 0, "u8", 1024, 0.75, 2.5, 3, 37, "pair", 1),
    fft(5, 4, 0.0, 1, "s16", 2048, 0.0, "rectangular", 7, "noise"),
    mtm(64, 513, -0.49, 1, "f32", 4096, 0.3, 2.5, 4, 5, "pair", 1),
    fft(100, 401, F1, 1, "u8", 8192, 0.0, "kaiser", 5, "pair"),
    fft(1, 1, 0.0, 0, "f32", 16384, 0.75, "rectangular", 3, "noise"),
    mtm(5, 4, F2, 0, "u8", 16384, 0.5, 4.5, 8, 3, "pair"),
    fft(16, 129, F1, 1, "s16", 256, 0.75, "hanning", 37, "zero"),
    mtm(5, 4, -0.49, 0, "f32", 1024, 0.5, 2.5, 4, 37, "zero"),
    # the measured headline shape
    fft(64, 513, F1, 0, "f32", 16384, 0.5, "hanning", 3, "line"),
    # far into a stream: lo D passes 2^36, both stages on virtual bases
    fft(16, 129, F1, 0, "f32", 1024, 0.5, "hanning", 37, "line", 0, far_first(16, 1024, 0.5)),
    mtm(3, 17, F2, 1, "s16", 4096, 0.3, 2.0, 0, 5, "noise", 0, far_first(3, 4096, 0.3)),
]


# ---- geometry ---------------------------------------------------------------------------------------------------------------------
def hop(c):
    return hop_len(c.n, c.ovl)


def lo_hi(c):
    """The baseband samples [lo, hi) the frames read, as the entry computes them (lo clamped at 0)."""
    h = hop(c)
    return max(0, c.first * h - (c.n - h)), (c.first + c.frames) * h


def base_of(c):
    """Global index of the first input sample the piece holds."""
    lo, _ = lo_hi(c)
    return max(0, lo * c.D - (c.T - 1))


def nsamples_of(c):
    """Global length of the input stream."""
    return lo_hi(c)[1] * c.D + c.D // 2 + 1


def line_bin(c):
    return int(round(LINE_AT * c.n))


def lobe(c):
    """Half width, in bins, of what a line off a bin centre fills: the window's main lobe, or the tapers' band."""
    return int(np.ceil(c.nw)) + 1 if c.est == "mtm" else 3


def settled_frames(c):
    """The frames whose window lies wholly past the filter's start-up: its first sample m has m D >= T."""
    h = hop(c)
    start = lambda f: f * h if c.history_mode else max(0, f * h - (c.n - h))
    return [f - c.first for f in range(c.first, c.first + c.frames) if start(f) * c.D >= c.T]


# ---- input ------------------------------------------------------------------------------------------------------------------------
def seed_of(c):
    return 7 * c.D + 11 * c.T + c.n + 3 * c.frames + 13 * len(c.scene) + 1000 * c.cplx + 17 * DQ.FMTS.index(c.fmt) + 5 * c.kmax


def signal(c):
    count = nsamples_of(c) - base_of(c)
    rng = np.random.default_rng(seed_of(c))
    n = np.arange(count, dtype=np.float64) + float(base_of(c) % (1 << 20))      # (the tones' own phase origin is of no interest)
    cn = lambda s: s * (rng.standard_normal(count) + 1j * rng.standard_normal(count))
    tone = lambda a, f, ph: a * np.exp(2j * np.pi * f * n + 1j * ph)
    if c.scene == "line":
        z = tone(0.7, c.freq + 0.37, 0.3) + tone(0.7e-3, c.freq + LINE_AT / c.D, 1.1) + cn(0.7e-6)
    elif c.scene == "pair":
        z = tone(0.6, c.freq + LINE_AT / c.D, 0.4) + tone(0.6e-4, c.freq + PAIR_AT / c.D, 1.1) + cn(0.6e-5)
    elif c.scene == "noise":
        return 0.25 * rng.standard_normal(count) + 1j * (0.1 * rng.standard_normal(count) + 0.05)
    elif c.scene == "zero":
        return np.zeros(count, np.complex128)
    else:
        raise ValueError(c.scene)
    return z.real + 0.8j * z.imag


def make_input(c):
    """(raw, x): the piece in the case's format (complex: [S][2] pairs) and the complex64 values the device must see."""
    return DQ.convert(signal(c), c.cplx, c.fmt)


# ---- both stages on the CPU ---------------------------------------------------------------------------------------------------------
def exact_baseband(c, x, g, W):
    """The float64 outputs [lo, hi), X.exact in slices so that no [nout][T] matrix passes ~100 MB."""
    lo, hi = lo_hi(c)
    step = max(1, 4000000 // c.T)
    return np.concatenate([X.exact(x, g, W, c.D, a, min(step, hi - a), base_of(c))[0] for a in range(lo, hi, step)])


def frames_of(c, y):
    """The frames' samples laid end to end ([frames * N]) for a plan of hop N, or y itself: what the row functions take as a stream
    that starts at baseband sample 0.  A piece (first > 0) holds y[lo:hi) and none of its frames reaches back to sample 0."""
    if c.first == 0:
        return y, c.ovl, c.history_mode
    h = hop(c)
    assert lo_hi(c)[0] == c.first * h - (c.n - h) and len(y) == (c.frames - 1) * h + c.n
    fr = np.lib.stride_tricks.sliding_window_view(y, c.n)[::h].copy()
    if c.history_mode:
        fr[:, :c.n - h] = 0
    return fr.reshape(-1), 0.0, 0


def rows64(oracle, c, y):
    z, ovl, hm = frames_of(c, y)
    if c.est == "fft":
        return XC.periodogram64(z, c.n, ovl, K.window(oracle, c.n, c.window), hm)[:c.frames]
    v, sig = K.tapers(oracle, c.n, c.kmax, c.nw)
    return XC.multitaper64(z, c.n, ovl, v, sig, hm)[:c.frames]


def rows32(oracle, c, y, ntap=None):
    z, ovl, hm = frames_of(c, np.asarray(y, np.complex64))
    if c.est == "fft":
        return XC.periodogram32(z, c.n, ovl, K.window(oracle, c.n, c.window), hm)[:c.frames]
    v, sig = K.tapers(oracle, c.n, c.kmax, c.nw)
    return XC.multitaper32(z, c.n, ovl, v, sig, hm, ntap)[:c.frames]


def baseband32(c, r, **kw):
    """The float32 stand-in of the first stage on outputs [lo, hi); kw: X.standin32's order and wrong-variant switches."""
    lo, hi = lo_hi(c)
    return X.standin32(r.x, r.g, r.W, c.D, lo, hi - lo, base_of(c), **kw)


Ref = namedtuple("Ref", "raw x taps g W y exact f32 f32_rows tau_taps tau_rows tau_f32 tau")


@functools.lru_cache(maxsize=None)
def reference(oracle, c):
    """The input piece, taps and tables, the float64 baseband and rows, the rows of both float32 stand-ins composed (first stage summed
    in tap order and in the kernel's row order, then the float32 second stage), tau_f32 = the larger of their tau_of and the bound
    tau = 4 max(tau_f32, 2^-24) of tests/_rows_check.py."""
    raw, x = make_input(c)
    taps = X.design(c.D, c.T)
    W = X.phase_word(c.freq)
    g = X.tables(W, taps)
    y = exact_baseband(c, x, g, W)
    exact = rows64(oracle, c, y)
    part = Ref(raw, x, taps, g, W, y, exact, None, None, 0.0, 0.0, 0.0, 0.0)
    f32 = rows32(oracle, c, baseband32(c, part, order="taps"))
    f32_rows = rows32(oracle, c, baseband32(c, part, order="rows"))
    assert exact.shape == f32.shape == f32_rows.shape == (c.frames, c.n)
    t_taps, t_rows = tau_of(f32, exact), tau_of(f32_rows, exact)
    for a in (raw, x, taps, g, y, exact, f32, f32_rows):
        a.setflags(write=False)
    t32 = max(t_taps, t_rows)
    return Ref(raw, x, taps, g, W, y, exact, f32, f32_rows, t_taps, t_rows, t32, bound(t32))
