"""The case matrix of the complex I/Q rows (tests only), shared by tests/test_iq_criterion.py (CPU) and tests/test_gpu_iq.py.

A case is (est, n, ovl, window, nw, kmax, frames, signal, fmt, history_mode): est 'fft' (window: a name of oracle.WINDOWS) or
'mtm' (nw, kmax).  Frame counts leave the last workgroup partly filled where a workgroup holds more than one frame (37 frames up
to N = 1024, 7 at N = 2048; from N = 4096 a workgroup is one frame).

Signals (complex, seeded; I and Q never alike):
  pos      one tone of 0.6 on a positive bin off centre, noise 100 dB below
  neg      the same on a negative bin
  weak     a 0.7 carrier on a positive bin, a tone 80 dB below it on a different NEGATIVE bin, noise 120 dB below it
  noise    Gaussian, sigma 0.25 on I and 0.1 on Q, a DC level of 0.05 on Q only
  crit     'weak' plus that noise at 1e-5 of its size: unequal I and Q powers, DC on Q only, one positive and one negative tone --
           the criterion test's signal, on which every wrong row it builds differs from the right one
  impulse  one complex sample (0.5 - 0.25 i) per hop at a position that moves
  zero     digital silence
Integer formats: the parts are rounded to x * 20000 (s16) or x * 100 + 128 (u8), and the reference sees the library's
conversions of those integers, x / 32768 and (x - 128) / 128.
"""
import functools
from collections import namedtuple

import numpy as np

import _iq_exact as XC
import _rows_cases as K
from _exact import hop_len
from _rows_check import bound, tau_of

Case = namedtuple("Case", "est n ovl window nw kmax frames signal fmt history_mode")


def fft(n, ovl, window, frames, signal, fmt="f32", history_mode=0):
    return Case("fft", n, ovl, window, 0.0, 0, frames, signal, fmt, history_mode)


def mtm(n, ovl, nw, kmax, frames, signal, fmt="f32", history_mode=0):
    return Case("mtm", n, ovl, "rectangular", nw, kmax, frames, signal, fmt, history_mode)


def case_id(c):
    return "%s-n%d-o%g-%s-nw%g-k%d-f%d-%s-%s-h%d" % c


# every N (a different compile, a different last-pass register-to-bin map) with a Hanning and a rectangular window; 1, 4 and 5
# tapers at N = 1024 and 4096, 9 at 16384; overlaps 0, 0.5, 0.75, 0.3; both history modes; the three formats; every signal
CASES = [
    fft(256, 0.5, "hanning", 37, "weak"), fft(256, 0.0, "rectangular", 37, "impulse", "s16"),
    fft(512, 0.75, "hanning", 37, "noise", "u8"), fft(512, 0.3, "rectangular", 37, "pos", "f32", 1),
    fft(1024, 0.3, "hanning", 37, "neg"), fft(1024, 0.5, "rectangular", 37, "noise", "s16", 1),
    mtm(1024, 0.0, 2.0, 0, 37, "weak"), mtm(1024, 0.5, 2.5, 3, 37, "noise"), mtm(1024, 0.75, 2.5, 4, 37, "pos", "u8"),
    fft(2048, 0.5, "hanning", 7, "weak", "s16"), fft(2048, 0.0, "rectangular", 7, "noise"),
    fft(4096, 0.75, "hanning", 7, "weak"), fft(4096, 0.0, "rectangular", 5, "impulse"),
    mtm(4096, 0.3, 2.0, 0, 6, "neg"), mtm(4096, 0.0, 2.5, 3, 5, "noise", "s16"), mtm(4096, 0.5, 2.5, 4, 7, "weak", "f32", 1),
    fft(8192, 0.3, "hanning", 5, "noise"), fft(8192, 0.5, "rectangular", 6, "pos", "u8"),
    fft(16384, 0.5, "hanning", 5, "weak"), fft(16384, 0.0, "rectangular", 5, "neg", "s16", 1),
    mtm(16384, 0.0, 4.5, 8, 5, "noise"),
    # more workgroups than one XCD slice rule keeps (67 -> a grid of 64): the persistent loop's second frame
    fft(4096, 0.75, "hanning", 67, "noise"),
    # the same where a workgroup holds several frames (16 and 4): 71 units of work on a grid of 64, the last frame group partly
    # filled (5 and 1 frames) and the second of its workgroup, so that the clamp runs in a later pass (tests/_grid_passes.py)
    fft(256, 0.5, "hanning", 1125, "noise"), mtm(1024, 0.75, 2.5, 4, 281, "weak", "s16"),
    # silence: exactly zero rows
    fft(1024, 0.5, "hanning", 9, "zero"), mtm(4096, 0.0, 2.5, 4, 5, "zero", "u8"), fft(256, 0.75, "hanning", 37, "zero", "s16"),
]

# the criterion test's cases (CPU): the rule accepts the stand-in and rejects the wrong rows on each
CRITERION_CASES = [fft(1024, 0.5, "hanning", 5, "crit"), mtm(1024, 0.5, 2.5, 4, 5, "crit"), mtm(4096, 0.0, 2.5, 4, 3, "crit"),
                   fft(16384, 0.5, "hanning", 3, "crit")]


def tone_bins(n):
    """The bins of 'weak' / 'crit': the carrier (positive) and the weak tone (negative), both off centre."""
    return 0.23 * n + 0.37, -(0.37 * n + 0.21)


def seed_of(c):
    return 7 * c.n + 11 * c.kmax + c.frames + 13 * len(c.signal) + 1000 * K.WINDOW_NAMES.index(c.window)


def signal(c, count):
    n = c.n
    rng = np.random.default_rng(seed_of(c))
    t = np.arange(count, dtype=np.float64)
    h = hop_len(n, c.ovl)
    cnoise = lambda s: s * (rng.standard_normal(count) + 1j * rng.standard_normal(count))
    kc, kw = tone_bins(n)
    if c.signal == "pos":
        z = 0.6 * np.exp(2j * np.pi * (0.11 * n + 0.29) * t / n + 0.4j) + cnoise(0.6e-5)
    elif c.signal == "neg":
        z = 0.6 * np.exp(-2j * np.pi * (0.31 * n + 0.43) * t / n + 0.9j) + cnoise(0.6e-5)
    elif c.signal in ("weak", "crit"):
        z = 0.7 * np.exp(2j * np.pi * kc * t / n + 0.3j) + 0.7e-4 * np.exp(2j * np.pi * kw * t / n + 1.1j) + cnoise(0.7e-6)
        if c.signal == "crit":
            z = z + 1e-5 * (0.25 * rng.standard_normal(count) + 1j * (0.1 * rng.standard_normal(count) + 0.05))
    elif c.signal == "noise":
        z = 0.25 * rng.standard_normal(count) + 1j * (0.1 * rng.standard_normal(count) + 0.05)
    elif c.signal == "impulse":
        z = np.zeros(count, np.complex128)
        for j in range(count // h):
            z[j * h + (7 * j + 3) % h] = 0.5 - 0.25j
    elif c.signal == "zero":
        z = np.zeros(count, np.complex128)
    else:
        raise ValueError(c.signal)
    lim = np.nextafter(1.0, 0.0)
    return (np.clip(z.real, -1.0, lim) + 1j * np.clip(z.imag, -1.0, lim)).astype(np.complex64)


def make_input(c):
    """(raw, z): the interleaved parts [S][2] in the case's format, and the complex64 samples the device must see."""
    h = hop_len(c.n, c.ovl)
    count = c.frames * h + min(3, h - 1)                       # (a few samples past the last whole hop)
    z = signal(c, count)
    parts = np.stack([z.real, z.imag], axis=1).astype(np.float64)
    if c.fmt == "s16":
        raw = np.clip(np.round(parts * 20000), -32768, 32767).astype(np.int16)
        v = raw.astype(np.float32) / np.float32(32768.0)
    elif c.fmt == "u8":
        raw = np.clip(np.round(parts * 100 + 128), 0, 255).astype(np.uint8)
        v = (raw.astype(np.float32) - np.float32(128.0)) / np.float32(128.0)
    else:
        assert c.fmt == "f32"
        raw = np.ascontiguousarray(parts.astype(np.float32))
        v = raw
    return raw, (v[:, 0] + 1j * v[:, 1]).astype(np.complex64)


def rows_of(oracle, c, z, ntap=None):
    """(exact float64 rows, float32 stand-in rows) of the complex stream z."""
    if c.est == "fft":
        w = K.window(oracle, c.n, c.window)
        return XC.periodogram64(z, c.n, c.ovl, w, c.history_mode), XC.periodogram32(z, c.n, c.ovl, w, c.history_mode)
    v, sig = K.tapers(oracle, c.n, c.kmax, c.nw)
    return XC.multitaper64(z, c.n, c.ovl, v, sig, c.history_mode), XC.multitaper32(z, c.n, c.ovl, v, sig, c.history_mode, ntap)


Ref = namedtuple("Ref", "raw z exact f32 tau_f32 tau")


@functools.lru_cache(maxsize=None)
def reference(oracle, c):
    """Everything the CPU knows of a case, computed once: its samples, the float64 rows, the stand-in's rows, tau_f32 and the
    bound tau = 4 max(tau_f32, 2^-24) (tests/_rows_check.py: rule and margin as for the real rows)."""
    raw, z = make_input(c)
    exact, f32 = rows_of(oracle, c, z)
    assert exact.shape == f32.shape == (c.frames, c.n)
    t32 = tau_of(f32, exact)
    return Ref(raw, z, exact, f32, t32, bound(t32))
