"""The case matrix of the digital down-converter (tests only), shared by tests/test_ddc_criterion.py (CPU) and tests/test_gpu_ddc.py.

A case is (D, T, freq, cplx, fmt, signal, nout, first): decimation, taps (the default design for D with T taps), the frequency moved
to 0 Hz, real or complex input, sample format, signal, outputs, and the global index of the first output (a piece of a long stream,
passed by its virtual base, when it is not 0).  The stream ends D/2 + 1 samples past the last whole output: a ragged tail.

Shapes, for where the kernel can go wrong: (1,1) the pure mixer; (1,33) one row, five tap blocks; (2,9), (3,17) odd D; (5,4) taps
shorter than the step (rows without a tap); (8,65) .. (64,513) the default designs, one to several row chunks; (100,401) D no power of
two; (1024,1025) the largest D, one row a chunk; (7,8192) the longest filter, 1171 taps a row.  (4,33) with 20 000 outputs spans
twenty tiles.

Signals (seeded):
  noise   Gaussian, sigma 0.25 (complex: 0.25 and 0.1 on I and Q, a DC level on Q)
  tone    0.6 at freq + 0.1 / D (inside the passband), noise 100 dB below
  weak    a 0.7 carrier at freq + 0.37 (out of band), a tone 80 dB below it at freq + 0.05 / D, noise 120 dB below
Integer formats: rounded to x * 20000 (s16) or x * 100 + 128 (u8); the reference sees the library's conversions of those integers.
"""
import functools
from collections import namedtuple

import numpy as np

import _ddc_exact as X

Case = namedtuple("Case", "D T freq cplx fmt signal nout first")

SHAPES = [(1, 1), (1, 33), (2, 9), (3, 17), (5, 4), (8, 65), (16, 129), (32, 257), (64, 513), (100, 401), (1024, 1025), (7, 8192)]
FREQS = [0.1234567, -0.49, 0.25 + 2.0 ** -40, 0.0]
FMTS = ["f32", "s16", "u8"]
SIGNALS = ["noise", "tone", "weak"]

# every shape once, formats, input kinds, frequencies and signals dealt round: each of the six instantiations twice
CASES = [Case(D, T, FREQS[i % 4], i % 2, FMTS[i % 3], SIGNALS[(i // 2) % 3], 40, 0) for i, (D, T) in enumerate(SHAPES)]
CASES += [
    Case(4, 33, 0.1234567, 0, "f32", "noise", 20000, 0),                   # many tiles
    Case(16, 129, 0.1234567, 0, "f32", "tone", 1500, 0),                   # a whole tile and a partial one
    Case(64, 513, 0.25 + 2.0 ** -40, 1, "s16", "weak", 40, 0),
    Case(2, 9, 0.0, 0, "u8", "tone", 40, 0),
    Case(16, 129, -0.49, 1, "f32", "noise", 40, 0),
    # the rule at a large sample index: pieces passed by their virtual base
    Case(16, 129, 0.1234567, 0, "f32", "tone", 40, (1 << 36) // 16),
    Case(3, 17, 0.25 + 2.0 ** -40, 1, "s16", "noise", 40, (1 << 36) // 3),
    Case(64, 513, -0.49, 0, "f32", "noise", 1100, (1 << 36) // 64 + 5),
]

# the criterion test's cases (CPU): non-zero frequencies, so that every wrong variant differs from the right output
CRITERION_SHAPES = [(2, 9), (8, 65), (32, 257), (100, 401)]


def case_id(c):
    return "D%d-T%d-f%.7g-%s-%s-%s-n%d-at%d" % (c.D, c.T, c.freq, "cplx" if c.cplx else "real", c.fmt, c.signal, c.nout, c.first)


def base_of(c):
    """Global index of the first sample the piece holds."""
    return max(0, c.first * c.D - (c.T - 1))


def nsamples_of(c):
    """Global length of the stream: the last output's samples and a ragged tail."""
    return (c.first + c.nout) * c.D + c.D // 2 + 1


def signal(c, seed):
    count = nsamples_of(c) - base_of(c)
    rng = np.random.default_rng(seed)
    n = np.arange(count, dtype=np.float64) + float(base_of(c) % (1 << 20))    # (the tones' own phase origin is of no interest)
    cn = lambda s: s * (rng.standard_normal(count) + 1j * rng.standard_normal(count))
    if c.signal == "noise":
        z = 0.25 * rng.standard_normal(count) + 1j * (0.1 * rng.standard_normal(count) + 0.05)
    elif c.signal == "tone":
        z = 0.6 * np.exp(2j * np.pi * (c.freq + 0.1 / c.D) * n + 0.4j) + cn(0.6e-5)
    elif c.signal == "weak":
        z = 0.7 * np.exp(2j * np.pi * (c.freq + 0.37) * n + 0.3j) + 0.7e-4 * np.exp(2j * np.pi * (c.freq + 0.05 / c.D) * n + 1.1j) + cn(0.7e-6)
    else:
        raise ValueError(c.signal)
    return z


def make_input(c, seed=None):
    """(raw, x): the piece in the case's format (complex: [S][2] pairs) and the complex64 values the device must see."""
    return convert(signal(c, seed_of(c) if seed is None else seed), c.cplx, c.fmt)


def convert(z, cplx, fmt):
    """make_input's clipping and conversion of the complex128 signal z (real input: its real part); tests/_zoom_cases.py shares it."""
    lim = np.nextafter(1.0, 0.0)
    parts = np.stack([np.clip(z.real, -1.0, lim), np.clip(z.imag, -1.0, lim)], axis=1)
    if not cplx:
        parts[:, 1] = 0.0
    if fmt == "s16":
        raw = np.clip(np.round(parts * 20000), -32768, 32767).astype(np.int16)
        v = raw.astype(np.float32) / np.float32(32768.0)
    elif fmt == "u8":
        raw = np.clip(np.round(parts * 100 + 128), 0, 255).astype(np.uint8)
        v = (raw.astype(np.float32) - np.float32(128.0)) / np.float32(128.0)
    else:
        raw = np.ascontiguousarray(parts.astype(np.float32))
        v = raw
    if not cplx:
        return np.ascontiguousarray(raw[:, 0]), v[:, 0].astype(np.complex64)
    return np.ascontiguousarray(raw), (v[:, 0] + 1j * v[:, 1]).astype(np.complex64)


def seed_of(c):
    return 7 * c.D + 11 * c.T + c.nout + 13 * len(c.signal) + 1000 * c.cplx + 17 * FMTS.index(c.fmt)


Ref = namedtuple("Ref", "raw x taps g W exact A f32 tau_f32 tau")


@functools.lru_cache(maxsize=None)
def reference(c):
    """Everything the CPU knows of a case, computed once: the input, taps and tables, the float64 outputs and amplitudes, the float32
    stand-in's outputs, tau_f32 and the bound tau = 4 max(tau_f32, 2^-24).  Nothing here comes from a device."""
    raw, x = make_input(c)
    taps = X.design(c.D, c.T)
    W = X.phase_word(c.freq)
    g = X.tables(W, taps)
    ex, A = X.exact(x, g, W, c.D, c.first, c.nout, base_of(c))
    f32 = X.standin32(x, g, W, c.D, c.first, c.nout, base_of(c))
    t32 = X.tau_of(f32, ex, A)
    for a in (raw, x, taps, g, ex, A, f32):
        a.setflags(write=False)
    return Ref(raw, x, taps, g, W, ex, A, f32, t32, X.bound(t32))
