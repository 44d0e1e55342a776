"""The digital down-converter's definition in float64, and its plain float32 stand-in (tests only).

    W      = round(freq 2^64) mod 2^64                  phi(n) = (W n mod 2^64) / 2^64 turns      (Python integers: exact)
    g[t]   = h[t] exp(+2 pi i phi(t))                   product in double, each part rounded once to float32
    y[m]   = exp(-2 pi i phi(n0)) sum_t g[t] x[n0 - t]  n0 = (m + 1) D - 1,  x[n] = 0 for n < 0

`exact` takes the float tables and the phase word and does the rest in float64 / complex128.  `standin32` is the same case in
float32: a sequential sum over t = 0, 1, ... of complex64 products, then a rotation whose angle is accurate to double and rounded
to complex64.  Its switches build the WRONG outputs tests/test_ddc_criterion.py must see rejected.  `order` keeps the arithmetic and
changes the sequence of the sum alone: "taps" (t ascending, the default), "rows" (the order ddc.hip documents: t = r, r + D, r + 2D, ...
for r = 0 .. min(D, T) - 1, one accumulator throughout) and "down" (t descending, the order tests/test_zoom_criterion.py holds out).

A piece of a long stream: `x` holds samples [base, base + len(x)) and outputs [first, first + nout) are asked for; every sample they
read (n0 - t >= base, or below 0) must be in the piece.
"""
import math

import numpy as np

TWO64 = 1 << 64


def phase_word(freq):
    return round(freq * 2.0 ** 64) % TWO64


def turns(W, n):
    """phi(n) in [-1/2, 1/2) as the nearest double."""
    p = (W * n) % TWO64
    return (p - TWO64 if p >= TWO64 // 2 else p) / 2.0 ** 64


def tables(W, taps32):
    """g[t] as complex64, the restatement of glfer_hip_ddc_tables: libm's cos and sin of 2 pi phi(t) in double."""
    g = np.empty((len(taps32), 2), np.float32)
    for t, h in enumerate(np.asarray(taps32, np.float32)):
        ang = 2.0 * math.pi * turns(W, t)
        g[t, 0] = float(h) * math.cos(ang)                            # (part by part: a zero keeps its sign)
        g[t, 1] = float(h) * math.sin(ang)
    return g.view(np.complex64)[:, 0]


def design64(decim, ntaps=0, cutoff=0.0, beta=0.0):
    """The Kaiser-windowed sinc low-pass by numpy in float64, unit sum (the formula glfer_hip_ddc_design is held to)."""
    T = ntaps if ntaps > 0 else (1 if decim == 1 else min(8 * decim + 1, 8192))
    c = cutoff if cutoff > 0 else 0.4 / decim
    b = beta if beta > 0 else 8.0
    t = np.arange(T, dtype=np.float64)
    h = 2.0 * c * np.sinc(2.0 * c * (t - (T - 1) / 2.0)) * np.kaiser(T, b)
    return h / h.sum()


def design(decim, ntaps=0):
    return design64(decim, ntaps).astype(np.float32)


def windows(x, D, T, first, nout, base=0):
    """[nout][T]: row i holds x[n0 - t] over t for output first + i (zeros below sample 0)."""
    x = np.asarray(x)
    lo = (first + 1) * D - 1 - (T - 1)                               # the oldest sample read
    pad = 0
    if lo < base:
        assert base == 0, "a piece must hold every sample its outputs read"
        pad = -lo
        x = np.concatenate([np.zeros(pad, x.dtype), x])
    start = lo - base + pad
    need = start + (nout - 1) * D + T
    assert need <= len(x), (need, len(x))
    w = np.lib.stride_tricks.sliding_window_view(x, T)[start:start + (nout - 1) * D + 1:D]
    return w[:, ::-1]


def rotation(W, D, first, nout, at=0):
    """exp(-2 pi i phi(n0 + at)) per output, complex128."""
    ang = np.array([turns(W, (first + i + 1) * D - 1 + at) for i in range(nout)], np.float64)
    return np.exp(-2j * np.pi * ang)


def exact(x, g, W, D, first, nout, base=0):
    """(y complex128 [nout], A float64 [nout]), A[m] = sum_t |g[t]| |x[n0 - t]|."""
    g = np.asarray(g, np.complex64)
    w = windows(np.asarray(x, np.complex128), D, len(g), first, nout, base)
    g64 = g.astype(np.complex128)
    return (w @ g64) * rotation(W, D, first, nout), np.abs(w) @ np.abs(g64)


def tap_order(D, T, order="taps"):
    """The sequence in which the T products of one output are added."""
    if order == "taps":
        return list(range(T))
    if order == "rows":
        return [t for r in range(min(D, T)) for t in range(r, T, D)]
    if order == "down":
        return list(range(T - 1, -1, -1))
    raise ValueError(order)


def standin32(x, g, W, D, first, nout, base=0, conj_taps=False, delay=0, rot_at=0, reverse_taps=False, float_phase=None, order="taps"):
    """The float32 computation; the keyword switches make the wrong variants.  float_phase: a freq whose float32 product with
    float32(n0) replaces the integer phase.  order: the sequence of the sum (tap_order), no wrong variant."""
    g = np.asarray(g, np.complex64)
    if conj_taps:
        g = np.conj(g)
    if reverse_taps:
        g = g[::-1].copy()
    x = np.asarray(x, np.complex64)
    if delay:
        x = np.concatenate([np.zeros(delay, np.complex64), x[:-delay]])
    w = windows(x, D, len(g), first, nout, base)
    acc = np.zeros(nout, np.complex64)
    for t in tap_order(D, len(g), order):
        acc = acc + g[t] * w[:, t]
    if float_phase is None:
        rot = rotation(W, D, first, nout, rot_at)
    else:
        n0 = np.array([(first + i + 1) * D - 1 for i in range(nout)], np.float64).astype(np.float32)
        ph = np.float32(float_phase) * n0                                      # float32 product
        rot = np.exp(-2j * np.pi * (ph.astype(np.float64) % 1.0))
    return acc * rot.astype(np.complex64)


def tau_of(y, ex, A):
    """The largest |y - exact| / A over the outputs with A > 0 (inf for a non-finite value, or a non-zero one where A = 0)."""
    y = np.asarray(y, np.complex128)
    if not np.isfinite(y.view(np.float64)).all():
        return np.inf
    dead = A == 0
    if (y[dead] != 0).any():
        return np.inf
    if dead.all():
        return 0.0
    return float((np.abs(y[~dead] - ex[~dead]) / A[~dead]).max())


FLOOR, MARGIN = 2.0 ** -24, 4.0


def bound(tau_f32):
    return MARGIN * max(float(tau_f32), FLOOR)


def check(y, ex, A, tau, what=""):
    """Asserts |y[m] - exact[m]| <= tau A[m] for every output (A = 0: exactly zero); returns the largest fraction of the bound."""
    y = np.asarray(y, np.complex128)
    assert y.shape == ex.shape == A.shape, (what, y.shape, ex.shape)
    assert np.isfinite(y.view(np.float64)).all(), "%s: non-finite outputs" % what
    dead = A == 0
    assert not (y[dead] != 0).any(), "%s: an output with no input under its taps is not zero" % what
    if dead.all():
        return 0.0
    frac = np.zeros(len(A))
    frac[~dead] = np.abs(y[~dead] - ex[~dead]) / (tau * A[~dead])
    i = int(np.argmax(frac))
    assert frac[i] <= 1.0, "%s: output %d is %.3f of the bound (tau %.3e): got %r exact %r A %.6g" % (what, i, frac[i], tau, y[i], ex[i], A[i])
    return float(frac[i])
