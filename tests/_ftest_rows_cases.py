"""The bin-by-bin case matrix of the harmonic F rows (tests only): one list per group of tests/test_gpu_ftest_rows.py, shared with
tests/test_ftest_rows_criterion.py, which runs the float32 stand-ins and the oracle against float64 arithmetic on every input of the
matrix without a GPU.

A case is tests/_ftest_cases.py's: (n, ovl, nw, kmax, frames, signal, fmt, sub_mean, history_mode); sub_mean is what the DEVICE is
asked for (1: the reference's order, 2: the in-kernel sums), the reference removes its means either way.  Signals, all seeded:

  line      a 0.6 carrier 0.37 of a bin above bin carrier_bin(n), a line LINE_DB[nw, kmax] dB under it 0.08 of a bin above bin
            line_bin(n), Gaussian noise 36 dB under the line: what the statistic is for.  The level is chosen per (nw, kmax) so that
            in every settled frame the line's F is at least 20 and the largest F outside the carrier's +-(ceil(nw) + 1) bins
            (line_conditions(), asserted on the CPU): the higher-order tapers leak, and a line 80 dB down is buried.  A line's
            distance from its bin caps its F whatever its level (0.21 of a bin: 18 ... 43), and below N = 1024 the carrier's
            leakage through the last tapers of kmax + 1 >= 2 nw buries a line 40 dB down: those sizes carry `line` under the well
            concentrated sets (nw, kmax) = (4.0, 2), (4.0, 3), (4.5, 4), (4.5, 5)
  line_on   the same with both tones on their bins: the carrier bin's den is what is left of a near-total cancellation
  line_dc   `line` plus a DC level of 0.3 (mean removal in the reference's order)
  gap       0.25 sigma noise with ceil(n / hop) hops of silence from hop 3 on: one whole frame without power between loud ones
  bin_lo, bin_hi, noise, impulse, alt, lsb1, zero: tests/_rows_cases.py::signal

N = 8 and N = 16 carry no `line`: at N = 8 the carrier's +-(ceil(2.0) + 1) covers all four bins below Nyquist; at N = 16 the two bins
left hold F64 < 1 at every level from 40 to 60 dB under nw = 2, and any wider taper set covers them too.
"""
import functools
from collections import namedtuple

import numpy as np

import _exact as X
import _rows_cases as R
from _ftest_rows_check import bound, tau_of_ftest

Case = namedtuple("Case", "n ovl nw kmax frames signal fmt sub_mean history_mode")


def case(n, ovl, nw, kmax, frames, signal="line", fmt="f32", sub_mean=0, history_mode=0):
    return Case(n, ovl, nw, kmax, frames, signal, fmt, sub_mean, history_mode)


def case_id(c):
    return "n%d-o%g-nw%g-k%d-f%d-%s-%s-m%d-h%d" % c


LINE_KINDS = ("line", "line_on", "line_dc")
CARRIER = 0.6
# dB under the carrier per taper set, taken from 50 / 40 by float64 measurement on the cases of the matrix that use the set (at 60 the
# line is buried under most of them); line_conditions() is asserted on every one of them by tests/test_ftest_rows_criterion.py
LINE_DB = {(2.0, 2): 50.0, (2.0, 3): 50.0, (2.5, 3): 40.0, (2.5, 4): 40.0, (4.0, 2): 50.0, (4.0, 3): 40.0, (4.0, 7): 50.0,
           (4.5, 4): 40.0, (4.5, 5): 40.0, (4.5, 8): 50.0}
NOISE_UNDER_LINE_DB = 36.0
OFFSETS = (0.37, 0.08)                           # of a bin: the carrier's and the line's distance from their bins


def carrier_bin(n):
    return max(1, int(round(0.12 * n)))


def line_bin(n):
    return int(round(0.40 * n))


def excluded(c):
    """The bins below Nyquist that belong to the carrier: +-(ceil(nw) + 1) around its bin."""
    k = np.arange(c.n // 2)
    return np.abs(k - carrier_bin(c.n)) <= int(np.ceil(c.nw)) + 1


def settled_frames(c):
    """The frames whose samples all come from the stream (none with the history zeroed in every frame at an overlap)."""
    h = X.hop_len(c.n, c.ovl)
    if h == c.n:
        return list(range(c.frames))
    if c.history_mode:
        return []
    return list(range(-(-(c.n - h) // h), c.frames))


def line_conditions(c, num, den, frames=None):
    """(the least F64 at the line's bin, whether that bin holds the largest F64 outside the carrier's bins) over the settled frames."""
    out = ~excluded(c)
    assert out[line_bin(c.n)]
    least, largest = np.inf, True
    for f in settled_frames(c) if frames is None else frames:
        F = num[f, :c.n // 2] / den[f, :c.n // 2]
        least = min(least, F[line_bin(c.n)])
        largest = largest and int(np.flatnonzero(out)[np.argmax(F[out])]) == line_bin(c.n)
    return float(least), bool(largest)


# (a) every size: `line` at every one from 32 on (two tapers sets, an even and an odd kmax, from 2048), `line_on` from 64 on, and
#     two or three of the other kinds; NW from {2.0, 2.5, 4.0, 4.5}; overlaps 0, 0.5, 0.75 and a hop that is no sixteenth (0.9)
SIZE_CASES = [
    case(8, 0.0, 2.0, 2, 33, "noise"), case(8, 0.5, 2.0, 2, 35, "impulse"), case(8, 0.0, 2.0, 2, 21, "bin_lo"), case(8, 0.5, 2.0, 2, 21, "zero"),
    case(16, 0.5, 2.0, 2, 39, "impulse"), case(16, 0.0, 2.0, 3, 37, "bin_hi"), case(16, 0.75, 2.5, 4, 37, "noise"), case(16, 0.0, 2.0, 2, 21, "alt"),
    case(32, 0.75, 4.0, 3, 37), case(32, 0.0, 2.5, 4, 31, "impulse"), case(32, 0.5, 4.0, 7, 31, "lsb1", "s16"),
    case(64, 0.5, 4.5, 4, 29), case(64, 0.0, 4.0, 3, 27, "line_on"), case(64, 0.0, 2.5, 3, 21, "bin_lo"), case(64, 0.75, 4.0, 7, 29, "gap"),
    case(128, 0.5, 4.0, 2, 21), case(128, 0.9, 4.5, 8, 23, "noise"), case(128, 0.0, 2.5, 3, 21, "alt"), case(128, 0.5, 2.5, 4, 21, "zero"),
    case(256, 0.75, 4.5, 5, 39), case(256, 0.0, 2.0, 2, 17, "line_on"), case(256, 0.0, 4.0, 7, 17, "bin_hi"), case(256, 0.5, 2.5, 3, 21, "impulse"),
    case(512, 0.5, 4.0, 3, 19), case(512, 0.0, 2.5, 4, 19, "line_on"), case(512, 0.9, 2.5, 3, 25, "noise"), case(512, 0.75, 2.0, 2, 21, "lsb1", "s16"),
    case(1024, 0.0, 4.0, 3, 13), case(1024, 0.75, 2.5, 4, 23, "line_on"), case(1024, 0.0, 2.0, 3, 13, "bin_lo"), case(1024, 0.5, 2.5, 4, 15, "gap"),
    case(1024, 0.0, 4.5, 8, 13, "alt"),
    case(2048, 0.5, 2.0, 2, 15), case(2048, 0.75, 2.5, 3, 21), case(2048, 0.0, 4.0, 7, 9, "line_on"), case(2048, 0.9, 2.5, 4, 21, "noise"),
    case(2048, 0.5, 4.5, 8, 11, "impulse"),
    case(4096, 0.75, 2.5, 4, 11), case(4096, 0.0, 4.0, 7, 7), case(4096, 0.5, 4.5, 8, 9, "line_on"), case(4096, 0.0, 2.5, 3, 7, "bin_hi"),
    case(4096, 0.5, 2.0, 2, 9, "zero"), case(4096, 0.75, 4.0, 7, 11, "gap"),
    case(8192, 0.5, 2.5, 4, 9), case(8192, 0.0, 4.0, 7, 7), case(8192, 0.75, 2.5, 3, 9, "line_on"), case(8192, 0.0, 4.5, 8, 5, "alt"),
    case(8192, 0.0, 2.0, 2, 5, "bin_lo"),
    case(16384, 0.75, 4.5, 8, 9), case(16384, 0.0, 2.0, 3, 5), case(16384, 0.5, 2.5, 4, 7, "line_on"), case(16384, 0.0, 4.0, 7, 5, "noise"),
    case(16384, 0.0, 2.5, 4, 5, "bin_hi"), case(16384, 0.5, 2.0, 2, 7, "lsb1", "s16"),
]

# (b) the epilogue route works in groups of at most 32 768 frames (N < 256): two groups at N = 16
LONG_CASES = [case(16, 0.0, 2.0, 2, 32768 + 1009, "noise")]

# (c) variations, each on `line` at a small size, at N = 2048 and at N = 16384
_SHAPES = ((128, 0.5, 4.5, 4, 29), (2048, 0.75, 2.5, 3, 21), (16384, 0.5, 4.0, 7, 7))
FORMAT_CASES = [case(*s, "line", fmt) for fmt in ("s16", "u8") for s in _SHAPES]
FORMAT_OFFSET = 3                                 # every one of them starts this many samples into its allocation
# mean removal: the reference's order (1) on `line` over a DC level; the in-kernel sums (2), which include/glfer_hip.h defines as
# the reference's rows only while a hop's mean is small against its rms, on `line` itself (R.mean2_condition, asserted)
# (the small size at overlap 0.75: with one or two hops a frame what is left around bin 0 is itself a clean line there, and its F,
# 10^3 ... 10^4 in float64, is larger than the weak line's)
_MEAN_SHAPES = ((128, 0.75, 4.5, 4, 29),) + _SHAPES[1:]
MEAN_CASES = [case(*s, "line_dc", "f32", 1) for s in _MEAN_SHAPES] + [case(*s, "line", "f32", 2) for s in _MEAN_SHAPES]
HISTORY_CASES = [case(*s, "line", "f32", 0, 1) for s in _SHAPES]
# launches that start and end inside the stream: (case, first frame); they end 3 frames before the stream does
RANGE_CASES = [(case(128, 0.5, 4.5, 4, 45), 1), (case(2048, 0.75, 2.5, 3, 47), 32), (case(16384, 0.5, 4.0, 7, 13), 3)]

# (d) the other entries: the rows-and-F entry, a batch of unlike streams of one length, a ragged call of unlike streams of unequal length
ROWS_FTEST_CASE = case(4096, 0.5, 2.5, 4, 9)
BATCH_CASE = case(2048, 0.5, 2.5, 3, 13)
BATCH_MEMBERS = [BATCH_CASE._replace(signal=s) for s in ("line", "zero", "noise")]
RAGGED_CASE = case(1024, 0.75, 4.5, 4, 23)
RAGGED_MEMBERS = [RAGGED_CASE._replace(signal=s, frames=f) for s, f in (("line", 23), ("zero", 5), ("noise", 14))]

ALL_CASES = list(dict.fromkeys(SIZE_CASES + LONG_CASES + FORMAT_CASES + MEAN_CASES + HISTORY_CASES + [c for c, _ in RANGE_CASES]
                               + [ROWS_FTEST_CASE] + BATCH_MEMBERS + RAGGED_MEMBERS))


def seed_of(c):
    return c.n + 7 * c.kmax + c.frames + 13 * len(c.signal)


def line_amplitude(c):
    return CARRIER * 10.0 ** (-LINE_DB[(c.nw, c.kmax)] / 20.0)


def signal(c, count, line_db=None):
    """`count` float samples of the case's signal (before the conversion to its sample format)."""
    n, h = c.n, X.hop_len(c.n, c.ovl)
    rng = np.random.default_rng(seed_of(c))
    t = np.arange(count, dtype=np.float64)
    if c.signal in LINE_KINDS:
        off = (0.0, 0.0) if c.signal == "line_on" else OFFSETS
        amp = line_amplitude(c) if line_db is None else CARRIER * 10.0 ** (-line_db / 20.0)
        x = (CARRIER * np.sin(2 * np.pi * (carrier_bin(n) + off[0]) * t / n + 0.3) + amp * np.sin(2 * np.pi * (line_bin(n) + off[1]) * t / n + 1.1)
             + amp * 10.0 ** (-NOISE_UNDER_LINE_DB / 20.0) * rng.standard_normal(count) + (0.3 if c.signal == "line_dc" else 0.0))
    elif c.signal == "gap":
        x = 0.25 * rng.standard_normal(count)
        x[3 * h:(3 - (-n // h)) * h] = 0.0
    else:
        return R.signal(c, count, seed_of(c))
    return np.clip(x, -1.0, np.nextafter(1.0, 0.0)).astype(np.float32)


def make_input(oracle, c, line_db=None):
    """(raw, xf): the samples in the case's format and the floats the reference sees (wav_fmt.c's conversions)."""
    h = X.hop_len(c.n, c.ovl)
    assert h >= 1
    x = signal(c, c.frames * h + min(3, h - 1), line_db)      # (a few samples past the last whole hop)
    if c.fmt == "s16":
        raw = np.clip(np.round(x.astype(np.float64) * 20000), -32768, 32767).astype(np.int16)
        return raw, oracle.pcm_s16_to_float(raw)
    if c.fmt == "u8":
        raw = np.clip(np.round(x.astype(np.float64) * 100 + 128), 0, 255).astype(np.uint8)
        return raw, oracle.pcm_u8_to_float(raw)
    assert c.fmt == "f32"
    return x, x


@functools.lru_cache(maxsize=64)
def tapers(oracle, n, kmax, nw):
    return oracle.dpss(n, kmax, nw)[0]


Ref = namedtuple("Ref", "raw xf want num den tot f32 tau_single tau_paired tau_f32 tau")


@functools.lru_cache(maxsize=4)
def reference(oracle, c):
    """Everything the CPU knows of a case: its samples, the oracle's F rows (mu live), the float64 parts, the float32 stand-in's rows,
    the rule solved for tau on the one-sequence-per-transform stand-in and on the paired one, tau_f32 and the bound
    tau = 4 max(tau_f32, 2^-24).  tau_f32 is the one-sequence stand-in's; the paired figure is recorded beside it."""
    raw, xf = make_input(oracle, c)
    m = 1 if c.sub_mean else 0
    v = tapers(oracle, c.n, c.kmax, c.nw)
    _, want = oracle.spectrogram_mtm_ftest(xf, c.n, c.ovl, c.nw, c.kmax, sub_mean=m, history_mode=c.history_mode, mu_live=1)
    num, den, tot = X.ftest64(xf, c.n, c.ovl, v, c.kmax, sub_mean=m, history_mode=c.history_mode)
    f32 = X.ftest32(xf, c.n, c.ovl, v, c.kmax, sub_mean=m, history_mode=c.history_mode)[0]
    assert want.shape == num.shape == f32.shape == (c.frames, c.n // 2 + 1)
    t1 = tau_of_ftest(f32, num, den, tot, c.kmax)
    t2 = tau_of_ftest(X.ftest32_paired(xf, c.n, c.ovl, v, c.kmax, sub_mean=m, history_mode=c.history_mode)[0], num, den, tot, c.kmax)
    return Ref(raw, xf, want, num, den, tot, f32, t1, t2, t1, bound(t1))
