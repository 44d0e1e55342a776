"""The harmonic F-test case matrix (tests only): one list per group of tests/test_gpu_ftest.py, shared with
tests/test_ftest_criterion.py, which runs the oracle against float64 arithmetic on every input of the matrix without a
GPU -- a case the reference alone cannot pass is found there, not on the device.

A case is (n, ovl, nw, kmax, frames, signal, fmt, sub_mean, history_mode).  The paired in-launch form transforms the
sequences [hn,] taper 0 .. kmax two at a time: kmax + 2 of them with mu live, kmax + 1 without, so every case meets an
even and an odd count between its live and its dead run, and N = 2048 ... 16384 have an even and an odd kmax each.
"""
import functools
from collections import namedtuple

import numpy as np

from _exact import ftest64, hop_len
from _signals import synth

Case = namedtuple("Case", "n ovl nw kmax frames signal fmt sub_mean history_mode")


def case(n, ovl, nw, kmax, frames, signal="synth", fmt="f32", sub_mean=0, history_mode=0):
    return Case(n, ovl, nw, kmax, frames, signal, fmt, sub_mean, history_mode)


def case_id(c):
    return "n%d-o%g-nw%g-k%d-f%d-%s-%s-m%d-h%d" % c


# (a), (b): every block size; overlaps 0, 0.5, 0.75 and a hop that is no sixteenth multiple; kmax from {2, 3, 4, 7, 8},
# nw from {2.0, 2.5, 4.0, 4.5}; small odd frame counts; at least one plain-noise input per size
SIZE_CASES = [
    case(8, 0.0, 2.0, 2, 33), case(8, 0.5, 2.0, 2, 35, "noise"),
    case(16, 0.5, 2.0, 3, 39, "noise"), case(16, 0.75, 2.5, 4, 37),     # (0.9 is a hop of ONE sample here: frame 0 has no strongest bin)
    case(32, 0.75, 2.5, 4, 37), case(32, 0.0, 4.0, 7, 31, "noise"),
    case(64, 0.9, 4.0, 7, 29, "noise"), case(64, 0.5, 2.0, 2, 27),
    case(128, 0.5, 4.5, 8, 21), case(128, 0.9, 2.5, 3, 23, "noise"),
    case(256, 0.75, 2.0, 2, 39), case(256, 0.0, 4.0, 7, 17, "noise"),
    case(512, 0.9, 2.5, 3, 25), case(512, 0.5, 4.5, 8, 19, "noise"),
    case(1024, 0.0, 2.5, 4, 13, "noise"), case(1024, 0.75, 4.0, 7, 23),
    case(2048, 0.5, 2.0, 2, 15), case(2048, 0.9, 2.5, 3, 21, "noise"),
    case(4096, 0.75, 4.0, 7, 11, "noise"), case(4096, 0.0, 4.5, 8, 7),
    case(8192, 0.9, 2.5, 4, 9), case(8192, 0.5, 4.0, 7, 7, "noise"),
    case(16384, 0.0, 2.0, 3, 5, "noise"), case(16384, 0.75, 4.5, 8, 9),
]

# (c): the two in-launch forms against each other
MUTUAL_CASES = [case(512, 0.75, 2.5, 4, 25), case(2048, 0.0, 4.0, 7, 9, "noise"), case(4096, 0.5, 2.5, 3, 11),
                case(16384, 0.5, 4.0, 7, 5, "noise")]

# (d): 16-bit and 8-bit samples (every in-launch size: each is an instantiation per format and form)
FORMAT_CASES = [case(n, ovl, nw, kmax, frames, signal, fmt)
                for fmt in ("s16", "u8")
                for n, ovl, nw, kmax, frames, signal in ((64, 0.5, 2.5, 3, 29, "synth"), (256, 0.75, 2.5, 4, 21, "noise"),
                                                         (512, 0.75, 4.0, 7, 19, "noise"), (1024, 0.9, 2.0, 2, 17, "synth"),
                                                         (2048, 0.0, 4.0, 7, 9, "noise"), (4096, 0.5, 2.5, 4, 9, "synth"),
                                                         (8192, 0.5, 2.5, 3, 7, "synth"), (16384, 0.0, 2.0, 2, 5, "synth"))]
# the stream starts this many samples into its allocation (an odd count: 16-bit samples off a 4-byte boundary)
FORMAT_OFFSETS = {case_id(c): 3 for c in FORMAT_CASES if (c.fmt, c.n) in (("s16", 1024), ("u8", 2048), ("s16", 8192), ("u8", 256))}

# (e): per-hop mean removal, in the reference's order (1) and with the tree sums (2); hops of 2, 4, 8, 16 sixteenths
# and overlap 0.9.  'dc': a DC level of the size of the signal's rms, the input on which the ORDER of a hop's sum
# shows in the rows (sub_mean = 1 only: include/glfer_hip.h defines mode 2 as the reference's rows only while a hop's
# mean is small against its rms, which holds for 'synth' and 'noise')
MEAN_CASES = [case(n, ovl, nw, kmax, frames, signal, "f32", m)
              for m in (1, 2)
              for n, ovl, nw, kmax, frames, signal in ((128, 0.875, 2.5, 4, 33, "synth"), (256, 0.75, 2.0, 3, 29, "noise"),
                                                       (256, 0.9, 2.5, 4, 27, "synth"), (1024, 0.5, 4.0, 7, 17, "synth"),
                                                       (2048, 0.0, 2.5, 4, 9, "noise"), (2048, 0.875, 2.0, 3, 25, "synth"),
                                                       (4096, 0.9, 4.0, 7, 15, "synth"), (4096, 0.5, 2.5, 4, 9, "noise"),
                                                       (16384, 0.75, 4.5, 8, 9, "synth"), (16384, 0.0, 2.0, 2, 5, "noise"))]
MEAN_CASES += [case(1024, 0.5, 2.5, 4, 17, "dc", "f32", 1), case(4096, 0.0, 2.5, 3, 7, "dc", "f32", 1),
               case(2048, 0.75, 4.0, 7, 13, "dc", "s16", 1)]

# (f): history zeroed in every frame; launches that start and end inside the stream (first_frame, with and without
# mean removal; the launch ends 3 frames before the stream does)
HISTORY_CASES = [case(64, 0.75, 2.5, 4, 29, "synth", "f32", 0, 1), case(1024, 0.5, 2.0, 3, 15, "noise", "f32", 0, 1),
                 case(4096, 0.75, 4.0, 7, 11, "synth", "f32", 1, 1), case(4096, 0.9, 2.5, 4, 9, "noise", "f32", 0, 1)]
RANGE_CASES = [(case(n, ovl, nw, kmax, frames, signal, "f32", m), first)
               for m in (0, 1)
               for n, ovl, nw, kmax, frames, signal, first in ((128, 0.5, 2.5, 4, 45, "synth", 1), (512, 0.75, 2.0, 3, 41, "noise", 5),
                                                               (2048, 0.75, 4.0, 7, 47, "synth", 32), (8192, 0.9, 2.5, 4, 49, "noise", 33))]

# (g): more frames than one pass of the grid holds, and no multiple of the frames per block.
#   N = 16: the epilogue route works in groups of at most 32 768 frames -> 40 001 frames, two groups.
#   N = 256 / 2048: launch16_fmt (spectro16.hip) starts at most 4 x resident blocks, resident = 256 CUs x (waves per
#   SIMD x 256 / block size) blocks = 256 x 3 at N = 256 and 256 x 2 at N = 2048 (blocks of 256 lanes: 16 and 2 frames
#   each) -> 3072 x 16 = 49 152 and 2048 x 2 = 4 096 frames in one pass; past that by the prime 1009.
LONG_CASES = [case(16, 0.0, 2.0, 3, 40001), case(256, 0.75, 2.5, 4, 4 * 256 * 3 * 16 + 1009), case(2048, 0.75, 2.5, 3, 4 * 256 * 2 * 2 + 1009)]

# (i): the plan after the call; the last one with cfg.psd_pitch = 2112
PLAN_CASES = [case(512, 0.5, 2.0, 2, 20, "synth", "f32", 1), case(2048, 0.5, 2.5, 4, 11), case(4096, 0.75, 4.0, 7, 9)]

ALL_CASES = SIZE_CASES + MUTUAL_CASES + FORMAT_CASES + MEAN_CASES + HISTORY_CASES + [c for c, _ in RANGE_CASES] + LONG_CASES + PLAN_CASES


def make_input(oracle, c):
    """(raw, xf): the samples in the case's format and the floats the reference sees (wav_fmt.c's conversions)."""
    h = hop_len(c.n, c.ovl)
    assert h >= 1
    count = c.frames * h + min(3, h - 1)                      # (a few samples past the last whole hop)
    seed = c.n + 7 * c.kmax + c.frames
    if c.signal == "noise":
        x = np.clip(0.25 * np.random.default_rng(seed).standard_normal(count), -1.0, np.nextafter(1.0, 0.0)).astype(np.float32)
    else:
        x = synth(count, fs=8000.0, seed=seed)
        if c.signal == "dc":                                  # rms of synth: sqrt(0.5^2/2 + 0.25^2/2 + 0.05^2) = 0.40
            x = np.clip(x + np.float32(0.4), -1.0, np.nextafter(1.0, 0.0)).astype(np.float32)
    if c.fmt == "s16":
        raw = np.clip(np.round(x * 20000), -32768, 32767).astype(np.int16)
        return raw, oracle.pcm_s16_to_float(raw)
    if c.fmt == "u8":
        raw = np.clip(np.round(x * 100 + 128), 0, 255).astype(np.uint8)
        return raw, oracle.pcm_u8_to_float(raw)
    assert c.fmt == "f32"
    return x, x


@functools.lru_cache(maxsize=64)
def _tapers(oracle, n, kmax, nw):
    return oracle.dpss(n, kmax, nw)[0]


@functools.lru_cache(maxsize=3)
def reference(oracle, c):
    """(raw, xf, want, num, den): the case's samples, as stored and as floats, the oracle's F rows (mu live) and the float64
    weights of the bound.
    The reference's mean removal is one thing (fft.c:86-96) whichever way the device is asked to take the sums."""
    raw, xf = make_input(oracle, c)
    m = 1 if c.sub_mean else 0
    _, want = oracle.spectrogram_mtm_ftest(xf, c.n, c.ovl, c.nw, c.kmax, sub_mean=m, history_mode=c.history_mode, mu_live=1)
    num, den, _ = ftest64(xf, c.n, c.ovl, _tapers(oracle, c.n, c.kmax, c.nw), c.kmax, sub_mean=m, history_mode=c.history_mode)
    assert want.shape == num.shape == (c.frames, c.n // 2 + 1)
    return raw, xf, want, num, den
