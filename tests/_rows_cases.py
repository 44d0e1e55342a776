"""The bin-by-bin case matrix (tests only): one list per group of tests/test_gpu_rows.py, shared with
tests/test_rows_criterion.py, which runs the float32 stand-in and the oracle against float64 arithmetic on every input of
the matrix without a GPU -- a case the reference alone cannot pass is found there, not on the device.

A case is (est, n, ovl, window, nw, kmax, frames, signal, fmt, sub_mean, history_mode): est 'fft' (window: a name of
oracle.WINDOWS) or 'mtm' (nw, kmax; the window is rectangular).  sub_mean is what the REFERENCE does (0 / 1): the device is
asked for its mode 1 or 2 by the test.  How the rows are asked of the device (form, frame range, pitch, batch ...) is the
GPU module's business: the inputs and the float64 rows are the same.

Signals, all seeded:
  weak     a 0.7 tone off bin centre, a tone 80 dB below it elsewhere, noise 120 dB below it
  noise    0.25 sigma Gaussian;   synth: the suite's usual two tones over noise (tests/_signals.py)
  impulse  one sample of 0.5 per hop at a position that moves (overlap 0, rectangular: every bin of a row equal)
  bin      a 0.5 tone exactly on bin n/4 + 1 (rectangular window, overlap 0: every other bin is pure rounding);
  bin_lo / bin_hi: the same on bins 1 and n/2 - 1;   alt: +-0.5 alternating (all power at Nyquist)
  lsb1 / lsb2   integer streams of one / two LSBs of dither;   zero: digital silence
  keyed / keyed_noise / keyed_dc   (tests/_pairs_cases.py's, no case of this module uses them) 'weak' / 0.25 sigma noise times a level
                of KEY_LEVELS per hop; hops of 0.5 DC (exact, or over a 0.7e-6 sigma floor) among hops of 'weak'
  full / tiny   (tests/_nonlin_cases.py's, no case of this module uses them) a +-0.99 tone; a 0.7e-4 tone over 0.3e-4 sigma noise
"""
import functools
from collections import namedtuple

import numpy as np

import _exact as X
from _rows_check import bound, tau_of, tau_of_spectrum
from _signals import rel_err, synth

Case = namedtuple("Case", "est n ovl window nw kmax frames signal fmt sub_mean history_mode")
TOL = 1e-5


def fft(n, ovl, window, frames, signal="weak", fmt="f32", sub_mean=0, history_mode=0):
    return Case("fft", n, ovl, window, 0.0, 0, frames, signal, fmt, sub_mean, history_mode)


def mtm(n, ovl, nw, kmax, frames, signal="weak", fmt="f32", sub_mean=0, history_mode=0):
    return Case("mtm", n, ovl, "rectangular", nw, kmax, frames, signal, fmt, sub_mean, history_mode)


def case_id(c):
    return "%s-n%d-o%g-%s-nw%g-k%d-f%d-%s-%s-m%d-h%d" % c


WINDOW_NAMES = ["hanning", "blackman", "gaussian", "welch", "bartlett", "rectangular", "hamming", "kaiser"]


def _frames_for(n):
    return 21 if n <= 256 else 13 if n <= 2048 else 9 if n <= 16384 else 5 if n <= 65536 else 3


# (a) the periodogram at every block size: 'weak' at every one of them, plus one of noise / impulse / bin / synth;
#     overlaps 0, 0.5, 0.75, 0.875 and hops that are no sixteenth (0.9, 0.33)
_OVL = [0.5, 0.0, 0.75, 0.9, 0.875, 0.33]
_WIN = ["hanning", "kaiser", "blackman", "hamming"]
_SECOND = ["noise", "impulse", "bin", "synth"]
FFT_SIZE_CASES = []
for _i, _p in enumerate(range(3, 21)):
    _n = 1 << _p
    FFT_SIZE_CASES.append(fft(_n, _OVL[_i % 6], _WIN[_i % 4], _frames_for(_n), "weak"))
    _s = _SECOND[_i % 4]
    if _s in ("impulse", "bin"):
        FFT_SIZE_CASES.append(fft(_n, 0.0, "rectangular", _frames_for(_n), _s))
    else:
        FFT_SIZE_CASES.append(fft(_n, _OVL[(_i + 2) % 6], _WIN[(_i + 1) % 4], _frames_for(_n), _s))

# (b) all eight windows at one small, one middle, one large size
FFT_WINDOW_CASES = [fft(n, 0.5, w, _frames_for(n), "weak") for n in (64, 4096, 65536) for w in WINDOW_NAMES]

# (c) the multitaper at every block size, even and odd taper counts, NW in {2.0, 2.5, 4.0, 4.5}.  Five tapers at NW = 2.5, N = 4096
#     is the half-table form of spectro16y.hip; three and nine tapers there its full-table form; even counts stay packed.
#     Odd counts at N = 256 ... 2048 run spectro16xl.hip wherever the taper half tables fit the LDS (every count at 256 / 512,
#     up to 21 tapers at 1024): spectro16x.hip takes the two N = 1024 cases with 23 and 25 tapers
MTM_SIZE_CASES = [
    mtm(8, 0.0, 2.0, 2, 21), mtm(8, 0.5, 2.0, 2, 21, "noise"),
    mtm(16, 0.5, 2.0, 3, 21), mtm(16, 0.75, 2.5, 4, 21, "noise"),
    mtm(32, 0.75, 2.5, 4, 21), mtm(32, 0.0, 4.0, 7, 21, "impulse"),
    mtm(64, 0.9, 4.0, 7, 21), mtm(64, 0.5, 2.0, 2, 21, "noise"),
    mtm(128, 0.5, 4.5, 8, 21), mtm(128, 0.33, 2.5, 3, 21, "noise"),
    mtm(256, 0.75, 2.0, 2, 21), mtm(256, 0.0, 4.0, 7, 21, "noise"), mtm(256, 0.5, 2.5, 4, 37, "impulse"),
    mtm(512, 0.9, 2.5, 3, 13), mtm(512, 0.5, 4.5, 8, 25, "noise"),
    mtm(1024, 0.0, 2.5, 4, 23), mtm(1024, 0.75, 4.0, 7, 13, "noise"), mtm(1024, 0.875, 2.0, 2, 23, "synth"),
    mtm(1024, 0.5, 12.0, 22, 13), mtm(1024, 0.0, 14.0, 24, 11, "noise"),     # 23 / 25 tapers: their half tables do not fit the LDS -> spectro16x.hip
    mtm(2048, 0.5, 2.0, 2, 19), mtm(2048, 0.33, 2.5, 3, 13, "noise"), mtm(2048, 0.0, 4.5, 8, 21, "impulse"),
    mtm(4096, 0.0, 2.5, 4, 13), mtm(4096, 0.75, 2.5, 4, 15, "noise"), mtm(4096, 0.5, 2.0, 2, 11), mtm(4096, 0.75, 4.0, 7, 11, "noise"),
    mtm(4096, 0.0, 4.5, 8, 9), mtm(4096, 0.0, 2.5, 4, 9, "impulse"), mtm(4096, 0.0, 2.5, 4, 9, "bin"),
    mtm(8192, 0.9, 2.5, 4, 9), mtm(8192, 0.5, 4.0, 7, 7, "noise"),
    mtm(16384, 0.0, 4.5, 8, 7), mtm(16384, 0.75, 2.0, 3, 9, "noise"), mtm(16384, 0.5, 2.5, 4, 7, "synth"),
]

# (d) the periodogram's forms where a size has more than one (GLFER_FORM=h|w|x), and tones on the edge bins
FFT_FORM_CASES = [fft(512, 0.75, "hanning", 13), fft(2048, 0.5, "hanning", 13), fft(4096, 0.75, "kaiser", 11, "noise"),
                  fft(8192, 0.0, "hanning", 9), fft(16384, 0.5, "blackman", 7), fft(16384, 0.0, "rectangular", 5, "impulse")]
EDGE_CASES = [fft(n, 0.0, "rectangular", 5, s) for n in (16, 256, 1024, 4096, 32768, 262144) for s in ("bin_lo", "bin_hi", "alt")]
EDGE_CASES += [mtm(n, 0.0, 2.5, 4, 6, s) for n in (64, 512, 4096, 16384) for s in ("bin_lo", "bin_hi", "alt")]

# (e) history zeroed in every frame; launches that start and end inside the stream (first frame; they end 3 frames early)
HISTORY_CASES = [fft(64, 0.75, "hanning", 21, "weak", "f32", 0, 1), fft(1024, 0.5, "hanning", 15, "noise", "f32", 0, 1),
                 fft(4096, 0.875, "kaiser", 19, "weak", "f32", 1, 1), fft(65536, 0.5, "hanning", 5, "weak", "f32", 0, 1),
                 mtm(512, 0.75, 2.5, 4, 17, "weak", "f32", 0, 1), mtm(4096, 0.75, 2.5, 4, 11, "weak", "f32", 0, 1),
                 mtm(16384, 0.5, 4.5, 8, 7, "noise", "f32", 1, 1)]
RANGE_CASES = [(fft(128, 0.5, "hanning", 45), 1), (fft(1024, 0.75, "hanning", 41, "noise"), 5), (fft(4096, 0.75, "kaiser", 47), 2),
               (fft(32768, 0.5, "hanning", 11), 3), (mtm(256, 0.75, 2.5, 4, 75), 33), (mtm(1024, 0.5, 2.0, 2, 43, "noise"), 7),
               (mtm(4096, 0.0, 2.5, 4, 29), 11), (mtm(4096, 0.75, 2.5, 4, 47, "noise", "f32", 1), 32), (mtm(16384, 0.5, 4.5, 8, 13), 3)]

# (f) more frames than one pass of the grid (all frames checked).  spectro_small: groups of at most 32 768 frames (N = 16).
#     spectro16h.hip: the periodogram at N = 2048, 4 096 + 1 009 frames.  launch16_fmt (spectro16.hip) starts at most 4 x
#     resident blocks: 2048 x 2 = 4 096 frames at N = 2048 (four tapers: packed), 3072 x 16 = 49 152 at N = 256, where the
#     five-taper plan runs spectro16xl.hip in the same blocks.  spectro16y.hip: 16 384 frames a pass (checked on cuts of the
#     stream by the GPU module: the float64 rows of 20 000 frames are not kept whole).  Covered elsewhere, on 65 ... 71 units of
#     work (a grid of 64: persistent_grid keeps whole XCD slices) and at the launchers' own thresholds -- tests/_walk_cases.py,
#     tests/test_gpu_walk.py: spectro16h.hip's SHIFT = 2 / 4 / 8 forms (from work >= 4 x resident on), its multitaper form,
#     spectro16x.hip, spectro16xl.hip at N = 512 ... 2048, spectro16w.hip in every form, the packed kernel at N = 512 ... 8192, and
#     spectro_big.hip past subfft_kernel's grid cap and past its first scratch group (cuts); tests/test_gpu_round3.py keeps the
#     long launches of the large blocks against the oracle on a few rows
LONG_CASES = [fft(16, 0.0, "hanning", 40001, "noise"), fft(2048, 0.5, "hanning", 4096 + 1009, "noise"),
              mtm(256, 0.75, 2.5, 4, 49152 + 1009, "noise"), mtm(2048, 0.75, 2.0, 3, 4096 + 1009, "noise")]
LONG_Y = mtm(4096, 0.0, 2.5, 4, 16384 + 4097, "weak")
LONG_Y_CUTS = [(0, 24), (16384 - 12, 16384 + 36), (16384 + 4097 - 24, 16384 + 4097)]

# (g) 16-bit and 8-bit samples (some streams start an odd number of samples into their allocation), dither, silence
FORMAT_CASES = [c for fmt in ("s16", "u8") for c in (
    fft(64, 0.5, "hanning", 21, "weak", fmt), fft(512, 0.75, "hanning", 13, "noise", fmt), fft(4096, 0.75, "kaiser", 11, "weak", fmt),
    fft(16384, 0.0, "hanning", 7, "noise", fmt), fft(131072, 0.5, "hanning", 3, "weak", fmt),
    mtm(256, 0.5, 2.5, 4, 21, "weak", fmt), mtm(1024, 0.75, 2.0, 2, 13, "noise", fmt), mtm(4096, 0.0, 2.5, 4, 11, "weak", fmt),
    mtm(16384, 0.0, 4.5, 8, 7, "synth", fmt))]
FORMAT_OFFSETS = {case_id(c): 3 for c in FORMAT_CASES if (c.fmt, c.n) in (("s16", 512), ("u8", 4096), ("s16", 16384), ("u8", 256), ("s16", 131072))}
LSB_CASES = [fft(1024, 0.5, "hanning", 13, "lsb1", "s16"), fft(4096, 0.0, "kaiser", 9, "lsb2", "s16"), fft(256, 0.75, "hanning", 21, "lsb1", "u8"),
             fft(65536, 0.0, "hanning", 3, "lsb2", "u8"), mtm(4096, 0.0, 2.5, 4, 9, "lsb1", "s16"), mtm(512, 0.5, 2.0, 2, 13, "lsb2", "u8"),
             mtm(16384, 0.0, 4.5, 8, 5, "lsb1", "s16"),
             fft(1024, 0.5, "hanning", 9, "zero", "f32"), fft(4096, 0.75, "hanning", 9, "zero", "s16"), fft(64, 0.0, "hanning", 9, "zero", "u8"),
             mtm(4096, 0.0, 2.5, 4, 9, "zero", "s16"), mtm(1024, 0.5, 2.5, 4, 9, "zero", "f32"), fft(65536, 0.5, "hanning", 3, "zero", "f32")]

# (h) per-hop mean removal (the reference's, fft.c:86-96) on all kinds of input; the device takes it as sub_mean = 1 in its
#     table form and through the corrected copy.  MEAN2: the inputs whose hop means are small against the rms, where
#     include/glfer_hip.h gives sub_mean = 2 (the in-kernel sums) the reference's rows too
MEAN_CASES = [fft(128, 0.5, "hanning", 21, "weak", "f32", 1), fft(1024, 0.75, "hanning", 17, "noise", "f32", 1), fft(1024, 0.0, "rectangular", 9, "impulse", "f32", 1),
              fft(4096, 0.875, "hanning", 19, "weak", "f32", 1), fft(4096, 0.5, "kaiser", 11, "synth", "s16", 1), fft(4096, 0.0, "rectangular", 7, "bin", "f32", 1),
              fft(16384, 0.75, "blackman", 9, "noise", "f32", 1), fft(65536, 0.5, "hanning", 5, "weak", "f32", 1), fft(2048, 0.9, "hanning", 15, "lsb2", "u8", 1),
              mtm(256, 0.75, 2.0, 3, 29, "noise", "f32", 1), mtm(1024, 0.5, 4.0, 7, 17, "weak", "f32", 1), mtm(2048, 0.0, 2.5, 4, 9, "noise", "f32", 1),
              mtm(4096, 0.75, 2.5, 4, 15, "weak", "f32", 1), mtm(4096, 0.0, 2.5, 4, 9, "impulse", "f32", 1), mtm(4096, 0.5, 4.0, 7, 9, "synth", "u8", 1),
              mtm(16384, 0.0, 4.5, 8, 7, "weak", "f32", 1), mtm(16384, 0.5, 2.0, 2, 7, "noise", "s16", 1)]
#     (tones and tones over noise; plain noise only on hops of 2048 samples and more, where a hop's mean, rms / sqrt(hop) in
#     size, stays under the tenth of the rms that mean2_condition() asks for by more than four standard deviations)
MEAN2_CASES = [c for c in MEAN_CASES if c.fmt == "f32" and (c.signal in ("weak", "synth") or (c.signal == "noise" and X.hop_len(c.n, c.ovl) >= 2048))]


def mean2_condition(c, xf):
    """Every whole hop's mean at most a tenth of its rms."""
    h = X.hop_len(c.n, c.ovl)
    hops = np.asarray(xf[:len(xf) // h * h], np.float64).reshape(-1, h)
    return bool((np.abs(hops.mean(axis=1)) <= 0.1 * np.sqrt((hops ** 2).mean(axis=1))).all())

# (i) rows on a pitch, a batch of streams, halfcomplex spectra, the moving average inside the launch
PITCH_CASES = [(fft(4096, 0.75, "hanning", 11), 2112), (mtm(4096, 0.0, 2.5, 4, 11), 2112), (fft(1024, 0.5, "hanning", 13, "noise"), 528),
               (mtm(16384, 0.0, 4.5, 8, 5), 8208), (fft(64, 0.5, "hanning", 21), 48)]
BATCH_SIGNALS = ["weak", "synth", "noise", "synth", "impulse"]                    # stream 0, a middle one and the last are checked
BATCH_CASES = [fft(1024, 0.5, "hanning", 13), fft(4096, 0.75, "hanning", 11), mtm(4096, 0.0, 2.5, 4, 10), mtm(512, 0.5, 2.0, 3, 17),
               fft(64, 0.5, "kaiser", 21), mtm(16384, 0.0, 4.5, 8, 5)]
SPECTRUM_CASES = [fft(8, 0.5, "hanning", 21), fft(64, 0.0, "kaiser", 21, "noise"), fft(256, 0.75, "hanning", 21), fft(1024, 0.5, "blackman", 13, "noise"),
                  fft(4096, 0.0, "hanning", 9), fft(4096, 0.0, "rectangular", 9, "impulse"), fft(16384, 0.5, "hanning", 7), fft(32768, 0.0, "hanning", 5),
                  fft(2048, 0.0, "rectangular", 9, "alt")]
# the average is taken INSIDE the estimator launch (spectro16h.hip's AVG form; glfer_hip.cpp avg_in_launch) for the periodogram at
# N = 512 ... 4096, history from the stream, no mean removal or the reference's at a hop of 2 / 4 / 8 / 16 sixteenths, from frame
# b0 = ceil((N - H) / H) + depth - 1 on, when at least 256 frames follow b0; the frames before b0 and every other plan take
# the two launches.  The first six are in-launch cases (avg_in_launch_from() says from which frame), the last four are not
AVG_CASES = [fft(512, 0.0, "kaiser", 301), fft(1024, 0.5, "hanning", 331), fft(2048, 0.875, "hanning", 337, "noise", "f32", 1),
             fft(4096, 0.75, "hanning", 311, "weak", "f32", 1), fft(4096, 0.75, "hanning", 291, "noise"), fft(512, 0.5, "kaiser", 307, "weak", "s16"),
             fft(1024, 0.5, "hanning", 21), fft(4096, 0.9, "hanning", 300, "weak", "f32", 1), mtm(4096, 0.0, 2.5, 4, 13), fft(16384, 0.5, "hanning", 9)]
AVG_DEPTH = 4

_batch_members = [c._replace(signal=s) for c in BATCH_CASES for s in (BATCH_SIGNALS[0], BATCH_SIGNALS[2], BATCH_SIGNALS[4])]
ALL_CASES = list(dict.fromkeys(
    FFT_SIZE_CASES + FFT_WINDOW_CASES + MTM_SIZE_CASES + FFT_FORM_CASES + EDGE_CASES + HISTORY_CASES + [c for c, _ in RANGE_CASES]
    + LONG_CASES + [LONG_Y._replace(frames=b - a) for a, b in LONG_Y_CUTS] + FORMAT_CASES + LSB_CASES + MEAN_CASES
    + [c for c, _ in PITCH_CASES] + _batch_members + SPECTRUM_CASES + AVG_CASES))


def avg_in_launch_from(c, depth=AVG_DEPTH):
    """The first frame of a whole-stream run_avg call whose average is taken inside the estimator launch, or None where the
    whole call takes the two launches (glfer_hip.cpp avg_in_launch, restated for aligned streams)."""
    h = X.hop_len(c.n, c.ovl)
    b0 = -(-(c.n - h) // h) + depth - 1
    ok = c.est == "fft" and 512 <= c.n <= 4096 and not c.history_mode and depth <= 4 and b0 + 256 <= c.frames
    if c.sub_mean:
        ok = ok and (16 * h) % c.n == 0 and 16 * h // c.n in (2, 4, 8, 16)
    return b0 if ok else None


def seed_of(c):
    return c.n + 7 * c.kmax + c.frames + 13 * len(c.signal) + 1000 * WINDOW_NAMES.index(c.window)


KEY_LEVELS = (1.0, 1e-2, 1e-3, 1e-5, 1e-6, 0.0)


def key_runs(rng, nhops, span, levels):
    """One of `levels` per hop, drawn for runs of 1 ... 2 span hops (span: the hops of a frame): under overlap a frame holds
    onsets and releases, and a run of a frame's length and more leaves whole frames at one level -- digital silence among them."""
    out = []
    while len(out) < nhops:
        out += [levels[int(rng.integers(len(levels)))]] * int(rng.integers(1, 2 * span + 1))
    return np.asarray(out[:nhops], np.float64)


def signal(c, count, seed=None):
    """`count` float samples of the case's signal (before the conversion to its sample format)."""
    n = c.n
    rng = np.random.default_rng(seed_of(c) if seed is None else seed)
    t = np.arange(count, dtype=np.float64)
    h = X.hop_len(n, c.ovl)
    if c.signal == "weak":
        k0, k1 = 0.23 * n + 0.37, 0.37 * n + 0.21
        x = 0.7 * np.sin(2 * np.pi * k0 * t / n + 0.3) + 0.7e-4 * np.sin(2 * np.pi * k1 * t / n + 1.1) + 0.7e-6 * rng.standard_normal(count)
    elif c.signal in ("keyed", "keyed_noise", "keyed_dc"):    # (tests/_pairs_cases.py: a level per hop)
        weak = 0.7 * np.sin(2 * np.pi * (0.23 * n + 0.37) * t / n + 0.3) + 0.7e-4 * np.sin(2 * np.pi * (0.37 * n + 0.21) * t / n + 1.1) \
            + 0.7e-6 * rng.standard_normal(count)
        nhops = -(-count // h)
        if c.signal == "keyed_dc":
            kind = np.repeat(key_runs(rng, nhops, -(-n // h), (0.0, 1.0, 2.0)), h)[:count]
            x = np.where(kind == 0, weak, np.where(kind == 1, 0.5, 0.5 + 0.7e-6 * rng.standard_normal(count)))
        else:
            base = weak if c.signal == "keyed" else 0.25 * rng.standard_normal(count)
            x = base * np.repeat(key_runs(rng, nhops, -(-n // h), KEY_LEVELS), h)[:count]
    elif c.signal == "noise":
        x = 0.25 * rng.standard_normal(count)
    elif c.signal == "synth":
        return synth(count, fs=8000.0, seed=seed_of(c) if seed is None else seed)
    elif c.signal == "full":                                  # (tests/_nonlin_cases.py: RA9MB's 1/x regime)
        x = 0.99 * np.sin(2 * np.pi * (0.11 * n + 0.29) * t / n + 0.5)
    elif c.signal == "tiny":                                  # (tests/_nonlin_cases.py: RA9MB's x/a regime, the limiter's log near -10)
        x = 0.7e-4 * np.sin(2 * np.pi * (0.19 * n + 0.41) * t / n + 0.9) + 0.3e-4 * rng.standard_normal(count)
    elif c.signal == "impulse":
        x = np.zeros(count)
        for j in range(count // h):
            x[j * h + (7 * j + 3) % h] = 0.5
    elif c.signal in ("bin", "bin_lo", "bin_hi"):
        k = {"bin": n // 4 + 1, "bin_lo": 1, "bin_hi": n // 2 - 1}[c.signal]
        x = 0.5 * np.cos(2 * np.pi * ((k * t) % n) / n + 0.7)
    elif c.signal == "alt":
        x = 0.5 * (1.0 - 2.0 * (t % 2))
    elif c.signal in ("lsb1", "lsb2", "zero"):
        a = {"lsb1": 1, "lsb2": 2, "zero": 0}[c.signal]
        lsb = rng.integers(-a, a + 1, count).astype(np.float64)
        x = lsb / (20000.0 if c.fmt == "s16" else 100.0 if c.fmt == "u8" else 32768.0)
    else:
        raise ValueError(c.signal)
    return np.clip(x, -1.0, np.nextafter(1.0, 0.0)).astype(np.float32)


def make_input(oracle, c, seed=None):
    """(raw, xf): the samples in the case's format and the floats the reference sees (wav_fmt.c's conversions)."""
    h = X.hop_len(c.n, c.ovl)
    assert h >= 1
    count = c.frames * h + min(3, h - 1)                      # (a few samples past the last whole hop)
    x = signal(c, count, seed)
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
    return oracle.dpss(n, kmax, nw)


@functools.lru_cache(maxsize=64)
def window(oracle, n, name):
    """The window a frame is multiplied with: the plan's float32 table, and ones for 'rectangular', which the reference
    never applies (fft.c:139-148: the frame goes to the transform as it is; the multitaper's tapers carry the norm)."""
    if name == "rectangular":
        return np.ones(n, np.float32)
    return oracle.window(oracle.WINDOWS[name], n)


Ref = namedtuple("Ref", "raw xf exact f32 want tau_f32 tau tau_oracle e_ref")


def rows_of(oracle, c, xf, window32=None, taps=None):
    """(exact float64 rows, float32 stand-in rows, oracle rows) of the float stream xf under the case's estimator.  window32 /
    taps: the PLAN's own tables for the float64 rows (the GPU module passes them); the stand-in and the oracle use the oracle's."""
    m = 1 if c.sub_mean else 0
    if c.est == "fft":
        w = window(oracle, c.n, c.window)
        exact = X.periodogram64(xf, c.n, c.ovl, w if window32 is None else window32, m, c.history_mode)
        f32 = X.periodogram32(xf, c.n, c.ovl, w, m, c.history_mode)
        want = oracle.spectrogram_fft(xf, c.n, c.ovl, oracle.WINDOWS[c.window], sub_mean=m, history_mode=c.history_mode)
    else:
        v, sig = tapers(oracle, c.n, c.kmax, c.nw)
        ev, esig = (v, sig) if taps is None else taps
        exact = X.multitaper64(xf, c.n, c.ovl, ev, esig, m, c.history_mode)
        f32 = X.multitaper32(xf, c.n, c.ovl, v, sig, m, c.history_mode)
        want = oracle.spectrogram_mtm(xf, c.n, c.ovl, c.nw, c.kmax, sub_mean=m, history_mode=c.history_mode)
    assert exact.shape == f32.shape == want.shape == (c.frames, c.n // 2 + 1), (exact.shape, f32.shape, want.shape)
    return exact, f32, want


def peak_err(got, want):
    """The suite's peak-normalised figure: the worst frame's max(max-norm, 2-norm) error; a row of zeros must be met exactly."""
    worst = 0.0
    for f in range(len(want)):
        if np.asarray(want[f]).any():
            worst = max(worst, max(rel_err(got[f], want[f])))
        else:
            assert not np.asarray(got[f]).any(), "frame %d: the reference's row is 0 and this one is not" % f
    return worst


@functools.lru_cache(maxsize=4)
def reference(oracle, c, seed=None):
    """Everything the CPU knows of a case: its samples, the three kinds of rows, tau_f32, the bound tau = 4 max(tau_f32, 2^-24),
    the oracle's own tau and its peak-normalised distance from float64 (e_ref)."""
    raw, xf = make_input(oracle, c, seed)
    exact, f32, want = rows_of(oracle, c, xf)
    t32 = tau_of(f32, exact)
    return Ref(raw, xf, exact, f32, want, t32, bound(t32), tau_of(want, exact), peak_err(want, exact))


def oracle_bound(c, e_ref):
    """What device-against-oracle is held to per frame: the suite's 1e-5, and from N = 8192, where the reference's recurrence
    twiddles put it further than that from exact arithmetic, round 4's max(1e-5, 1.1 x err(oracle, exact))."""
    return TOL if c.n < 8192 else max(TOL, 1.1 * e_ref)


def spectrum_reference(oracle, c):
    """(raw, xf, exact_X, tau_f32, tau): the complex rule's parts for an 'fft' case."""
    assert c.est == "fft"
    raw, xf = make_input(oracle, c)
    w = window(oracle, c.n, c.window)
    m = 1 if c.sub_mean else 0
    exact_X = X.spectrum64(xf, c.n, c.ovl, w, m, c.history_mode)
    t32 = tau_of_spectrum(X.spectrum32(xf, c.n, c.ovl, w, m, c.history_mode), exact_X, c.n)
    return raw, xf, exact_X, t32, bound(t32)


def plain_average(rows, depth):
    """update_avg_plain (avg.c:108-159) over whole rows from an empty state, in float64: row f is the sum of the last
    min(f + 1, depth) rows over min(f + 1, depth) + 1 -- the reference's own divisor (effdepth + 1)."""
    rows = np.asarray(rows, np.float64)
    out = np.zeros_like(rows)
    for f in range(len(rows)):
        k = min(f + 1, depth)
        out[f] = rows[f + 1 - k:f + 1].sum(axis=0) / (k + 1)
    return out
