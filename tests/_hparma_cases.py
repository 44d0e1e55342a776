"""The HP-ARMA case matrix (tests only), shared by tests/test_hparma_criterion.py (no device) and tests/test_gpu_hparma_rows.py.

A case is (n, t, p_e, ovl, frames, signal, fmt, sub_mean, history_mode, route).  sub_mean is what the REFERENCE does (0 / 1);
the GPU module asks the device for its mode 1 or 2.  route is how the plan is made and launched:
  default   the launcher's own choice
  generic   GLFER_HPARMA_GENERIC=1 (read per launch): the kernel that takes the shape from its parameters
  w16       GLFER_HPARMA_WIDTH=16 (read when the plan is made): sixteen rotations a step, each over 4 lanes
kernel_route() restates hparma.hip's choice of kernel and walk for the record:
  fixed<128,33> / fixed<96,17>   the shape as compile-time constants (BASELINE config 5, glfer's defaults)
  scheduled / scheduled-4lane    the static rotation schedule, shape from the parameters (t <= 128, a multiple of 4; <= 64 columns)
  fast-walk                      t <= 128, <= 64 columns, t no multiple of 4: rotation after rotation, a column pair in registers
  general-walk                   t > 128 (with the looped autocorrelation) or more than 64 columns

Signals: tests/_rows_cases.py's synth, weak, noise, impulse, bin, alt, lsb1, zero, and
  tone     a lone 0.6 tone off bin centre          tones3   three tones over noise of 1 % of the largest
  dc       a constant 0.25                         gap      synth with its third hop silent (frames are independent and come from a queue)
  square   a full-scale square wave of 14 samples a period: 16-bit samples +32767 / -32768
What the oracle makes of them (asserted by the criterion module): zero leaves nu a NaN and the rank at its initial 4 -- a NaN
row for p_e >= 5, a = e_0 for p_e <= 4; dc and alt have rank 0; noise, impulse (overlap 0) and lsb1 have rank p_e, a = e_0:
rows of N and 1 / N.

Pairings that are NOT in the matrix because the reference's own 1-ulp movement there exceeds the evaluation allowance
(tau_cond > tau_eval, tests/test_hparma_criterion.py): listed in DROPPED with their figures.
"""
import functools
from collections import namedtuple

import numpy as np

import _exact as X
import _hparma_check as H
import _rows_cases as K
from _signals import synth

Case = namedtuple("Case", "n t p_e ovl frames signal fmt sub_mean history_mode route")
DRAWS = 12
SEED = 0                  # the draws s_amp is taken from
HELD_OUT_SEED = 20251     # ... and the held-out ones of the criterion module
HELD_OUT_DRAWS = 4
INT_FMT = {"lsb1": "s16", "square": "s16"}


def hp(n, t, p_e, signal="synth", ovl=0.0, frames=5, fmt=None, sub_mean=0, history_mode=0, route="default"):
    return Case(n, t, p_e, ovl, frames, signal, fmt or INT_FMT.get(signal, "f32"), sub_mean, history_mode, route)


def case_id(c):
    return "n%d-t%d-p%d-o%g-f%d-%s-%s-m%d-h%d-%s" % c


def kernel_route(c):
    ncol = c.p_e + 1
    sched = 2 <= ncol <= 64
    if c.t > 128 or ncol > 64:
        return "general-walk" + ("+looped-autocorrelation" if c.t > 128 else "")
    if c.t % 4:
        return "fast-walk"
    if c.route == "w16":
        return "scheduled-4lane"
    if c.route == "default" and sched and (c.t, ncol) in ((128, 33), (96, 17)):
        return "fixed<%d,%d>" % (c.t, ncol)
    return "scheduled"


ROUTES = {"fixed<128,33>", "fixed<96,17>", "scheduled", "scheduled-4lane", "fast-walk", "general-walk", "general-walk+looped-autocorrelation"}

SIGNALS = ["synth", "weak", "tone", "bin", "tones3", "noise", "impulse", "alt", "dc", "lsb1", "zero", "gap", "square"]
WHITE = ["noise", "impulse", "alt", "dc", "lsb1", "zero"]  # rank p_e, rank 0 or NaN: the block size does not matter to these


def _at(t, p_e, sizes, **kw):
    """One case per signal of `sizes` (signal -> N) at the shape."""
    return [hp(n, t, p_e, s, **kw) for s, n in sizes.items()]


# The block size of a tonal pairing is the smallest of 512 ... 4096 at which the reference's own 1-ulp movement stays under the
# evaluation allowance (tau_cond <= tau_eval, asserted by tests/test_hparma_criterion.py): the autocorrelation averages N
# products, so a small block leaves the noise subspace loose.  DROPPED lists the pairings that miss it at every size.

# (a) every signal at the two fixed shapes
SIGNAL_CASES = (_at(128, 32, {"synth": 4096, "tones3": 4096, "gap": 4096, "square": 2048}) + [hp(512, 128, 32, s) for s in WHITE]
                + _at(96, 16, {"synth": 4096, "weak": 2048, "tone": 1024, "tones3": 1024, "gap": 4096, "square": 4096}) + [hp(1024, 96, 16, s) for s in WHITE])

# (b) every route: the two fixed shapes through the generic kernel, the 4-lane rotation, 64 columns, one and two steps a sweep,
#     partly filled row chunks, the non-scheduled fast walk, t > 128, more than 64 columns -- two tonal inputs and one input of
#     each degenerate kind (white: noise, or one impulse a frame where noise comes out at rank p_e - 1; rank 0; silence)
ROUTE_CASES = []
for _r in ("generic", "w16"):
    ROUTE_CASES += _at(128, 32, {"synth": 4096, "tones3": 4096, "noise": 512, "dc": 512, "zero": 512}, route=_r)
    ROUTE_CASES += _at(96, 16, {"tone": 1024, "tones3": 1024, "noise": 1024, "dc": 1024, "zero": 1024}, route=_r)
ROUTE_CASES += _at(128, 63, {"weak": 4096, "tone": 4096, "impulse": 1024, "alt": 1024, "dc": 1024, "zero": 1024})
ROUTE_CASES += _at(8, 1, {"synth": 32, "tones3": 32, "noise": 32, "dc": 32, "zero": 32})
ROUTE_CASES += _at(64, 2, {"synth": 64, "tones3": 64, "noise": 64, "alt": 64, "zero": 64})
ROUTE_CASES += _at(100, 40, {"synth": 4096, "square": 2048, "impulse": 512, "dc": 512, "zero": 512})
ROUTE_CASES += _at(124, 31, {"synth": 2048, "gap": 1024, "noise": 1024, "dc": 1024, "zero": 1024})
ROUTE_CASES += _at(66, 16, {"tone": 1024, "tones3": 1024, "noise": 1024, "dc": 1024, "zero": 1024})
ROUTE_CASES += _at(160, 12, {"square": 512, "synth": 4096, "bin": 512, "noise": 512, "dc": 512, "zero": 512})
ROUTE_CASES += _at(80, 64, {"weak": 1024, "bin": 1024, "impulse": 512, "dc": 512, "zero": 512})

# (c) the rank-stays-4 edge on both sides of prank < p_e, in every sample format
SILENCE_CASES = [hp(64, 16, 1, "zero"), hp(64, 16, 4, "zero"), hp(64, 16, 5, "zero"), hp(64, 16, 4, "zero", fmt="s16"), hp(64, 16, 5, "zero", fmt="u8")]

# (d) the block sizes beyond those: the largest two, and tonal rows at the smallest
SIZE_CASES = [hp(16384, 96, 16, "synth", frames=4), hp(32768, 128, 32, "tones3", frames=4), hp(32768, 128, 32, "noise", frames=4),
              hp(512, 16, 8, "synth"), hp(64, 16, 8, "alt"), hp(32, 16, 6, "dc", frames=8)]

# (e) options, each against the oracle: sample formats (some streams start an odd number of samples into their allocation),
#     overlaps (0.33 and 0.9: hops that are no sixteenth), zeroed history, mean removal
FORMAT_CASES = [hp(n, t, p, s, ovl=o, fmt=fmt) for fmt in ("s16", "u8") for n, t, p, s, o in
                ((4096, 128, 32, "synth", 0.0), (1024, 96, 16, "tones3", 0.5), (1024, 66, 16, "tones3", 0.0), (512, 160, 12, "square", 0.0),
                 (1024, 96, 16, "dc", 0.0), (512, 128, 32, "noise", 0.0))]
FORMAT_OFFSETS = {case_id(c): 3 for c in FORMAT_CASES if (c.fmt, c.t) in (("s16", 128), ("u8", 96), ("s16", 66), ("u8", 160))}
OVERLAP_CASES = [hp(1024, 96, 16, "tones3", ovl=o, frames=8) for o in (0.5, 0.75, 0.33)] + [hp(4096, 128, 32, "tones3", ovl=o, frames=8) for o in (0.5, 0.75, 0.9)]
HISTORY_CASES = [hp(1024, 96, 16, "tones3", ovl=0.5, frames=6, history_mode=1), hp(4096, 128, 32, "tones3", ovl=0.75, frames=8, history_mode=1),
                 hp(1024, 66, 16, "tones3", ovl=0.5, frames=6, history_mode=1), hp(512, 128, 32, "impulse", ovl=0.5, frames=6, history_mode=1)]
MEAN_CASES = [hp(1024, 96, 16, "tones3", ovl=0.5, frames=6, sub_mean=1), hp(4096, 128, 32, "synth", sub_mean=1, frames=4), hp(4096, 128, 32, "tones3", sub_mean=1),
              hp(512, 160, 12, "square", sub_mean=1, fmt="s16"), hp(1024, 96, 16, "tones3", ovl=0.75, frames=8, sub_mean=1, history_mode=1),
              hp(1024, 66, 16, "tone", sub_mean=1, fmt="u8")]
#     sub_mean = 2 (the in-kernel sums) gives the reference's rows on inputs whose hop means are small against the rms
MEAN2_CASES = [c for c in MEAN_CASES if c.signal in ("synth", "tones3", "tone")]
# (f) a launch that starts inside the stream and ends early (first frame; it ends 2 frames early); rows on a pitch
RANGE_CASES = [(hp(1024, 96, 16, "tones3", ovl=0.5, frames=12), 3), (hp(4096, 128, 32, "tones3", ovl=0.75, frames=12), 5),
               (hp(512, 160, 12, "square", frames=8, fmt="s16"), 1)]
PITCH_CASES = [(hp(1024, 96, 16, "tones3", frames=6), 528), (hp(4096, 128, 32, "gap", frames=6), 2064)]
# (g) placement: one batch and one ragged call (their rows are run()'s bit for bit, tests/test_gpu_hparma_batch.py); the
#     streams are these signals in turn
BATCH_SIGNALS = ["synth", "zero", "tones3", "noise", "dc"]
BATCH_CASE = hp(4096, 128, 32, "synth", frames=4)
RAGGED_SIGNALS = ["tones3", "zero", "tone", "noise", "dc"]
RAGGED_CASE = hp(1024, 96, 16, "tones3", ovl=0.5, frames=7)
RAGGED_HOPS = [7, 1, 4, 0, 6]                               # frames of stream b (every hop is a frame)

# Pairings that are left out, each at the block size where it comes closest: the criterion module shows that they still miss the
# condition (one that meets it belongs in the matrix).  Tonal inputs whose rank cut falls inside the noise floor (weak, tone, bin
# at 33 columns; bin at 17; synth at 64 columns and on 66 rows), noise where it comes out at rank p_e - 1 and the last direction
# alone is the noise subspace, and three tones on 160 rows.
DROPPED = [hp(4096, 128, 32, "weak"), hp(4096, 128, 32, "tone"), hp(4096, 128, 32, "bin"), hp(4096, 96, 16, "bin"), hp(4096, 128, 63, "synth"),
           hp(4096, 66, 16, "synth"), hp(4096, 160, 12, "tones3"), hp(1024, 128, 63, "noise"), hp(512, 100, 40, "noise"), hp(512, 80, 64, "noise")]
# ... and two whose finiteness pattern the reference does not keep under a 1-ulp perturbation, so that it is no property of the
# operation: dc on three columns (the zero of A at z = 1 is an exact float cancellation: inf or 1e16) and dc with mean removal
# (silence, a NaN row, only while every sample of a hop is the same float)
UNSTABLE = [hp(64, 64, 2, "dc"), hp(1024, 96, 16, "dc", sub_mean=1)]

_members = [BATCH_CASE._replace(signal=s, fmt=INT_FMT.get(s, "f32")) for s in BATCH_SIGNALS] + [RAGGED_CASE._replace(signal=s, fmt=INT_FMT.get(s, "f32"), frames=k)
                                                                                                  for s, k in zip(RAGGED_SIGNALS, RAGGED_HOPS) if k]
ALL_CASES = list(dict.fromkeys(SIGNAL_CASES + ROUTE_CASES + SILENCE_CASES + SIZE_CASES + FORMAT_CASES + OVERLAP_CASES + HISTORY_CASES + MEAN_CASES
                               + [c for c, _ in RANGE_CASES] + [c for c, _ in PITCH_CASES] + _members))


def seed_of(c):
    return c.n + 3 * c.t + 7 * c.p_e + c.frames + 13 * len(c.signal)


def signal(c, count, seed=None):
    """`count` float samples of the case's signal (before the conversion to its sample format)."""
    seed = seed_of(c) if seed is None else seed
    n, t = c.n, np.arange(count, dtype=np.float64)
    rng = np.random.default_rng(seed)
    h = X.hop_len(n, c.ovl)
    if c.signal == "tone":
        x = 0.6 * np.sin(2 * np.pi * (0.17 * n + 0.31) * t / n + 0.4)
    elif c.signal == "tones3":
        x = (0.5 * np.sin(2 * np.pi * (0.11 * n + 0.27) * t / n + 0.2) + 0.2 * np.sin(2 * np.pi * (0.23 * n + 0.41) * t / n + 1.3)
             + 0.1 * np.sin(2 * np.pi * (0.38 * n + 0.13) * t / n + 2.1) + 0.005 * rng.standard_normal(count))
    elif c.signal == "dc":
        x = np.full(count, 0.25)
    elif c.signal == "gap":
        x = synth(count, fs=8000.0, seed=seed).astype(np.float64)
        x[2 * h:3 * h] = 0.0
    elif c.signal == "square":
        x = np.where((np.arange(count) // 7) % 2 == 0, 1.0, -1.0)
    else:
        return K.signal(c, count, seed)
    return np.clip(x, -1.0, np.nextafter(1.0, 0.0)).astype(np.float32)


def make_input(oracle, c, seed=None):
    """(raw, xf): the samples in the case's format (whole hops and a few samples more) and the floats the reference sees."""
    h = X.hop_len(c.n, c.ovl)
    count = c.frames * h + min(3, h - 1)
    x = signal(c, count, seed)
    if c.fmt == "s16":
        if c.signal == "square":
            raw = np.where(x > 0, 32767, -32768).astype(np.int16)
        else:
            raw = np.clip(np.round(x.astype(np.float64) * 20000), -32768, 32767).astype(np.int16)
        return raw, oracle.pcm_s16_to_float(raw)
    if c.fmt == "u8":
        raw = np.clip(np.round(x.astype(np.float64) * 100 + 128), 0, 255).astype(np.uint8)
        return raw, oracle.pcm_u8_to_float(raw)
    assert c.fmt == "f32"
    return x, x


def frames_of(oracle, c):
    return lambda x: oracle.hparma_frames(x, c.n, c.ovl, c.t, c.p_e, sub_mean=c.sub_mean, history_mode=c.history_mode)


Ref = namedtuple("Ref", "raw xf want a rank exact tau_f32 tau_eval s_amp tau_cond tau s_peak old_bound oracle_frac")


def old_bound(c, s_peak):
    """_spread.hparma_bound's rule on the peak-normalised spread."""
    return 1e-5 if (c.n, c.t, c.p_e) == (4096, 128, 32) else max(1e-5, 3.0 * s_peak)


def reference_of(oracle, c, raw, xf):
    ref = frames_of(oracle, c)(xf)
    want, a, rank = np.stack([r[0] for r in ref]), np.stack([r[1] for r in ref]), np.array([r[2] for r in ref])
    assert want.shape == (c.frames, c.n // 2 + 1), (want.shape, c)
    t32, te = H.tau_eval(a, c.n)
    s_amp, s_peak = H.spread(frames_of(oracle, c), xf, ref, c.n, DRAWS, SEED)
    tc = H.COND * s_amp if np.isfinite(s_amp) else 0.0
    tau = te + tc
    return Ref(raw, xf, want, a, rank, H.q64(a, c.n), t32, te, s_amp, tc, tau, s_peak, old_bound(c, s_peak), H.fraction(want, a, c.n, tau))


@functools.lru_cache(maxsize=8)
def reference(oracle, c, seed=None):
    """Everything the CPU knows of a case: its samples, the oracle's rows, AR vectors and ranks, q64, the bound's parts, the older
    tests' spread and bound, and the fraction of the bound the oracle's own rows (through its float transform) use."""
    raw, xf = make_input(oracle, c, seed)
    return reference_of(oracle, c, raw, xf)
