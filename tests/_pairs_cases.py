"""The keyed case matrix (tests only): multitaper rows of odd taper counts when the two frames that share a transform differ
in level.  Shared by tests/test_pairs_criterion.py (CPU: is a case adversarial, does the rule see the scales) and
tests/test_gpu_pairs.py (the device, bin by bin).  None of these cases is in tests/_rows_cases.py's ALL_CASES.

With an odd taper count spectro16x.hip, spectro16xl.hip and spectro16y.hip put the last taper of frames f and f + FPB into
one complex transform (odd_taper.hpp), FPB = 4096 / N.  WHICH frames pair is decided on the host (frame_cuts.h, restated in
device_pairs below): the groups of G = 2 FPB frames are aligned to the STREAM's frame indices, and only whole groups that
lie inside the call's range and past the stream's first ceil((N - H) / H) frames (zero history) reach those kernels -- the
frames in front of and behind them go to the packed kernel one by one.  So a call's first_frame moves the head and the tail,
not the grid; a frame never waits alone in a shared transform; and overlap costs a stream its first group(s).  Frame counts
are therefore the smallest of the table (two groups and an odd tail: 69 / 37 / 21 / 13 / 11 at N = 256 ... 4096) PLUS what
the census below needs in the body: four pairs in each order cannot come out of the 3 ... 8 pairs those counts leave.
issue_pairs is the other reading of the grid -- blocks counted from the call's first frame, a lone frame at the end -- kept
because a kernel that counted so would be held to the same conditions.

Signals (tests/_rows_cases.py signal()): keyed, keyed_noise, keyed_dc -- 'weak', 0.25 sigma noise times a level of
{1, 1e-2, 1e-3, 1e-5, 1e-6, 0} per hop, held for runs of 1 ... 2 frames' hops; keyed_dc (reference mean removal only): hops of
0.5 DC among hops of 'weak'.  The float sum of H halves is exact, so such a hop leaves the reference's mean removal as exact
zeros -- whole-DC frames are silent frames beside loud partners --; a second kind of DC run carries 'weak's own 0.7e-6 sigma floor
on the 0.5, and leaves it as that floor quantised to the float32 steps at 0.5: rounding residue beside a loud partner.
Seeds are per (case, slot) in SEEDS: found by tests/test_pairs_criterion.py's conditions (census + the three stand-in
figures), never by looking at device output; find_seed() is the search that made them.
"""
import functools
from collections import namedtuple

import numpy as np

import _exact as X
import _rows_cases as K
from _rows_check import bound, tau_of

mtm, case_id = K.mtm, K.case_id
RATIO = 1e6                      # partners' row powers at least this far apart
MIN_EACH_ORDER = 4


def fpb(n):
    assert 256 <= n <= 4096
    return 4096 // n


def first_inside(c):
    h = X.hop_len(c.n, c.ovl)
    return -(-(c.n - h) // h)


def shares_transforms(c):
    """Odd taper counts >= 3 at N = 256 ... 4096 (glfer_hip.cpp body_route: every such plan of this matrix)."""
    return c.est == "mtm" and c.kmax >= 2 and c.kmax % 2 == 0


def device_pairs(c, lo, hi):
    """(pairs, lone) of a call for frames [lo, hi) of a stream as frame_cuts.h cuts it: lone is always empty."""
    if not shares_transforms(c):
        return [], []
    g = fpb(c.n)
    G = 2 * g
    b0 = -(-max(lo, first_inside(c)) // G) * G
    b1 = hi // G * G
    return [(f, f + g) for f in range(b0, b1) if f % G < g], []


def issue_pairs(c, origin, hi):
    """(pairs, lone) with blocks of 2 FPB frames counted from `origin`: a frame whose partner lies past the end is lone."""
    g = fpb(c.n)
    first = [f for f in range(origin, hi) if (f - origin) % (2 * g) < g]
    return [(f, f + g) for f in first if f + g < hi], [f for f in first if f + g >= hi]


Census = namedtuple("Census", "pairs loud_first quiet_first silent_loud loud_silent live_loud_first live_quiet_first lone")


def census(power, pairs, lone):
    """power: the float64 row sums.  loud_first: pairs (A, B) with P_B <= P_A / RATIO (a silent B counts); live_*: both > 0."""
    lf = [(a, b) for a, b in pairs if power[a] > 0 and power[b] * RATIO <= power[a]]
    qf = [(a, b) for a, b in pairs if power[b] > 0 and power[a] * RATIO <= power[b]]
    return Census(len(pairs), len(lf), len(qf), sum(power[a] == 0 for a, b in qf), sum(power[b] == 0 for a, b in lf),
                  sum(power[b] > 0 for a, b in lf), sum(power[a] > 0 for a, b in qf), len(lone))


def adversarial(cs, need_lone):
    return (cs.loud_first >= MIN_EACH_ORDER and cs.quiet_first >= MIN_EACH_ORDER and cs.silent_loud >= 1 and cs.loud_silent >= 1
            and (cs.lone >= 1 or not need_lone))


# ---- the cases -----------------------------------------------------------------------------------------------------------
_BASE = {256: 69, 512: 37, 1024: 37, 2048: 29, 4096: 87}        # the table's counts; N >= 1024: more pairs for the census


def frames_of(n, ovl, more=1):
    """The base count -- times the frames' lengths that partners FPB hops apart share, where they overlap: such partners differ
    10^6 in power only where a run of the keying ends -- behind the groups that overlap keeps from the shared transforms."""
    G = 2 * fpb(n)
    h = X.hop_len(n, ovl)
    frames = -(-(-(-(n - h) // h)) // G) * G + _BASE[n] * min(4, max(1, -(-n // (fpb(n) * h)))) * more
    return frames + (frames % G == 0)                       # (never whole groups only: the last block is a partial one)


def _k(n, ovl, nw, kmax, signal="keyed", fmt="f32", sub_mean=0, history_mode=0, more=1):
    return mtm(n, ovl, nw, kmax, frames_of(n, ovl, more), signal, fmt, sub_mean, history_mode)


# 3 / 5 / 7 / 9 tapers over the overlaps 0, 0.5, 0.75 and 0.9 at every size; 23 tapers at N = 1024 (spectro16x.hip); at N = 4096
# five tapers NW 2.5 (spectro16y.hip's half-table form: the queue) and 3 / 9 tapers (its full-table form).  N = 256 ... 2048:
# spectro16xl.hip
SIZE_CASES = [
    _k(256, 0.0, 2.0, 2), _k(256, 0.5, 2.5, 4, "keyed_noise"), _k(256, 0.75, 4.0, 6), _k(256, 0.9, 4.5, 8, "keyed_noise"),
    _k(512, 0.75, 2.0, 2, "keyed_noise"), _k(512, 0.0, 2.5, 4), _k(512, 0.9, 4.0, 6), _k(512, 0.5, 4.5, 8, "keyed_noise"),
    _k(1024, 0.5, 2.0, 2), _k(1024, 0.75, 2.5, 4, "keyed_noise"), _k(1024, 0.0, 4.0, 6, "keyed_noise"), _k(1024, 0.9, 4.5, 8),
    _k(1024, 0.5, 12.0, 22),
    _k(2048, 0.0, 2.0, 2, "keyed_noise"), _k(2048, 0.9, 2.5, 4), _k(2048, 0.5, 4.0, 6), _k(2048, 0.75, 4.5, 8, "keyed_noise"),
    _k(4096, 0.0, 2.5, 4), _k(4096, 0.75, 2.5, 4, "keyed_noise"), _k(4096, 0.5, 2.0, 2), _k(4096, 0.9, 4.5, 8, "keyed_noise"),
    _k(4096, 0.75, 4.5, 8),
]
# even taper counts never share a transform: the same inputs through the packed kernel
CONTROL_CASES = [_k(1024, 0.5, 2.0, 3), _k(4096, 0.75, 2.5, 3, "keyed_noise")]

# run(first_frame = a, nframes = frames - a - 1), a in {1, FPB - 1, FPB, FPB + 1}
RANGE_CASES = [_k(256, 0.5, 2.5, 4, more=2), _k(512, 0.0, 2.5, 4, "keyed_noise", more=2), _k(1024, 0.75, 2.0, 2, more=2),
               _k(2048, 0.5, 2.5, 4, more=2), _k(4096, 0.0, 2.5, 4, "keyed_noise", more=2), _k(4096, 0.75, 4.5, 8, more=2)]


def range_firsts(c):
    g = fpb(c.n)
    return sorted({a for a in (1, g - 1, g, g + 1) if a >= 1})


def range_of(c, first):
    """[first, hi): the call ends one or two frames early, on a partial block of the grid counted from `first`."""
    hi = c.frames - 1
    return first, hi - ((hi - first) % (2 * fpb(c.n)) == 0)


# three keyed streams (slots 0, 1, 2) and digital silence in one batch
BATCH_CASES = [_k(512, 0.5, 2.5, 4), _k(4096, 0.0, 2.5, 4), _k(4096, 0.75, 2.0, 2, "keyed_noise")]
BATCH_SLOTS = 3

# streams of 0, 1, 2, FPB, 2 FPB + 1 and 4 FPB + 3 frames, hop = frame, loud ('keyed') and quiet (1e-5 x 'weak') by turns
RAGGED_CASES = [mtm(1024, 0.0, 2.5, 4, 0, "keyed"), mtm(4096, 0.0, 2.5, 4, 0, "keyed"), mtm(4096, 0.0, 4.5, 8, 0, "keyed")]
RAGGED_QUIET = 1e-5


def ragged_frames(n):
    """The six lengths in a fixed shuffled order: streams at odd places are the quiet ones, so the longest (two groups and more)
    is quiet between the loud streams of 1 and 2 FPB + 1 frames -- quiet and loud bodies share a launch of the sharing kernel at
    N = 1024 (G = 8) as at N = 4096."""
    g = fpb(n)
    return [1, 4 * g + 3, 2 * g + 1, 0, 2, g]


def ragged_streams(oracle, c):
    """[(samples float32, frames)] in buffer order; a stream of 0 frames is N - 1 samples."""
    out = []
    for i, fr in enumerate(ragged_frames(c.n)):
        m = c._replace(frames=max(fr, 1), signal="keyed" if i % 2 == 0 else "weak")
        x = K.signal(m, max(fr, 1) * c.n, seed=9000 + 31 * c.n + i)
        if i % 2:
            x = (x.astype(np.float64) * RAGGED_QUIET).astype(np.float32)
        elif fr:                                            # (a loud stream ends at full level, whatever its keying)
            x[-c.n:] = K.signal(m._replace(signal="weak"), fr * c.n, seed=9000 + 31 * c.n + i)[-c.n:]
        out.append((x[:fr * c.n] if fr else x[:c.n - 1], fr))
    return out


# mean removal in the reference's order (the device's sub_mean = 1), in the default form and under GLFER_MEAN_PREPASS=1
MEAN_CASES = [_k(1024, 0.5, 2.5, 4, "keyed_dc", "f32", 1), _k(1024, 0.75, 2.0, 2, "keyed", "f32", 1),
              _k(4096, 0.75, 2.5, 4, "keyed_dc", "f32", 1), _k(4096, 0.5, 2.5, 4, "keyed", "f32", 1)]
HISTORY_CASES = [_k(512, 0.75, 2.5, 4, "keyed", "f32", 0, 1), _k(4096, 0.75, 2.5, 4, "keyed_noise", "f32", 0, 1)]
FORMAT_CASES = [_k(256, 0.5, 2.5, 4, "keyed", "s16"), _k(2048, 0.0, 2.0, 2, "keyed_noise", "s16"), _k(4096, 0.75, 2.5, 4, "keyed", "s16"),
                _k(256, 0.75, 2.0, 2, "keyed_noise", "u8")]
# u8 at N = 2048 and 4096 are PLAIN cases: not in CHECKED.  Eight bits hold two live levels of the keying (1 and 1e-2: 70 LSB and
# 1 LSB; the rest is digital silence), 10^4 apart in power, and at these sizes the stand-in with both scales 1 stays within
# 0.6 ... 4.0 times the bound over 300 seeds each of keyed / keyed_noise at overlap 0 and 0.5: condition 3's 4x cannot be met, the
# rule's tau cannot tell a missing scale there.  What they still show under unequal partners: the u8 conversion on
# spectro16xl.hip / spectro16y.hip, and silence beside a loud partner -- with the scales 1 the silent-row rule fails (asserted on
# the CPU), whatever tau.
FORMAT_PLAIN_CASES = [_k(2048, 0.5, 2.5, 4, "keyed", "u8"), _k(4096, 0.0, 2.5, 4, "keyed", "u8")]
FORMAT_OFFSETS = {case_id(c): 3 for c in FORMAT_CASES + FORMAT_PLAIN_CASES if (c.fmt, c.n) in (("s16", 2048), ("u8", 256), ("u8", 4096))}


# long launches, judged on cuts.  N = 4096, five tapers: spectro16y.hip's queue, whose static first chunks end at frame 4 096 --
# the cuts round 16 384 and at the end lie in ticketed chunks.  N = 256, five tapers: spectro16xl.hip's workgroups take G = 32
# frames an iteration on a grid of at most 2 048 workgroups (xl_second_pass_from restates its launcher): the second iteration
# starts 65 536 frames into the body
def xl_second_pass_from(c):
    """The stream frame at which spectro16xl.hip's workgroups start their second iteration in a whole-stream call
    (launch16xl_fmt: grid = persistent_grid(ceil(body / G), 4 x 512), whole XCD slices from 64 up; a workgroup's next block is
    grid x G frames on), or None where one iteration covers the body."""
    G = 2 * fpb(c.n)
    b0 = -(-first_inside(c) // G) * G
    work = (c.frames // G * G - b0) // G
    grid = min(work, 2048)
    grid = grid & ~7 if grid >= 64 else grid
    return b0 + grid * G if grid < work else None


LONG_Y = mtm(4096, 0.0, 2.5, 4, 16384 + 4097, "keyed")
LONG_XL = mtm(256, 0.75, 2.5, 4, 32 + 65536 + 1009, "keyed_noise")
LONG_CASES = [(LONG_Y, 16384), (LONG_XL, xl_second_pass_from(LONG_XL))]
LONG_MIN_PAIRS = 8                                           # a cut with this many pairs holds one 10^6 apart in each order


def long_cuts(c, seam):
    """The first 24 frames, 48 round the seam, the last 24 -- each widened to the partners of its frames in the whole-stream
    call, so that a pair is judged whole."""
    pairs = lambda a, b: [p for p in device_pairs(c, max(a - 2 * fpb(c.n), 0), min(b + 2 * fpb(c.n), c.frames))[0]
                          if a <= p[0] < b or a <= p[1] < b]
    out = []
    for a, b in [(0, 24), (seam - 24, seam + 24), (c.frames - 24, c.frames)]:
        fr = [f for p in pairs(a, b) for f in p]
        out.append((min([a] + fr), max([b] + [f + 1 for f in fr])))
    return out


def cut_pairs(c, a, b):
    """The whole-stream call's pairs inside the (widened) cut [a, b), as indices into the cut."""
    return [(p - a, q - a) for p, q in device_pairs(c, 0, c.frames)[0] if a <= p and q < b]


def cut_reference(oracle, c, xf, a, b):
    """(K.Ref, lead) of frames [a, b) of a long stream from the samples those frames read: the piece starts `lead` hops early,
    and its first `lead` rows (zero history in the piece, not in the stream) are computed and dropped."""
    h = X.hop_len(c.n, c.ovl)
    lead = min(a, first_inside(c))
    sub = xf[(a - lead) * h:b * h]
    exact, f32, want = (rows[lead:] for rows in K.rows_of(oracle, c._replace(frames=b - a + lead), sub))
    t32 = tau_of(f32, exact)
    return K.Ref(sub, sub, exact, f32, want, t32, bound(t32), tau_of(want, exact), K.peak_err(want, exact)), lead


# every (case, slot, ranges) the CPU module holds to its conditions; ranges: the calls' [lo, hi)
def _whole(c):
    return [(0, c.frames)]


_ranges = {}
for _c in SIZE_CASES + CONTROL_CASES + MEAN_CASES + HISTORY_CASES + FORMAT_CASES + RANGE_CASES:
    _ranges.setdefault((_c, 0), _whole(_c))
for _c in BATCH_CASES:
    for _s in range(BATCH_SLOTS):
        _ranges.setdefault((_c, _s), _whole(_c))
for _c in RANGE_CASES:                                      # (a case of two groups: the union of its calls)
    _ranges[(_c, 0)] = _whole(_c) + [range_of(_c, a) for a in range_firsts(_c)]
CHECKED = [(c, s, r) for (c, s), r in _ranges.items()]

SEEDS = {
    ('mtm-n256-o0-rectangular-nw2-k2-f69-keyed-f32-m0-h0', 0): 5404,
    ('mtm-n256-o0.5-rectangular-nw2.5-k4-f101-keyed_noise-f32-m0-h0', 0): 5529,
    ('mtm-n256-o0.75-rectangular-nw4-k6-f101-keyed-f32-m0-h0', 0): 5464,
    ('mtm-n256-o0.9-rectangular-nw4.5-k8-f101-keyed_noise-f32-m0-h0', 0): 5567,
    ('mtm-n512-o0.75-rectangular-nw2-k2-f53-keyed_noise-f32-m0-h0', 0): 5722,
    ('mtm-n512-o0-rectangular-nw2.5-k4-f37-keyed-f32-m0-h0', 0): 5642,
    ('mtm-n512-o0.9-rectangular-nw4-k6-f90-keyed-f32-m0-h0', 0): 5710,
    ('mtm-n512-o0.5-rectangular-nw4.5-k8-f53-keyed_noise-f32-m0-h0', 0): 5764,
    ('mtm-n1024-o0.5-rectangular-nw2-k2-f45-keyed-f32-m0-h0', 0): 6148,
    ('mtm-n1024-o0.75-rectangular-nw2.5-k4-f45-keyed_noise-f32-m0-h0', 0): 6266,
    ('mtm-n1024-o0-rectangular-nw4-k6-f37-keyed_noise-f32-m0-h0', 0): 6246,
    ('mtm-n1024-o0.9-rectangular-nw4.5-k8-f127-keyed-f32-m0-h0', 0): 6285,
    ('mtm-n1024-o0.5-rectangular-nw12-k22-f45-keyed-f32-m0-h0', 0): 6288,
    ('mtm-n2048-o0-rectangular-nw2-k2-f29-keyed_noise-f32-m0-h0', 0): 7238,
    ('mtm-n2048-o0.9-rectangular-nw2.5-k4-f129-keyed-f32-m0-h0', 0): 7430,
    ('mtm-n2048-o0.5-rectangular-nw4-k6-f33-keyed-f32-m0-h0', 0): 7263,
    ('mtm-n2048-o0.75-rectangular-nw4.5-k8-f62-keyed_noise-f32-m0-h0', 0): 7372,
    ('mtm-n4096-o0-rectangular-nw2.5-k4-f87-keyed-f32-m0-h0', 0): 9276,
    ('mtm-n4096-o0.75-rectangular-nw2.5-k4-f353-keyed_noise-f32-m0-h0', 0): 9620,
    ('mtm-n4096-o0.5-rectangular-nw2-k2-f177-keyed-f32-m0-h0', 0): 9352,
    ('mtm-n4096-o0.9-rectangular-nw4.5-k8-f359-keyed_noise-f32-m0-h0', 0): 9680,
    ('mtm-n4096-o0.75-rectangular-nw4.5-k8-f353-keyed-f32-m0-h0', 0): 9570,
    ('mtm-n1024-o0.5-rectangular-nw2-k3-f45-keyed-f32-m0-h0', 0): 6164,
    ('mtm-n4096-o0.75-rectangular-nw2.5-k3-f353-keyed_noise-f32-m0-h0', 0): 9614,
    ('mtm-n1024-o0.5-rectangular-nw2.5-k4-f45-keyed_dc-f32-m1-h0', 0): 6203,
    ('mtm-n1024-o0.75-rectangular-nw2-k2-f45-keyed-f32-m1-h0', 0): 6153,
    ('mtm-n4096-o0.75-rectangular-nw2.5-k4-f353-keyed_dc-f32-m1-h0', 0): 9581,
    ('mtm-n4096-o0.5-rectangular-nw2.5-k4-f177-keyed-f32-m1-h0', 0): 9367,
    ('mtm-n512-o0.75-rectangular-nw2.5-k4-f53-keyed-f32-m0-h1', 0): 5662,
    ('mtm-n4096-o0.75-rectangular-nw2.5-k4-f353-keyed_noise-f32-m0-h1', 0): 9621,
    ('mtm-n256-o0.5-rectangular-nw2.5-k4-f101-keyed-s16-m0-h0', 0): 5452,
    ('mtm-n2048-o0-rectangular-nw2-k2-f29-keyed_noise-s16-m0-h0', 0): 7238,
    ('mtm-n4096-o0.75-rectangular-nw2.5-k4-f353-keyed-s16-m0-h0', 0): 9542,
    ('mtm-n256-o0.75-rectangular-nw2-k2-f101-keyed_noise-u8-m0-h0', 0): 5514,
    ('mtm-n256-o0.5-rectangular-nw2.5-k4-f170-keyed-f32-m0-h0', 0): 5520,
    ('mtm-n512-o0-rectangular-nw2.5-k4-f74-keyed_noise-f32-m0-h0', 0): 5757,
    ('mtm-n1024-o0.75-rectangular-nw2-k2-f82-keyed-f32-m0-h0', 0): 6185,
    ('mtm-n2048-o0.5-rectangular-nw2.5-k4-f62-keyed-f32-m0-h0', 0): 7205,
    ('mtm-n4096-o0-rectangular-nw2.5-k4-f175-keyed_noise-f32-m0-h0', 0): 9442,
    ('mtm-n4096-o0.75-rectangular-nw4.5-k8-f701-keyed-f32-m0-h0', 0): 9918,
    ('mtm-n512-o0.5-rectangular-nw2.5-k4-f53-keyed-f32-m0-h0', 0): 5671,
    ('mtm-n512-o0.5-rectangular-nw2.5-k4-f53-keyed-f32-m0-h0', 1): 6674,
    ('mtm-n512-o0.5-rectangular-nw2.5-k4-f53-keyed-f32-m0-h0', 2): 7681,
    ('mtm-n4096-o0-rectangular-nw2.5-k4-f87-keyed-f32-m0-h0', 1): 10285,
    ('mtm-n4096-o0-rectangular-nw2.5-k4-f87-keyed-f32-m0-h0', 2): 11294,
    ('mtm-n4096-o0.75-rectangular-nw2-k2-f353-keyed_noise-f32-m0-h0', 0): 9606,
    ('mtm-n4096-o0.75-rectangular-nw2-k2-f353-keyed_noise-f32-m0-h0', 1): 10615,
    ('mtm-n4096-o0.75-rectangular-nw2-k2-f353-keyed_noise-f32-m0-h0', 2): 11624,
    (case_id(LONG_Y), 0): 29672,                            # (the reduced census of its cuts, test_cuts_of_the_long_launches)
    (case_id(LONG_XL), 0): K.seed_of(LONG_XL),
}


def seed_of(c, slot=0):
    return SEEDS.get((case_id(c), slot), K.seed_of(c) + 1009 * slot)


Figures = namedtuple("Figures", "ref scaled unit exchanged")


def whole_pairs(c):
    return device_pairs(c, 0, c.frames)[0]


@functools.lru_cache(maxsize=4)
def figures(oracle, c, seed):
    """K.reference of the keyed stream and the three paired stand-ins' tau over the bound, on the whole-stream call's pairs."""
    r = K.reference(oracle, c, seed)
    pairs = whole_pairs(c)
    v, sig = K.tapers(oracle, c.n, c.kmax, c.nw)
    m = 1 if c.sub_mean else 0
    t = [tau_of(X.multitaper32_paired(r.xf, c.n, c.ovl, v, sig, m, c.history_mode, pairs, s), r.exact) / r.tau
         for s in ("own", "unit", "exchanged")] if pairs else [0.0, 0.0, 0.0]
    return Figures(r, *t)


def conditions(oracle, c, seed, ranges, unit_min=4.0):
    """(ok, lines): the census of every call's pairs under both readings of the grid, and the stand-in figures."""
    fg = figures(oracle, c, seed)
    power = fg.ref.exact.sum(axis=1)
    ok, lines = True, []
    for lo, hi in ranges:
        dev = census(power, *device_pairs(c, lo, hi))
        iss = census(power, *issue_pairs(c, lo, hi))
        lines.append("frames [%d, %d) device grid %s | grid from the first frame %s" % (lo, hi, tuple(dev), tuple(iss)))
        ok = ok and adversarial(iss, True) and (adversarial(dev, False) or not shares_transforms(c))
    if shares_transforms(c):
        ok = ok and fg.scaled <= 0.5 and fg.unit >= unit_min and fg.exchanged > 1.0
    return ok, lines


def find_seed(oracle, c, slot, ranges, tries=400):
    """The first seed from the case's own on that meets conditions() -- the unscaled stand-in 5x over the bound, to stay clear
    of the 4x asserted --; the frames' energies sift the candidates first."""
    base = K.seed_of(c) + 1009 * slot
    for s in range(base, base + tries):
        xf = K.make_input(oracle, c, s)[1]
        energy = (X.frames64(xf, c.n, c.ovl, 1 if c.sub_mean else 0, c.history_mode) ** 2).sum(axis=1)
        if not all(adversarial(census(energy, *issue_pairs(c, lo, hi)), True)
                   and (adversarial(census(energy, *device_pairs(c, lo, hi)), False) or not shares_transforms(c)) for lo, hi in ranges):
            continue
        if conditions(oracle, c, s, ranges, 5.0)[0]:
            return s
    return None
