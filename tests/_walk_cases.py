"""The register-walk and second-unit case matrix (tests only), shared by tests/test_walk_criterion.py (CPU) and
tests/test_gpu_walk.py (the device, bin by bin under tests/_rows_check.py's unchanged rule).  None of these cases is in
tests/_rows_cases.py's ALL_CASES.  The schedule they are built on is tests/_grid_passes.py's restatement of the launchers.

B  WALK_CASES: the periodogram at overlap 87.5 / 75 / 50 % without mean removal on streams whose body reaches launch16h_fmt's
   `work >= 4 * resident`: spectro16h.hip's SHIFT = 2 / 4 / 8 instantiations, where a slot walks `per` consecutive frames and keeps
   16 - SHIFT of its sample registers.  Frames = ceil(R / H) head frames (packed kernel) + the threshold of the size + a
   remainder that leaves a partly filled last slot (per = 4 with G.WALK_REM_EVEN, per = 5 with G.WALK_REM_ODD).
C  SECOND_CASES: 65 ... 71 units of work on a grid of 64 for spectro16xl / spectro16x / spectro16 (GLFER_FORM=x) / spectro16h's
   multitaper form / spectro16w, inputs keyed to the units: the level of a body frame's newest hop is
   (1, 1e-3, 0)[(pass + logical workgroup) mod 3], so a workgroup's consecutive units always differ in level and every level
   occurs in both passes; odd taper counts take tests/_pairs_cases.py's keyed inputs with a census of the second pass's pairs.
D  BIG_CASES: spectro_big.hip past subfft_kernel's 4096-workgroup grid cap and past the launcher's first scratch group, on cuts.

Seeds are found against conditions on float64 frame powers (find_seed), never from device output.
"""
import functools
from collections import namedtuple

import numpy as np

import _exact as X
import _grid_passes as G
import _pairs_cases as P
import _rows_cases as K
from _rows_check import bound, tau_of, tau_of_spectrum

fft, mtm, case_id = K.fft, K.mtm, K.case_id
RATIO = 1e6                      # neighbouring frames' row powers at least this far apart
LOUD = 1e-3                      # a loud frame: at least this fraction of the stream's strongest frame


# ---- B -------------------------------------------------------------------------------------------------------------------
def _w(n, ovl, window, rem, signal, fmt="f32"):
    return fft(n, ovl, window, G.walk_frames(n, X.hop_len(n, ovl), rem), signal, fmt)


_E, _O = G.WALK_REM_EVEN, G.WALK_REM_ODD
WALK_CASES = [
    _w(512, 0.75, "hanning", _E, "keyed"), _w(512, 0.5, "kaiser", _O, "keyed_noise", "s16"),
    _w(1024, 0.875, "hanning", _O, "keyed"), _w(1024, 0.75, "blackman", _E, "keyed_noise", "u8"),       # (u8 / s16 at 75 %: TW1R off)
    _w(2048, 0.5, "hanning", _E, "weak"), _w(2048, 0.75, "hamming", _O, "keyed", "s16"),
    _w(4096, 0.75, "hanning", _O, "keyed"),                                                             # C2's own shape
    _w(4096, 0.5, "hanning", _E, "keyed_noise"), _w(4096, 0.875, "kaiser", _O, "noise"), _w(4096, 0.75, "hanning", _E, "keyed", "s16"),
    _w(8192, 0.75, "hanning", _O, "keyed_noise"), _w(8192, 0.5, "blackman", _O, "keyed", "u8"),
    _w(16384, 0.875, "hanning", _O, "keyed"), _w(16384, 0.5, "kaiser", _O, "weak", "s16"),
]
# the same plans one work unit below the threshold: SHIFT = 0
BELOW_CASES = [c._replace(frames=G.first_inside(c.n, X.hop_len(c.n, c.ovl)) + (4 * G.walk_resident(c.n) - 1) * G.KERNELS["spectro16h"].fpb(c.n))
               for c in (WALK_CASES[0], WALK_CASES[6], WALK_CASES[12])]
WALK_OFFSETS = {case_id(c): 2 for c in WALK_CASES if (c.fmt, c.n) in (("s16", 2048), ("u8", 8192))}      # (even: the pairs stay aligned)


def head_of(c):
    return G.first_inside(c.n, X.hop_len(c.n, c.ovl))


def walk_of(c, lo=0, hi=None, nbatch=1):
    """(b0, G.Walk) of a call over frames [lo, hi) of the case's stream."""
    hi = c.frames if hi is None else hi
    b0, b1 = G.cut_frames(lo, hi, head_of(c))
    return b0, G.walk(c.n, X.hop_len(c.n, c.ovl), b1 - b0, nbatch)


# one range call per overlap: first_frame off the slot grid of the whole-stream call and of its own, ending inside a slot
RANGE_CASES = [WALK_CASES[2], WALK_CASES[6], WALK_CASES[1]]          # 87.5 / 75 / 50 %


def range_of(c):
    """[first, hi): starts 7 frames behind the head, ends 2 frames early or a frame or two more (whichever leaves the call's own last slot partly
    filled) -- the body stays above the threshold, and tests/test_grid_passes_host.py asserts that the start lies off the whole-stream
    call's slot grid."""
    lo, hi = head_of(c) + 7, c.frames - 2
    while walk_of(c, lo, hi)[1].last_slot_frames == walk_of(c, lo, hi)[1].per:
        hi -= 1
    return lo, hi


# a two-stream batch and a ragged call of unequal streams, both bodies above the threshold
BATCH_CASE = WALK_CASES[7]
RAGGED_CASE = WALK_CASES[0]
RAGGED_MORE = 8 * 16 + 5                                             # the second stream's frames beyond the first's


def is_keyed(c):
    return c.signal.startswith("keyed")


def walk_conditions(c, power, lo=0, hi=None):
    """(ok, lines).  power: the float64 row sums of the stream's frames.  At every place `it` of a slot's walk (it mod 16 / SHIFT is
    the rotation phase, it mod 2 the parity) the body of the call [lo, hi) holds a frame at least RATIO below its predecessor
    (a silent one counts), one at least RATIO above, and a silent frame next to a loud one."""
    b0, w = walk_of(c, lo, hi)
    f = b0 + np.arange(len(w.it))
    p, q = power[f], power[f - 1]
    loud = LOUD * power.max()
    nxt = power[np.minimum(f + 1, len(power) - 1)]
    down = (q > 0) & (p * RATIO <= q)
    up = (p > 0) & (q * RATIO <= p)
    quiet = (p == 0) & ((q >= loud) | (nxt >= loud))
    ok, lines = w.shift > 0, []
    for it in range(w.per):
        m = w.it == it
        n = (int((down & m).sum()), int((up & m).sum()), int((quiet & m).sum()))
        lines.append("it %d phase %d parity %d: %d down, %d up, %d silent beside loud" % (it, it % w.nphase, it & 1, *n))
        ok = ok and min(n) >= 1
    return ok, lines


def frame_power(c, xf):
    """The frames' sample energies: what sifts seeds (the float64 row sums follow them up to the window)."""
    return (X.frames64(xf, c.n, c.ovl) ** 2).sum(axis=1)


SEEDS = {   # found by find_seed(); every other case meets the conditions with its own seed
    ('fft-n16384-o0.875-hanning-nw0-k0-f1041-keyed-f32-m0-h0', 0): 17495,
}


def seed_of(c, slot=0):
    return SEEDS.get((case_id(c), slot), K.seed_of(c) + 1009 * slot)


def find_seed(oracle, c, slot=0, tries=50, ranges=((0, None),)):
    """The first seed from the case's own on whose frame energies meet walk_conditions() on every range (the criterion test
    then asserts them on the float64 rows)."""
    base = K.seed_of(c) + 1009 * slot
    for s in range(base, base + tries):
        e = frame_power(c, K.make_input(oracle, c, s)[1])
        if all(walk_conditions(c, e, lo, hi)[0] for lo, hi in ranges):
            return s
    return None


# ---- the stand-ins of a wrong walk, built from the schedule: float32 rows with some frames assembled wrongly ----------------
def _frames_of(xf, c, frames, hops):
    """Float32 frames whose q-th hop (oldest first) is the stream's hop hops[i][q]."""
    h = X.hop_len(c.n, c.ovl)
    x = np.asarray(xf, np.float32)
    out = np.empty((len(frames), c.n), np.float32)
    for i in range(len(frames)):
        for q, src in enumerate(hops[i]):
            out[i, q * h:(q + 1) * h] = x[src * h:(src + 1) * h]
    return out


def _some(frames, most=192):
    """At most `most` of the frames, the first and the last among them."""
    frames = np.asarray(frames)
    return frames if len(frames) <= most else frames[np.unique(np.linspace(0, len(frames) - 1, most).astype(int))]


WALK_STANDINS = ("landing_exchanged", "kept_hop_stale", "slot_start_from_previous_slot")


def walk_standin(oracle, c, r, kind):
    """(rows, frames): r.f32 with the frames `frames` recomputed in float32 from wrongly assembled samples.
    landing_exchanged: one frame a slot (it = 1) takes its newest hop from the following frame -- the PF2 landing sets exchanged;
    kept_hop_stale: at one rotation phase (it = per - 1) a kept hop in the middle of the frame is the one the register held a
    frame earlier; slot_start_from_previous_slot: a slot's first frame (it = 0) keeps the previous slot's last frame's registers
    where they were -- every kept hop a frame stale -- and loads only its newest hop."""
    b0, w = walk_of(c)
    nh = w.nphase
    f = b0 + np.arange(len(w.it))
    own = lambda fr: [list(range(k - nh + 1, k + 1)) for k in fr]
    if kind == "landing_exchanged":
        fr = _some(f[(w.it == 1) & (f + 1 < c.frames)])
        hops = own(fr)
        for hp in hops:
            hp[-1] += 1
    elif kind == "kept_hop_stale":
        fr = _some(f[w.it == w.per - 1])
        hops = own(fr)
        for hp in hops:
            hp[(nh - 1) // 2] -= 1
    else:
        assert kind == "slot_start_from_previous_slot"
        fr = _some(f[(w.it == 0) & (w.slot > 0)])
        hops = [[k - nh + q for q in range(nh - 1)] + [k] for k in fr]
    rows = np.array(r.f32, copy=True)
    rows[fr] = X._power32(X._rfft32(_frames_of(r.xf, c, fr, hops) * K.window(oracle, c.n, c.window)), c.n)
    return rows, fr


# ---- C -------------------------------------------------------------------------------------------------------------------
# kernel: the KERNELS entry whose second unit the case runs; form: tests/_rows_device.py's switch; dev_mean: the device's
# sub_mean (None: the case's); offset: samples into the allocation; key: 'pass' (levels by unit) or 'pairs' (keyed, odd tapers)
Second = namedtuple("Second", "kernel c form dev_mean offset spectrum key units")
LEVELS = (1.0, 1e-3, 0.0)


def _shared_odd(s):
    return s.kernel in ("spectro16x", "spectro16xl")


def second_cut(s, frames=None):
    """(b0, b1) of the whole-stream call: the frames the case's kernel takes."""
    c = s.c
    frames = c.frames if frames is None else frames
    if s.kernel == "spectro16" or s.spectrum:                        # the packed route and N = 32768 take the call whole
        return 0, frames
    return G.cut_frames(0, frames, head_of(c), G.frame_group(_shared_odd(s), c.n))


def _s(kernel, c, form="default", dev_mean=None, offset=0, spectrum=False, units=71):
    """The case with its frame count: the head, `units` units of body work of which the last is partly filled where a unit has
    more than one frame (the shared-odd kernels take whole groups: their odd frames are the packed tail), and a tail."""
    key = "pairs" if kernel in ("spectro16x", "spectro16xl") else "pass"
    s = Second(kernel, c, form, dev_mean, offset, spectrum, key, units)
    fpb = G.KERNELS[kernel].fpb(c.n)
    if _shared_odd(s):
        grp = G.frame_group(True, c.n)
        b0 = -(-head_of(c) // grp) * grp
        return s._replace(c=c._replace(frames=b0 + units * fpb + grp // 2 + 1))
    b0 = 0 if kernel == "spectro16" or spectrum else head_of(c)
    return s._replace(c=c._replace(frames=b0 + G.second_unit_frames(kernel, c.n, units)))


SECOND_CASES = [
    _s("spectro16xl", mtm(512, 0.5, 2.5, 4, 0, "keyed")), _s("spectro16xl", mtm(1024, 0.0, 2.5, 4, 0, "keyed_noise"), units=69),
    _s("spectro16xl", mtm(2048, 0.5, 2.5, 4, 0, "keyed"), units=70),
    _s("spectro16x", mtm(1024, 0.5, 12.0, 22, 0, "keyed")),
    _s("spectro16", fft(512, 0.75, "hanning", 0, "weak"), "x"), _s("spectro16", fft(1024, 0.0, "kaiser", 0, "noise"), "x", units=66),
    _s("spectro16", fft(4096, 0.5, "hanning", 0, "weak"), "x", units=70), _s("spectro16", fft(8192, 0.75, "blackman", 0, "noise"), "x"),
    _s("spectro16", mtm(512, 0.0, 2.5, 3, 0, "noise"), "x", units=68), _s("spectro16", mtm(1024, 0.5, 2.0, 3, 0, "weak"), "x"),
    _s("spectro16", mtm(4096, 0.75, 4.0, 7, 0, "weak"), "x", units=67), _s("spectro16", mtm(8192, 0.0, 2.5, 3, 0, "noise"), "x"),
    _s("spectro16h_mt", mtm(8192, 0.0, 2.5, 4, 0, "weak")), _s("spectro16h_mt", mtm(8192, 0.5, 2.5, 4, 0, "weak", "f32", 1), dev_mean=2, units=69),
    _s("spectro16h_mt", mtm(8192, 0.75, 2.0, 3, 0, "weak", "f32", 1), dev_mean=2, units=66),
    _s("spectro16w", mtm(16384, 0.0, 4.5, 8, 0, "weak")),
    _s("spectro16w", fft(2048, 0.5, "hanning", 0, "noise"), "w"), _s("spectro16w", fft(4096, 0.75, "kaiser", 0, "weak"), "w", units=69),
    _s("spectro16w", fft(8192, 0.0, "hanning", 0, "weak"), "w", units=65),
    _s("spectro16w", mtm(2048, 0.0, 2.5, 4, 0, "weak"), "w", units=67), _s("spectro16w", mtm(4096, 0.5, 2.0, 3, 0, "noise", "s16"), "w", offset=2),
    _s("spectro16w", mtm(8192, 0.75, 4.0, 7, 0, "weak"), "w", units=70),
    _s("spectro16w", fft(32768, 0.5, "hanning", 0, "weak"), spectrum=True, units=66),
]


def second_id(s):
    return "%s-%s-%s%s" % (s.kernel, case_id(s.c), s.form, "-spectrum" if s.spectrum else "")


def second_passes(s):
    """(b0, b1, G.Passes of the body)."""
    b0, b1 = second_cut(s)
    return b0, b1, G.passes("spectro16h" if s.kernel == "spectro16h_mt" else s.kernel, s.c.n, b1 - b0)


def second_pairs(s):
    """Odd taper counts: the (A, B) frame pairs of the body's SECOND pass (stream frame indices)."""
    b0, b1, p = second_passes(s)
    return [(a, b) for a, b in P.device_pairs(s.c, 0, s.c.frames)[0] if p.pass_of[a - b0] >= 1]


def second_levels(s):
    """'pass' cases: the level of every hop of the stream (hop f is frame f's newest)."""
    b0, b1, p = second_passes(s)
    lv = np.ones(s.c.frames + 1)
    lv[b0:b1] = np.asarray(LEVELS)[(p.pass_of + p.logical) % 3]
    return lv


def _convert(oracle, c, x):
    if c.fmt == "s16":
        raw = np.clip(np.round(x.astype(np.float64) * 20000), -32768, 32767).astype(np.int16)
        return raw, oracle.pcm_s16_to_float(raw)
    if c.fmt == "u8":
        raw = np.clip(np.round(x.astype(np.float64) * 100 + 128), 0, 255).astype(np.uint8)
        return raw, oracle.pcm_u8_to_float(raw)
    return x, x


def second_pairs_ok(s, power):
    """A pair RATIO apart in each order, and a silent frame beside a live partner, in the SECOND pass."""
    cs = P.census(power, second_pairs(s), [])
    return cs.loud_first >= 1 and cs.quiet_first >= 1 and cs.silent_loud + cs.loud_silent >= 1, cs


def second_input(oracle, s, seed=None):
    """(raw, xf) of the case."""
    c = s.c
    if s.key == "pairs":
        return K.make_input(oracle, c, second_seed(s) if seed is None else seed)
    h = X.hop_len(c.n, c.ovl)
    count = c.frames * h + min(3, h - 1)
    x = K.signal(c, count).astype(np.float64) * np.repeat(second_levels(s), h)[:count]
    return _convert(oracle, c, x.astype(np.float32))


SECOND_SEEDS = {   # found by find_second_seed() on the frames' energies; every other case passes with its own seed
    'spectro16xl-mtm-n2048-o0.5-rectangular-nw2.5-k4-f287-keyed-f32-m0-h0-default': 7429,
}


def second_seed(s):
    return SECOND_SEEDS.get(second_id(s), K.seed_of(s.c))


def find_second_seed(oracle, s, tries=400):
    for seed in range(K.seed_of(s.c), K.seed_of(s.c) + tries):
        if second_pairs_ok(s, frame_power(s.c, K.make_input(oracle, s.c, seed)[1]))[0]:
            return seed
    return None


def ref_of(oracle, c, raw, xf):
    """K.Ref of the float stream xf under the case's estimator."""
    exact, f32, want = K.rows_of(oracle, c, xf)
    t32 = tau_of(f32, exact)
    return K.Ref(raw, xf, exact, f32, want, t32, bound(t32), tau_of(want, exact), K.peak_err(want, exact))


@functools.lru_cache(maxsize=2)
def second_reference(oracle, s):
    raw, xf = second_input(oracle, s)
    return ref_of(oracle, s.c, raw, xf)


def second_spectrum_reference(oracle, s):
    """(exact_X, spectrum32, tau_f32, tau) of a spectrum=True case."""
    c = s.c
    _, xf = second_input(oracle, s)
    w = K.window(oracle, c.n, c.window)
    exact_X = X.spectrum64(xf, c.n, c.ovl, w)
    t32 = tau_of_spectrum(X.spectrum32(xf, c.n, c.ovl, w), exact_X, c.n)
    return exact_X, t32, bound(t32)


SECOND_STANDINS = ("unit_from_predecessor", "partners_scales_exchanged")


def second_standin(oracle, s, r, kind):
    """unit_from_predecessor: every second-pass frame's row is the row of the frame its lanes handled one pass earlier
    (passes().prev) -- the unit computed from its predecessor's samples; partners_scales_exchanged (odd tapers): the paired
    float32 stand-in with the partners' scales exchanged, in the second pass's pairs only."""
    c = s.c
    b0, b1, p = second_passes(s)
    if kind == "unit_from_predecessor":
        rows = np.array(r.f32, copy=True)
        late = np.flatnonzero(p.pass_of >= 1)
        rows[b0 + late] = r.f32[b0 + p.prev[late]]
        return rows
    assert kind == "partners_scales_exchanged" and s.key == "pairs"
    v, sig = K.tapers(oracle, c.n, c.kmax, c.nw)
    return X.multitaper32_paired(r.xf, c.n, c.ovl, v, sig, 0, 0, second_pairs(s), "exchanged")


# ---- D -------------------------------------------------------------------------------------------------------------------
# N = 32768, W = 16: subfft_kernel's workgroups take 4 of the nf * W work items each (spectro_big.hip:48-50, 335-336), so 1024
# frames fill the 4096-workgroup grid and frame 1024 is workgroup 0's second item.  N = 2^20, W = 512: a frame's scratch is
# 512 * 1024 * 8 bytes = 4 MiB, group = 512 MiB / 4 MiB = 128 frames (:322-333): frames 128 ... 130 are the second group
BIG_CAP = (fft(32768, 0.75, "hanning", 1024 + 5, "noise"), [(0, 3), (1022, 1027), (1026, 1029)])
BIG_GROUP = (fft(1 << 20, 0.875, "hanning", 131, "noise"), [(0, 3), (126, 131), (128, 131)])
BIG_CASES = [BIG_CAP, BIG_GROUP]


def big_wrap_frame(n):
    """The first frame whose first work item is a workgroup's second: 4096 workgroups x 4 items over W = n / 2048 items a frame."""
    return 4096 * 4 // (n // 2048)


def big_group_frames(n, ntap=1):
    return (512 << 20) // (ntap * (n // 2048) * 1024 * 8)
