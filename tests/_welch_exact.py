"""Float64 'exact-arithmetic' Welch rows (segment-averaged auto-spectra, cross-spectrum, coherence) of two interleaved channels,
their float32 stand-in, and the cases and inputs the Welch tests share (tests only): tests/_cross_exact.py for Spectrogram.cross_welch.

Row r of (L, step, first) averages the frames f = first + r step + s, s = 0 .. L-1, of _cross_exact's per-frame spectra:

    Sxx[r] = (1/L) sum_s Sxx_f    Syy likewise    Sxy[r] = (1/L) sum_s Sxy_f    coh[r] = |Sxy[r]|^2 / (Sxx[r] Syy[r]), 0 where that is 0

welch64: the per-frame float64 rows of cross64 averaged in float64.  welch32: the per-frame float32 sums of cross32 accumulated in
float32 in the kernel's order (segments in increasing s) and scaled by float32 1 / L; the quotient in double from those.  An FFT
plan is the one-taper case: tapers = [window] (a rectangular window is all ones), sig = [0], so c = 1 / N.
"""
import collections

import numpy as np

import _cross_exact as E
import _grid_passes as G
from _exact import hop_len

LINE10_DB = -10.0


def rows_of(nframes, segments, step, first=0):
    """(F - first - L) / step + 1, or 0 if F - first < L."""
    return (nframes - first - segments) // step + 1 if nframes - first >= segments else 0


def _rows(per_frame, segments, step, first, nrows, acc, order):
    nrows = rows_of(per_frame.sxx.shape[0], segments, step, first) if nrows is None else nrows
    out = []
    for a in (per_frame.sxx, per_frame.syy, per_frame.sxy):
        a = np.asarray(a)
        o = np.zeros((nrows,) + a.shape[1:], acc[np.iscomplexobj(a)])
        for r in range(nrows):
            for s in order(segments):
                o[r] += a[first + r * step + s]
        out.append(o)
    return out


def welch64(per_frame, segments, step, first=0, nrows=None):
    """per_frame: cross64's rows of the stream.  Returns Cross of float64 / complex128 [rows][n/2+1]."""
    sxx, syy, sxy = (o / segments for o in _rows(per_frame, segments, step, first, nrows, (np.float64, np.complex128), range))
    return E.Cross(sxx, syy, sxy, E._coh(sxx, syy, sxy))


def welch32(per_frame, segments, step, first=0, nrows=None, reverse=False):
    """per_frame: cross32's rows of the stream.  Float32 accumulation over the segments (reverse: in decreasing s), one float32
    1 / L; coh float64 from the float32 rows."""
    order = (lambda n: range(n - 1, -1, -1)) if reverse else range
    inv = np.float32(1.0 / segments)
    sxx, syy, sxy = _rows(per_frame, segments, step, first, nrows, (np.float32, np.complex64), order)
    sxx, syy = (sxx * inv).astype(np.float32), (syy * inv).astype(np.float32)
    sxy = ((sxy.real * inv).astype(np.float32) + 1j * (sxy.imag * inv).astype(np.float32)).astype(np.complex64)
    return E.Cross(sxx, syy, sxy, E._coh(sxx, syy, sxy))


# ---- plans: (kind, window name or kmax, nw).  The MTM kinds fix their segment count: (kmax, L) = (0, 3), (1, 2), (4, 3)
KINDS = (("fft", "rectangular", None), ("mtm", 0, 2.0), ("fft", "hanning", None), ("mtm", 1, 2.0), ("fft", "blackman", None), ("mtm", 4, 2.5))
MTM_SEGMENTS = {0: 3, 1: 2, 4: 3}
FMTS = ("f32", "s16", "u8")


def params_of(lib, n, kind, overlap, fmt="f32", hist=0):
    sf = {"f32": lib.SAMPLES_F32, "s16": lib.SAMPLES_S16, "u8": lib.SAMPLES_U8}[fmt]
    if kind[0] == "fft":
        return lib.FftParams(n=n, window_type=lib.WINDOWS[kind[1]], overlap=overlap, history_mode=hist, sample_format=sf)
    return lib.MtmParams(n=n, overlap=overlap, w=kind[2], kmax=kind[1], history_mode=hist, sample_format=sf)


_tables = {}


def tables_of(lib, n, kind):
    """(tapers [J][n] float64, sig [J]) of the plan: host code of the library, no device."""
    key = (n,) + tuple(kind)
    if key not in _tables:
        if kind[0] == "fft":
            w = np.ones(n) if kind[1] == "rectangular" else lib.make_window(lib.WINDOWS[kind[1]], n).astype(np.float64)
            _tables[key] = (w[None, :], np.zeros(1))
        else:
            _tables[key] = lib.make_dpss(n, kind[1], kind[2])
    return _tables[key]


# ---- inputs: _cross_exact's nine, and line10
def make_input(name, n, nsamples, seed):
    """line10: independent noise of sigma 0.2 in each channel and a common sine at bin N/4 + 3, 10 dB under each channel's noise
    in total power, phases 0.3 and 1.1."""
    if name != "line10":
        return E.make_input(name, n, nsamples, seed)
    rng = np.random.default_rng([seed, n, 1010])
    t = np.arange(nsamples, dtype=np.float64)
    amp = 0.2 * np.sqrt(2.0) * 10.0 ** (LINE10_DB / 20.0)
    x = 0.2 * rng.standard_normal(nsamples) + amp * np.sin(2 * np.pi * E.line_bin(n) * t / n + 0.3)
    y = 0.2 * rng.standard_normal(nsamples) + amp * np.sin(2 * np.pi * E.line_bin(n) * t / n + 1.1)
    return np.clip(np.stack([x, y], axis=1), -0.999, 0.999).astype(np.float32)


# ---- the cases of tests/test_gpu_welch.py (tests/test_welch_criterion.py runs the rule on some of the same inputs)
Case = collections.namedtuple("Case", "n kind ovl fmt hist segments step rows name")
SIZES = (256, 512, 1024, 2048, 4096, 8192)
OVERLAPS = (0.0, 0.3, 0.5, 0.75)
FFT_SEGMENTS = (2, 3, 8)


def frames_per_block(n):
    return max(1, 4096 // n)


def cases():
    out = []
    count = {"fft": 0, "mtm": 0}

    def segments_step(kind):
        """FFT plans walk the grid {2, 3, 8} x {1, L, L + 2} in turn; the MTM kinds fix L and take the three steps in turn."""
        i = count[kind[0]]
        count[kind[0]] += 1
        seg = MTM_SEGMENTS[kind[1]] if kind[0] == "mtm" else FFT_SEGMENTS[i % 3]
        return seg, (1, seg, seg + 2)[(i // 3) % 3]

    for s, n in enumerate(SIZES):
        fpb = frames_per_block(n)
        for i, name in enumerate(E.INPUTS):
            kind = KINDS[(i + s) % 6]
            if name == "edge_tones" and kind == KINDS[0]:
                # Tones on the odd bins 1 and N/2 - 1 under a rectangular window: the float32 samples satisfy x[t + N/2] == -x[t]
                # bit for bit, so every even bin of the float64 reference is an EXACT zero -- a degenerate reference, where the
                # rule's "coh == 0 where Sxx Syy == 0" (written for silent channels) would ask a float32 transform to cancel
                # exactly.  Any other window breaks the antisymmetry, so this input takes the Hanning window instead
                # (tests/test_welch_criterion.py::test_float64_products_vanish_for_silence_only holds every case to that).
                kind = KINDS[2]
            seg, step = segments_step(kind)
            # never a multiple of the block's frames, so the clamp runs; more than one block at least once per size
            rows = (fpb + 5 if i == 0 else (5 if (i + s) % 2 else 7)) if fpb > 1 else (2 if step > seg else 3)
            out.append(Case(n, kind, OVERLAPS[(i + 2 * s) % 4], "f32", 0, seg, step, rows, name))
        for j, fmt in enumerate(("s16", "u8")):
            kind = KINDS[(j + s + 2) % 6]
            seg, step = segments_step(kind)
            out.append(Case(n, kind, OVERLAPS[(j + s) % 4], fmt, 0, seg, step, 5 if fpb > 1 else 2, "noise"))
        kind = KINDS[(2 * s + 1) % 6]
        seg, step = segments_step(kind)
        out.append(Case(n, kind, OVERLAPS[1 + s % 3], FMTS[s % 3], 1, seg, step, 7 if fpb > 1 else 2, "delay3"))
    out.append(Case(256, KINDS[2], 0.5, "f32", 0, 64, 64, 3, "noise"))             # one long accumulation
    return out


def line10_case(n):
    """Hanning, 50 % overlap, L = step = 16, three rows."""
    return Case(n, KINDS[2], 0.5, "f32", 0, 16, 16, 3, "line10")


def case_id(c):
    kind = c.kind[1] if c.kind[0] == "fft" else "k%d" % (c.kind[1] + 1)
    return "n%d-%s-o%g-%s-h%d-L%d-s%d-r%d-%s" % (c.n, kind, c.ovl, c.fmt, c.hist, c.segments, c.step, c.rows, c.name)


def frames_of(c):
    return (c.rows - 1) * c.step + c.segments


_inputs, _refs = {}, {}


def case_input(c, seed=0, nbatch=1):
    """(the stream in the plan's format, its float32 values), made once per case and left unchanged.  The inputs of
    _cross_exact.PASS_INPUTS are laid out for the passes of the call's grid over the case's rows (a batch of nbatch streams
    shares the grid: other boundaries)."""
    key = (c.n, c.ovl, c.fmt, frames_of(c), c.name, seed) + ((c.segments, c.step, nbatch) if c.name in E.PASS_INPUTS else ())
    if key not in _inputs:
        if c.name in E.PASS_INPUTS:
            stride = G.passes("spectro16cx", c.n, c.rows, nbatch).stride
            xy = E.make_pass_input(c.name, c.n, hop_len(c.n, c.ovl), frames_of(c), seed, stride, c.segments, c.step)
        else:
            xy = make_input(c.name, c.n, frames_of(c) * hop_len(c.n, c.ovl), seed)
        raw = E.quantise(xy, c.fmt)
        _inputs[key] = (raw, E.to_float32(raw, c.fmt))
    return _inputs[key]


# ---- rows past one pass of the grid: 71 units of work, the rows of tests/_grid_passes.py's table (rows, not frames, are the work)
PASS_SIZES = (256, 2048, 8192)
PASS_PLANS = ((KINDS[2], 3, 1), (KINDS[2], 3, 5), (KINDS[3], 2, 2))           # Hanning (L, step) = (3, 1), (3, 5); two tapers (2, 2)
PASS_NAMES = ("noise",) + E.PASS_INPUTS


def pass_cases():
    """Every size with every plan; two of the four inputs each, so that every input is seen at every size and with every plan;
    overlaps and formats in turn (apart_by_pass never in u8: its quiet channel would be digital silence), one history_mode = 1."""
    out = []
    for s, n in enumerate(PASS_SIZES):
        for pl, (kind, seg, step) in enumerate(PASS_PLANS):
            i = 3 * s + pl
            for name in (PASS_NAMES[i % 4], PASS_NAMES[(i + 2) % 4]):
                fmt = FMTS[i % 3]
                out.append(Case(n, kind, OVERLAPS[i % 4], "s16" if fmt == "u8" and name == "apart_by_pass" else fmt, int(i == 4),
                                seg, step, G.TWO_PASS_FRAMES[n], name))
    return out


def row_bits(frame_bits, segments, step, rows):
    """A row's silence bits: those of its segments OR-ed."""
    frame_bits = np.asarray(frame_bits)
    out = np.zeros(rows, np.int64)
    for s in range(segments):
        out |= frame_bits[s:s + (rows - 1) * step + 1:step]
    return out


def welch32_packed(packed, segments, step, bits):
    """packed: _cross_exact.cross32_packed's per-frame rows with every bit set (nothing zeroed).  The float32 average over the
    segments, then the rows of a channel whose ROW bit is clear stored as zeros -- as the kernel does it."""
    w = welch32(packed, segments, step)
    sxx, syy, sxy = w.sxx.copy(), w.syy.copy(), w.sxy.copy()
    bits = np.asarray(bits)
    sxx[(bits & 1) == 0] = 0
    syy[(bits & 2) == 0] = 0
    sxy[bits != 3] = 0
    return E.Cross(sxx, syy, sxy, E._coh(sxx, syy, sxy))


def case_per_frame(lib, c, seed=0):
    """(cross64's, cross32's) per-frame rows of the case's stream, computed once and shared."""
    key = (c.n, c.kind, c.ovl, c.fmt, c.hist, frames_of(c), c.name, seed) + ((c.segments, c.step) if c.name in E.PASS_INPUTS else ())
    if key not in _refs:
        tapers, sig = tables_of(lib, c.n, c.kind)
        xy32 = case_input(c, seed)[1]
        _refs[key] = (E.cross64(xy32, c.n, c.ovl, tapers, sig, c.hist), E.cross32(xy32, c.n, c.ovl, tapers, sig, c.hist))
    return _refs[key]
