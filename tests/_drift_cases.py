"""The inputs the drift tests share: the device cases of tests/test_gpu_drift.py (tests/test_drift_criterion.py shows on the same
inputs that a mutated restatement changes output bits) and the detection cases of the criterion.  Inputs only; the definition
is tests/_drift_exact.py."""
import collections
import zlib

import numpy as np

import _drift_exact as X

Case = collections.namedtuple("Case", "name kind bins pitch T step F dmin dmax")

PAD = np.float32(1e30)            # what the padding between bins and pitch holds


def _case(name, kind, bins, T, step, nblocks, extra, dmin, dmax, pad=0):
    return Case(name, kind, bins, bins + pad, T, step, (nblocks - 1) * step + T + extra, dmin, dmax)


# The kernel's tile is 256 bins, its largest register group 64 drifts, its groups 8 / 32 / 64 wide; the halo is max(-dmin, dmax).
# Shapes: a row shorter than the halo, at a tile edge, one bin past it; one, two and four passes; step 1, T and T + 3; F = T and
# one row short of a further block (extra = step - 1); pitched rows (padding 1e30) and dense ones (the neighbours are the rows
# themselves, loud).
CASES = [
    _case("b1_T2_full", "noise", 1, 2, 1, 3, 0, -1, 1),
    _case("b5_T3_full_pitched", "noise", 5, 3, 3, 2, 2, -2, 2, pad=3),
    _case("b5_T16_full", "noise", 5, 16, 19, 2, 18, -15, 15),
    _case("b63_T17_full_pitched", "noise", 63, 17, 1, 4, 0, -16, 16, pad=1),
    _case("b64_T16_up", "noise", 64, 16, 16, 2, 15, 0, 15),
    _case("b65_T16_down_pitched", "noise", 65, 16, 19, 2, 18, -15, 0, pad=5),
    _case("b255_T3_full", "noise", 255, 3, 6, 2, 5, -2, 2),
    _case("b256_T2_full_pitched", "noise", 256, 2, 2, 3, 1, -1, 1, pad=2),
    _case("b257_T3_zero_only", "noise", 257, 3, 3, 3, 0, 0, 0),
    _case("b129_T64_two_passes", "noise", 129, 64, 64, 1, 0, -63, 63),
    _case("b257_T65_three_passes_pitched", "noise", 257, 65, 68, 2, 5, -64, 64, pad=3),
    _case("b65_T256_four_passes", "noise", 65, 256, 256, 1, 0, -127, 127),
    _case("b2049_T16_full", "noise", 2049, 16, 1, 3, 0, -15, 15),
    _case("b300_T16_nine_drifts", "noise", 300, 16, 16, 2, 3, -4, 4),
    # special values, 65 bins, T = 16, the full range, two blocks
    _case("inf", "inf", 65, 16, 16, 2, 0, -15, 15),
    _case("nan", "nan", 65, 16, 16, 2, 0, -15, 15),
    _case("silence", "silence", 65, 16, 16, 2, 0, -15, 15),
    _case("const", "const", 65, 16, 16, 2, 0, -15, 15),
    _case("cross", "cross", 65, 16, 16, 2, 0, -15, 15),
]
BY_NAME = {c.name: c for c in CASES}


def noise_rows(rng, F, bins):
    """unit-mean exponential noise, a frame's level a power of ten between 1e-2 and 1e2 that differs from its neighbours'"""
    decade = np.array([(7 * t) % 5 - 2 for t in range(F)], dtype=np.float64)
    return (rng.exponential(1.0, (F, bins)) * 10.0 ** decade[:, None]).astype(np.float32)


def make_rows(case):
    """[F][pitch] float32, the same at every call"""
    rng = np.random.default_rng(zlib.crc32(case.name.encode()))
    rows = np.full((case.F, case.pitch), PAD, dtype=np.float32)
    data = rows[:, :case.bins]
    if case.kind == "silence":
        data[:] = 0
    elif case.kind == "const":
        data[:] = 1.5
    elif case.kind == "cross":
        # two lines of power 1 through bin 32, drifts +9 and -9, in every block: at bin 32 the sums of +9 and -9 tie above drift 0's
        data[:] = 0
        for f in range(case.F):
            o = X.offset(case.T, 9, f % case.T)
            data[f, 32 + o] = 1
            data[f, 32 - o] = 1
    else:
        data[:] = noise_rows(rng, case.F, case.bins)
        if case.kind == "inf":
            data[3, 20] = np.inf
            data[case.T + 5, 0] = np.inf
        elif case.kind == "nan":
            data[10, 30] = np.nan         # on the zero-drift line of bin 30, off it for the twenty bins whose lines cross (10, 30)
            data[case.T + 15, 64] = np.nan
    return rows


_reference = {}


def reference(case):
    """(sums, best, drift) of the case by the float32 restatement, computed once"""
    if case.name not in _reference:
        got = X.drift_all(make_rows(case), case.bins, case.T, case.step, case.dmin, case.dmax)
        for a in got:
            a.setflags(write=False)
        _reference[case.name] = got
    return _reference[case.name]


# ---- the detection premise: a line of constant power A along k0 + o(d0, t) in unit-mean exponential noise, three blocks
Detect = collections.namedtuple("Detect", "T bins A d0 seed")
DETECT = [Detect(16, 257, 3.0, 9, 11), Detect(16, 257, 3.0, -13, 12), Detect(64, 129, 1.5, -40, 13), Detect(8, 65, 6.0, 7, 14)]
DETECT_BLOCKS = 3
DETECT_MARGIN = 1.25


def detect_k0(c):
    return c.bins // 2


def detect_rows(c):
    """[3 T][bins] float64: the noise and the line"""
    rng = np.random.default_rng(c.seed)
    rows = rng.exponential(1.0, (DETECT_BLOCKS * c.T, c.bins))
    for f in range(rows.shape[0]):
        rows[f, detect_k0(c) + X.offset(c.T, c.d0, f % c.T)] += c.A
    return rows


def detect_check(c, best, drift):
    """the premise on one call's best / drift: in every block the largest best is at k0 with drift d0 and stands at least 1.25
    times over the largest best outside k0 +- 2.  Returns the margins."""
    k0, margins = detect_k0(c), []
    for b in range(DETECT_BLOCKS):
        assert int(np.argmax(best[b])) == k0, (c, b, int(np.argmax(best[b])))
        assert int(drift[b][k0]) == c.d0, (c, b, int(drift[b][k0]))
        away = np.delete(best[b], np.arange(k0 - 2, k0 + 3))
        margins.append(float(best[b][k0]) / float(away.max()))
        assert margins[-1] >= DETECT_MARGIN, (c, b, margins[-1])
    return margins
