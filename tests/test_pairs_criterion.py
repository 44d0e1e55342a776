"""The keyed matrix (tests/_pairs_cases.py) on the CPU, no device involved: is every case of tests/test_gpu_pairs.py one that a
wrong scale in odd_taper.hpp could not pass?

For every (case, slot) of P.CHECKED, with its seed of P.SEEDS:
1. Reference and stand-in: the float32 stand-in and the oracle pass check_rows against float64 at the case's bound
   4 max(tau_f32, 2^-24) and the oracle the suite's 1e-5, as tests/test_rows_criterion.py asserts for its own cases.
2. The case is adversarial, for every call the GPU module makes of it (the whole stream; each first_frame of the range tests),
   under both readings of the pair grid (P.device_pairs: frame_cuts.h's; P.issue_pairs: blocks from the call's first frame):
   at least 4 partner pairs 10^6 apart in row power in each order, a (silent, loud) and a (loud, silent) pair, silent = float64
   row sum exactly 0; and, where the grid can leave one, a lone frame.
3. The rule sees the scales: _exact.multitaper32_paired on the whole stream's device pairs stays at or below 0.5 of the bound
   with the scales, exceeds it 4x with both scales 1 and exceeds it with the two scales exchanged.  With the scales 1 a silent
   frame beside a loud one is no longer silent, which check_rows refuses whatever tau.
The even-taper controls share no transform: 1 and 2 (on the grid a sharing kernel would use) show their inputs are the same
kind.  The ragged streams (0 ... 4 FPB + 3 frames) are too short for a census: they get 1 and the stand-in with the scales.
The cuts of the long launches are judged on the whole-stream call's pairs that touch them, with a reduced census (one pair
10^6 apart in each order in every cut of 8 pairs and more, the seam's among them) and the three stand-in figures there.  The two
plain u8 cases (N = 2048, 4096) cannot meet 3's 4x: they get 1, the silent pairs of 2 and the silent-row half of 3.
"""
import os
import subprocess

import numpy as np
import pytest

import _exact as X
import _pairs_cases as P
import _rows_cases as K
from _rows_check import FLOOR, bound, check_rows, tau_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _id(e):
    return "%s-slot%d" % (P.case_id(e[0]), e[1])


def test_every_case_has_its_seed_and_stays_out_of_the_rows_sweep():
    assert len({_id(e) for e in P.CHECKED}) == len(P.CHECKED)
    missing = [_id(e) for e in P.CHECKED if (P.case_id(e[0]), e[1]) not in P.SEEDS]
    assert not missing, missing
    assert not {c for c, _, _ in P.CHECKED} & set(K.ALL_CASES)
    sizes = {(c.n, c.kmax) for c in P.SIZE_CASES}
    assert {n for n, _ in sizes} == {256, 512, 1024, 2048, 4096} and {k for _, k in sizes} >= {2, 4, 6, 8, 22}
    assert {round(c.ovl, 2) for c in P.SIZE_CASES} == {0.0, 0.5, 0.75, 0.9}
    assert all(c.frames >= {256: 69, 512: 37, 1024: 21, 2048: 13, 4096: 11}[c.n] for c, _, _ in P.CHECKED)
    assert all(not P.shares_transforms(c) for c in P.CONTROL_CASES) and all(P.shares_transforms(c) for c in P.SIZE_CASES)


@pytest.mark.parametrize("e", P.CHECKED, ids=_id)
def test_case_is_adversarial_and_the_rule_sees_the_scales(oracle, e):
    c, slot, ranges = e
    seed = P.seed_of(c, slot)
    fg = P.figures(oracle, c, seed)
    r = fg.ref
    # 1
    assert np.isfinite(r.tau_f32) and r.tau == bound(r.tau_f32) and r.tau >= 4 * FLOOR
    assert check_rows(r.f32, r.exact, r.tau, _id(e)) <= 0.25 + 1e-12
    assert np.isfinite(r.tau_oracle) and r.e_ref <= K.TOL
    # 2
    power = r.exact.sum(axis=1)
    for lo, hi in ranges:
        dev, iss = P.census(power, *P.device_pairs(c, lo, hi)), P.census(power, *P.issue_pairs(c, lo, hi))
        print("pairs-criterion %-66s slot %d frames [%d, %d) g %d: device grid %s; grid from the first frame %s" % (
            P.case_id(c), slot, lo, hi, P.fpb(c.n), dev._asdict(), iss._asdict()))
        assert P.adversarial(iss, True), (lo, hi, iss)
        if P.shares_transforms(c):
            assert P.adversarial(dev, False), (lo, hi, dev)
        else:
            assert dev.pairs == 0
    # 3
    print("pairs-criterion %-66s slot %d seed %d tau_f32 %.3e bound %.3e paired stand-in / bound: scaled %.3f unscaled %.1f exchanged %.3g" % (
        P.case_id(c), slot, seed, r.tau_f32, r.tau, fg.scaled, fg.unit, fg.exchanged))
    if not P.shares_transforms(c):
        return
    assert fg.scaled <= 0.5 and fg.unit >= 4.0 and fg.exchanged > 1.0, fg[1:]
    pairs = P.whole_pairs(c)
    v, sig = K.tapers(oracle, c.n, c.kmax, c.nw)
    m = 1 if c.sub_mean else 0
    scaled = X.multitaper32_paired(r.xf, c.n, c.ovl, v, sig, m, c.history_mode, pairs, "own")
    assert check_rows(scaled, r.exact, r.tau, _id(e) + " paired stand-in") <= 0.5
    rest = sorted(set(range(c.frames)) - {f for p in pairs for f in p})
    assert np.array_equal(scaled[rest], r.f32[rest])                        # a frame in no pair: the unpaired stand-in's row
    with pytest.raises(AssertionError):                                      # a silent frame beside a loud one picks up its rounding
        check_rows(X.multitaper32_paired(r.xf, c.n, c.ovl, v, sig, m, c.history_mode, pairs, "unit"), r.exact, 1e30)


def test_paired_stand_in_is_the_unpaired_one_on_equal_partners(oracle):
    """A stationary input (tests/_rows_cases.py's kind): with or without the scales the shared transform holds the bound --
    which is why that matrix cannot see them."""
    c = K.mtm(1024, 0.5, 2.5, 4, 21, "noise")
    r = K.reference(oracle, c)
    v, sig = K.tapers(oracle, c.n, c.kmax, c.nw)
    pairs = P.device_pairs(c, 0, c.frames)[0]
    assert len(pairs) == 4                                                   # (frames 8 ... 15: the first group reaches back before sample 0)
    for s in ("own", "unit", "exchanged"):
        assert check_rows(X.multitaper32_paired(r.xf, c.n, c.ovl, v, sig, 0, 0, pairs, s), r.exact, r.tau, s) <= 0.5


def test_device_grid_is_frame_cuts(tmp_path):
    """P.device_pairs against glfer_amd/csrc/frame_cuts.h itself: tests/c_frame_cuts.c walks the header as a C99 caller and prints
    glfer_frame_group per size and glfer_cut_frames for lo in 0..40, hi in lo..lo+40, first_inside in {0, 1, 3, 7}, G in
    {1, 2, 8, 16}; the frames device_pairs pairs are the header's body [b0, b1), partners FPB apart inside one group."""
    exe = tmp_path / "c_frame_cuts"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "glfer_amd", "csrc"),
                    os.path.join(ROOT, "tests", "c_frame_cuts.c"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120, check=True).stdout.splitlines()
    groups = {int(l.split()[1]): (int(l.split()[2]), int(l.split()[3])) for l in out if l.startswith("group ")}
    for n in (256, 512, 1024, 2048, 4096):
        assert groups[n] == (2 * P.fpb(n), 1)
    size_of = {2 * P.fpb(n): n for n in (512, 1024, 4096)}                     # G = 16, 8, 2
    ovl_of = {0: 0.0, 1: 0.5, 3: 0.75, 7: 0.875}                             # first_inside = ceil((N - H) / H)
    seen = 0
    for l in out:
        if not l.startswith("cut "):
            continue
        lo, hi, fi, G, b0, b1 = (int(w) for w in l.split()[1:])
        if G not in size_of:
            continue
        c = K.mtm(size_of[G], ovl_of[fi], 2.5, 4, 100)
        assert P.first_inside(c) == fi
        pairs, lone = P.device_pairs(c, lo, hi)
        g = G // 2
        assert not lone and all(q - p == g and p // G == q // G and p % G < g for p, q in pairs)
        assert sorted(f for p in pairs for f in p) == list(range(b0, b1)), l
        seen += 1
    assert seen == 3 * 4 * 41 * 41


@pytest.mark.parametrize("c", P.RAGGED_CASES, ids=K.case_id)
def test_ragged_streams(oracle, c):
    streams = P.ragged_streams(oracle, c)
    g = P.fpb(c.n)
    assert sorted(fr for _, fr in streams) == sorted([0, 1, 2, g, 2 * g + 1, 4 * g + 3])
    v, sig = K.tapers(oracle, c.n, c.kmax, c.nw)
    peaks = []
    for i, (x, fr) in enumerate(streams):
        assert len(x) == (fr * c.n if fr else c.n - 1)
        if not fr:
            continue
        m = c._replace(frames=fr)
        exact, f32, want = K.rows_of(oracle, m, x)
        tau = bound(tau_of(f32, exact))
        pairs = P.device_pairs(m, 0, fr)[0]
        frac = check_rows(X.multitaper32_paired(x, c.n, 0.0, v, sig, 0, 0, pairs, "own"), exact, tau, "stream %d" % i)
        assert frac <= 0.5 and K.peak_err(want, exact) <= K.TOL
        peaks.append(float(np.abs(x).max()))
        print("pairs-criterion ragged %s stream %d frames %d pairs %d peak %.3g paired stand-in / bound %.3f" % (K.case_id(c), i, fr, len(pairs), peaks[-1], frac))
    assert max(peaks) >= 1e4 * min(p for p in peaks if p > 0)


def test_second_pass_of_the_long_n256_launch():
    """The seam the N = 256 cuts straddle, from spectro16xl.hip's launcher: 2 048 workgroups x 32 frames behind the first group."""
    c, seam = P.LONG_CASES[1]
    assert c is P.LONG_XL and seam == P.xl_second_pass_from(c) == 32 + 2048 * 32
    assert seam + 24 <= c.frames // 32 * 32                                  # (the seam's cut lies in the body)
    assert P.xl_second_pass_from(c._replace(frames=32 + 65536 + 31)) is None and P.xl_second_pass_from(c._replace(frames=49152 + 1009)) == 32 + 1560 * 32


@pytest.mark.parametrize("cs", P.LONG_CASES, ids=lambda cs: K.case_id(cs[0]))
def test_cuts_of_the_long_launches(oracle, cs):
    """The cuts the GPU module judges, widened to their frames' partners in the whole-stream call: stand-in and oracle as in 1,
    the paired stand-in on those pairs, and a reduced census -- a cut of LONG_MIN_PAIRS pairs and more holds at least one pair
    10^6 apart in each order; the seam's cut is such a cut."""
    c, seam = cs
    xf = K.make_input(oracle, c, P.seed_of(c))[1]
    v, sig = K.tapers(oracle, c.n, c.kmax, c.nw)
    cuts = P.long_cuts(c, seam)
    for i, (a, b) in enumerate(cuts):
        r, lead = P.cut_reference(oracle, c, xf, a, b)
        assert check_rows(r.f32, r.exact, r.tau) <= 0.25 + 1e-12 and np.isfinite(r.tau_oracle) and r.e_ref <= K.TOL
        pairs = P.cut_pairs(c, a, b)
        assert all(0 <= p and q < b - a for p, q in pairs)
        cen = P.census(r.exact.sum(axis=1), pairs, [])
        t = [tau_of(X.multitaper32_paired(r.xf, c.n, c.ovl, v, sig, 0, 0, [(p + lead, q + lead) for p, q in pairs], s)[lead:], r.exact) / r.tau
             for s in ("own", "unit", "exchanged")]
        print("pairs-criterion long %s frames [%d, %d): pairs of the whole-stream call %s paired stand-in / bound: scaled %.3f unscaled %.1f exchanged %.3g" % (
            K.case_id(c), a, b, cen._asdict(), t[0], t[1], t[2]))
        assert t[0] <= 0.5
        if i == 1:
            assert cen.pairs >= P.LONG_MIN_PAIRS and seam - 24 >= a and seam + 24 <= b
        if cen.pairs >= P.LONG_MIN_PAIRS:
            assert cen.loud_first >= 1 and cen.quiet_first >= 1 and t[1] >= 4.0 and t[2] > 1.0, (a, b, cen, t)


@pytest.mark.parametrize("c", P.FORMAT_PLAIN_CASES, ids=K.case_id)
def test_plain_u8_cases(oracle, c):
    """u8 at N = 2048 and 4096 (see tests/_pairs_cases.py): conditions 1 and the silent pairs of 2; of 3 the scaled stand-in and
    that the scales 1 break the silent-row rule.  The unscaled figure is printed: it is why these are no cases of CHECKED."""
    assert (c, 0) not in {(cc, s) for cc, s, _ in P.CHECKED}
    fg = P.figures(oracle, c, P.seed_of(c))
    r = fg.ref
    assert r.raw.dtype == np.uint8 and check_rows(r.f32, r.exact, r.tau) <= 0.25 + 1e-12 and r.e_ref <= K.TOL
    pairs = P.whole_pairs(c)
    cen = P.census(r.exact.sum(axis=1), pairs, [])
    print("pairs-criterion plain %s device grid %s paired stand-in / bound: scaled %.3f unscaled %.1f exchanged %.3g" % (
        K.case_id(c), cen._asdict(), fg.scaled, fg.unit, fg.exchanged))
    assert cen.silent_loud >= 1 and cen.loud_silent >= 1 and fg.scaled <= 0.5
    v, sig = K.tapers(oracle, c.n, c.kmax, c.nw)
    with pytest.raises(AssertionError):
        check_rows(X.multitaper32_paired(r.xf, c.n, c.ovl, v, sig, 0, 0, pairs, "unit"), r.exact, 1e30)
