"""The rules of tests/_adaptive_check.py held against the float32 stand-in and against mutations of it, and the premise of the
device's line assertion in float64.  No GPU: the stand-in is 'the device' here.

1. The stand-in passes the chained rule on every case within a QUARTER of the relative terms (2^-17 in amplitude, 2^-15 in dof:
   the derivation in _adaptive_check.py allows the device four times what the straightforward float32 evaluation needs), and the
   end-to-end rule on the noise-like cases.  The dof term at m = 0 is EXEMPT from the quarter test: there the stand-in is outside
   a quarter on tone inputs (the derivation's miss, _adaptive_check.start_dof_widen), the term is widened by the stand-in's own
   measured factor, and holding the stand-in against a bound made from its own error would say nothing.  Its fraction of the
   unwidened term is printed instead, and asserted to be what makes the widening necessary on at least one case.
2. Each mutation of _adaptive_exact.MUTATIONS is rejected by the chained rule on at least one case.
3. On the line inputs, in float64, the adaptive row has its largest bin outside the carrier's +-2 ceil(w) bins within the weak
   line's own +-ceil(w) bins (a multitaper line is a plateau that wide), and the fixed-weight row does not: for eight tapers at
   w = 4.5, every supported N, the three sample formats, full frames in history mode 0.  With five tapers at w = 2.5 the premise
   does NOT hold at the larger sizes -- just outside +-2 ceil(w) the fifth taper's first sidelobes stand 20 dB under the carrier
   and the broadband bound B_j = beta_j sigma2 / N is far below them, so the weights stay -- and those cases are not asserted on the
   device: test_line_premise_fails_with_five_tapers holds the failure itself, in float64.
"""
import numpy as np
import pytest

import _adaptive_check as K
import _adaptive_exact as X

# (n, kmax, w, overlap, history_mode, fmt, inputs): small sizes, every input, both history modes, an odd and an even taper count
CASES = (
    (256, 4, 2.5, 0.5, 0, "f32", X.INPUTS),
    (256, 1, 2.0, 0.0, 0, "s16", ("noise", "line", "silence", "dc")),
    (1024, 7, 4.5, 0.75, 1, "s16", ("noise", "dither", "line", "edge_tones", "silent_frame")),
    (512, 4, 2.5, 0.3, 1, "u8", ("noise", "two_level", "line_on_bin", "alternating", "impulses")),
)
TONE_STEPS = (0, 1, 7, 31)
STEPS = (0, 1, 7)


def _setup(lib, n, kmax, w, overlap, hm, fmt, name, frames=7):
    tapers, sig = lib.make_dpss(n, kmax, w)
    lam, beta = lib.adaptive_weights(lib.MtmParams(n=n, w=w, kmax=kmax, overlap=overlap))
    hop = int(n * (1.0 - overlap))
    x = X.make_input(name, n, frames * hop + 3, 5, fmt, w)
    E64, s2 = X.eigen64(x, n, overlap, tapers, hm)
    return x, tapers, sig, lam, beta, E64, s2


def _chain(device, steps, E64, lam, beta, s2, n, tau, rel, widen, start_dof=True):
    """device(iters) -> (psd, dof).  The chained rule at every step of `steps`; returns the worst fractions.  start_dof False: the
    dof of m = 0 is not checked."""
    fa = fd = 0.0
    for m in steps:
        psd_m = None if m == 0 else device(m)[0]
        psd_1, dof_1 = device(m + 1)
        if m == 0 and not start_dof:
            dof_1 = None
        a, d = K.chained(psd_m, psd_1, dof_1, E64, lam, beta, s2, n, tau, rel=rel, dof_widen=widen)
        fa, fd = max(fa, a), max(fd, d)
    return fa, fd


@pytest.mark.parametrize("case", CASES, ids=lambda c: "n%d_k%d_%s_hm%d" % (c[0], c[1] + 1, c[5], c[4]))
def test_stand_in_passes_both_rules_within_a_quarter(lib, case):
    n, kmax, w, overlap, hm, fmt, inputs = case
    for name in inputs:
        x, tapers, sig, lam, beta, E64, s2 = _setup(lib, n, kmax, w, overlap, hm, fmt, name)
        memo = {}

        def device(iters):
            if iters not in memo:
                memo[iters] = X.adaptive32(x, n, overlap, tapers, lam, beta, iters, hm)
            return memo[iters][:2]
        _, dof32_1, E32 = X.adaptive32(x, n, overlap, tapers, lam, beta, 1, hm)
        tau = K.eigen_tau(E32, E64)
        widen = K.start_dof_widen(dof32_1, E64, lam, beta, s2, n)
        steps = TONE_STEPS if name in ("line", "line_on_bin", "edge_tones") else STEPS
        fa, fd = _chain(device, steps, E64, lam, beta, s2, n, tau, rel=0.25, widen=1.0, start_dof=False)
        print("%-13s n=%d K=%d %s hm=%d: tau %.3g, chained fractions of the QUARTER terms: amp %.3f, dof at m >= 1 %.3f; dof at m = 0 "
              "(exempt): %.3f of the whole term" % (name, n, kmax + 1, fmt, hm, tau, fa, fd, (widen / 4.0 if widen > 1.0 else float("nan"))))
        if name in X.NOISE_LIKE:
            psd32 = device(8)[0]
            taup, want = K.end_to_end_tau(psd32, E32, E64, lam, beta, s2, n, 8)
            K.end_to_end(psd32, want, E64, taup)
        if name == "silence":
            assert (device(8)[0] == 0).all() and np.isfinite(device(8)[1]).all()


def test_start_dof_term_needs_its_widening(lib):
    """The stand-in is outside a quarter of the dof term at m = 0 on a tone input (here beyond the whole term): the widening is
    needed, and it is the measured factor times the margin."""
    n, kmax, w, overlap, hm, fmt = CASES[2][:6]
    x, tapers, sig, lam, beta, E64, s2 = _setup(lib, n, kmax, w, overlap, hm, fmt, "line")
    dof32_1 = X.adaptive32(x, n, overlap, tapers, lam, beta, 1, hm)[1]
    widen = K.start_dof_widen(dof32_1, E64, lam, beta, s2, n)
    assert widen > 4.0, widen
    with pytest.raises(AssertionError):
        K.chained(None, None, dof32_1, E64, lam, beta, s2, n, 0.0)                 # the unwidened term does not hold the stand-in
    K.chained(None, None, dof32_1, E64, lam, beta, s2, n, 0.0, dof_widen=widen)


# the case each mutation is shown on: a carrier's skirts are where the weights matter; zeroed history is where sigma2's does
MUTATION_CASES = {m: (256, 4, 2.5, 0.5, 0, "f32", "line") for m in X.MUTATIONS}
MUTATION_CASES["sigma2_fresh_only"] = (512, 4, 2.5, 0.75, 1, "f32", "line")


@pytest.mark.parametrize("mutation", X.MUTATIONS)
def test_rules_reject_mutation(lib, mutation):
    n, kmax, w, overlap, hm, fmt, name = MUTATION_CASES[mutation]
    x, tapers, sig, lam, beta, E64, s2 = _setup(lib, n, kmax, w, overlap, hm, fmt, name)
    _, dof32_1, E32 = X.adaptive32(x, n, overlap, tapers, lam, beta, 1, hm)
    tau = K.eigen_tau(E32, E64)
    widen = K.start_dof_widen(dof32_1, E64, lam, beta, s2, n)

    def good(iters):
        return X.adaptive32(x, n, overlap, tapers, lam, beta, iters, hm)[:2]

    def bad(iters):
        return X.adaptive32(x, n, overlap, tapers, lam, beta, iters, hm, mutate=mutation, sig=sig)[:2]
    _chain(good, STEPS, E64, lam, beta, s2, n, tau, rel=1.0, widen=widen)               # the case itself passes
    with pytest.raises(AssertionError):
        _chain(bad, STEPS, E64, lam, beta, s2, n, tau, rel=1.0, widen=widen)


# ---- inputs keyed to the grid's passes (tests/_grid_passes.py).  PASS_GRID is the GPU module's: every built size, K = 2 / 5 / 8 in
# turn (an odd count at N = 512 and at N = 4096: 32 and 256 lanes a frame), overlaps, history modes and formats in turn
PASS_TAPERS = ((1, 2.0), (4, 2.5), (7, 4.5))
PASS_GRID = tuple((n, PASS_TAPERS[i % 3][0], PASS_TAPERS[i % 3][1], (0.0, 0.5, 0.75, 0.3)[i % 4], int(i == 2), ("f32", "s16", "u8", "f32", "s16")[i])
                  for i, n in enumerate((256, 512, 1024, 2048, 4096)))


def pass_inputs_of(i):
    """Two of _adaptive_exact.PASS_INPUTS for case i of PASS_GRID: one on noise and one on the line, orders in turn."""
    orders = ("down", "up", "gap")
    return "noise_" + orders[i % 3], "line_" + orders[(i + 1) % 3]


def pass_stream(case, name, nbatch=1, seed=11, kernel="spectro16a"):
    """(x, the passes of its call): a stream of the two-pass frame count of its size, the levels laid out for the grid of a call
    over all its frames (as one of nbatch streams)."""
    import _grid_passes as G
    n, kmax, w, overlap, hm, fmt = case
    frames = G.TWO_PASS_FRAMES[n]
    p = G.passes(kernel, n, frames, nbatch)
    hop = int(n * (1.0 - overlap))
    nsamples = frames * hop + 3
    if name in X.PASS_INPUTS:
        return X.level_by_pass(name, n, hop, nsamples, seed, p.stride, fmt, w), p
    return X.make_input(name, n, nsamples, seed, fmt, w), p


# the criterion's cases: every case of the grid with the two inputs the GPU module gives it, and all six at N = 2048 and 4096
# (2 and 1 frames a block, 141 and 71 frames)
PASS_CRITERION = [(PASS_GRID[i], name) for i in (0, 1, 2) for name in pass_inputs_of(i)] + \
                 [(PASS_GRID[i], name) for i in (3, 4) for name in X.PASS_INPUTS]


@pytest.mark.parametrize("case,name", PASS_CRITERION, ids=lambda v: v if isinstance(v, str) else "n%d_k%d_%s" % (v[0], v[1] + 1, v[5]))
def test_sigma2_of_the_frame_one_pass_earlier_is_rejected(lib, case, name):
    """level_by_pass: the stand-in passes the chained rule (within a quarter of the relative terms, as on every other input); the
    stand-in that takes sigma2 -- what a block's lanes carry from a frame's first round to its epilogue -- from the frame one grid
    pass earlier is rejected: its weights are those of a frame 60 dB louder or quieter, or of silence (dof term), and where the
    stale frame was loud and this one is silent the silent frame's dof is not the one of sigma2 = 0."""
    n, kmax, w, overlap, hm, fmt = case
    x, p = pass_stream(case, name)
    assert p.npasses == 2
    tapers, sig = lib.make_dpss(n, kmax, w)
    lam, beta = lib.adaptive_weights(lib.MtmParams(n=n, w=w, kmax=kmax, overlap=overlap))
    E64, s2 = X.eigen64(x, n, overlap, tapers, hm)
    assert len(s2) == len(p.pass_of)
    # the levels do what the input is for: sigma2 of a frame and of the one a pass earlier differ by 10^5 or one of them is 0
    late = np.arange(p.stride + n // int(n * (1.0 - overlap)), len(s2))
    a, b = s2[late], s2[late - p.stride]
    assert ((a == 0) != (b == 0)).all() or (np.maximum(a, b) > 1e5 * np.minimum(a, b)).all(), name
    memo = {}

    def device(iters, stride=None):
        if (iters, stride) not in memo:
            memo[iters, stride] = X.adaptive32(x, n, overlap, tapers, lam, beta, iters, hm, s2_stride=stride)
        return memo[iters, stride][:2]
    _, dof32_1, E32 = X.adaptive32(x, n, overlap, tapers, lam, beta, 1, hm)
    tau = K.eigen_tau(E32, E64)
    widen = K.start_dof_widen(dof32_1, E64, lam, beta, s2, n)
    fa, fd = _chain(device, STEPS, E64, lam, beta, s2, n, tau, rel=0.25, widen=1.0, start_dof=False)
    print("%-10s n=%d K=%d %s: tau %.3g, chained fractions of the QUARTER terms: amp %.3f, dof %.3f" % (name, n, kmax + 1, fmt, tau, fa, fd))
    quiet = np.flatnonzero(s2 == 0)
    assert (device(8)[0][quiet] == 0).all() and np.isfinite(device(8)[1]).all()
    with pytest.raises(AssertionError):
        _chain(lambda it: device(it, p.stride), STEPS, E64, lam, beta, s2, n, tau, rel=1.0, widen=widen)


LINE_SIZES = (256, 512, 1024, 2048, 4096)
LINE_KMAX, LINE_W = 7, 4.5


def line_found(row, n, w):
    """The largest bin outside the carrier's +-2 ceil(w) bins lies within the weak line's +-ceil(w) bins."""
    cw = int(np.ceil(w))
    cb = int(X.carrier_bin(n))
    row = np.array(row, np.float64)
    row[max(cb - 2 * cw, 0):cb + 1 + 2 * cw + 1] = 0.0                     # (an off-bin carrier sits between cb and cb + 1)
    return abs(int(row.argmax()) - X.line_bin(n, w)) <= cw


def full_frames(n, overlap, nframes):
    hop = int(n * (1.0 - overlap))
    return range(-(-(n - hop) // hop), nframes)


@pytest.mark.parametrize("fmt", ("f32", "s16", "u8"))
@pytest.mark.parametrize("n", LINE_SIZES)
def test_line_premise_in_float64(lib, n, fmt):
    for name in ("line", "line_on_bin"):
        for overlap in (0.5, 0.75):
            x, tapers, sig, lam, beta, E64, s2 = _setup(lib, n, LINE_KMAX, LINE_W, overlap, 0, fmt, name, frames=8)
            S, _ = X.adaptive64(E64, lam, beta, s2, n, 8)
            F = X.fixed64(E64, sig)
            for f in full_frames(n, overlap, S.shape[0]):
                assert line_found(S[f], n, LINE_W), (name, overlap, f)
                assert not line_found(F[f], n, LINE_W), (name, overlap, f)


@pytest.mark.parametrize("fmt", ("f32", "s16", "u8"))
@pytest.mark.parametrize("n", (2048, 4096))
def test_line_premise_fails_with_five_tapers(lib, n, fmt):
    """Why the device assertion is made with eight tapers only: with five tapers at w = 2.5 the adaptive row in float64 does NOT
    have the weak line as its largest bin outside the carrier's +-2 ceil(w) bins, in any settled frame of either line input at
    either overlap (the carrier's skirt just outside those bins outranks it), and neither has the fixed-weight row."""
    for name in ("line", "line_on_bin"):
        for overlap in (0.5, 0.75):
            x, tapers, sig, lam, beta, E64, s2 = _setup(lib, n, 4, 2.5, overlap, 0, fmt, name, frames=8)
            S, _ = X.adaptive64(E64, lam, beta, s2, n, 8)
            F = X.fixed64(E64, sig)
            for f in full_frames(n, overlap, S.shape[0]):
                assert not line_found(S[f], n, 2.5), (name, overlap, f)
                assert not line_found(F[f], n, 2.5), (name, overlap, f)


def test_u8_line_at_30_db_is_found_by_the_fixed_row_too(lib):
    """Why the u8 line is 45 dB under the carrier and not 30: at 30 dB the fixed-weight row of eight tapers shows the line as well
    (its skirt beside an off-bin carrier stands 36 dB down), so the premise 'and the fixed-weight row does not' fails."""
    n, overlap = 1024, 0.5
    tapers, sig = lib.make_dpss(n, LINE_KMAX, LINE_W)
    x = X.make_input("line", n, 8 * (n // 2) + 3, 5, "u8", LINE_W, line_db=-30.0)
    E64, _ = X.eigen64(x, n, overlap, tapers, 0)
    F = X.fixed64(E64, sig)
    assert all(line_found(F[f], n, LINE_W) for f in full_frames(n, overlap, F.shape[0]))
