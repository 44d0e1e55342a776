"""The jackknife statistic's definition, its coverage, and the rule of tests/_jackknife_check.py held against the float32 stand-in
and against mutations of it.  No GPU: the stand-in is 'the device' here.

1. In float64: the K = 2 closed form 1/4 (ln E_1 - ln E_0)^2; silence gives 0, a zero delete-one estimate under a non-zero S gives
   +inf, nothing gives NaN.
2. Coverage: on independent unit-exponential eigenspectra with equal weights the interval at 0.95 (the library's own Student
   quantile) covers the true level ln 1 in 0.92 - 0.97 of 200 000 draws, for K = 5 and K = 8 (a seeded run: 0.941 and 0.939), and
   the mean logvar is 1.12 (K = 5) and 1.07 (K = 8) times trigamma(K), the variance of ln of a mean of K unit exponentials.
3. The stand-in passes the rule within a QUARTER of REL_LOG on every case of the GPU grid (GRID below; tests/test_gpu_jackknife.py
   runs the same cases through check_case on the device), and the conditions on the cases hold in float64: at most 1e-3 of a
   noise-like case's bins lie below the floor, and on tone inputs never the carrier's +-2 ceil(w) bins or the weak line's bin.
4. The rule rejects each mutation of _jackknife_exact.MUTATIONS on a tone case and on a noise case.
   NOT REJECTED, reported by test_mutations_the_rule_cannot_reject and not hidden: the `total - term` form on `line` and `dc`
   (UNREJECTED below).  The adaptive weights cannot fall below lambda_j (beta_0 / beta_j)^2 (u_j >= B_0 / B_j), 3e-4 .. 5.5e-4 for
   j = 1 at the grid's time-bandwidth products, so on these inputs the cancellation costs at most 2^-24 / 3e-4 in one l_i: the
   mutated stand-in reaches 0.33 of the bound at most (K = 2, N = 256, iters = 8) where the honest one reaches 0.07.
   test_total_minus_term_on_a_dominant_taper shows what the form does where one taper does dominate -- eigenspectra with one
   taper 75 dB above the others -- and that the rule rejects it there.
"""
import numpy as np
import pytest

import _adaptive_check as AK
import _adaptive_exact as X
import _jackknife_check as JK
import _jackknife_exact as JX

SIZES = (256, 512, 1024, 2048, 4096)
TAPERS = ((1, 2.0), (4, 2.5), (7, 4.5))                       # (kmax, w): K = 2, 5 (odd: the lone taper) and 8
OVERLAPS = (0.0, 0.75)
FMTS = ("f32", "s16", "u8")
INPUTS = ("noise", "two_level", "line", "line_on_bin", "dc", "silence", "silent_frame")
NOISE_LIKE = ("noise", "two_level")
TONES = ("line", "line_on_bin")
FRAMES = 37                                                   # the last frame group of every size is partly filled
ITERS = (0, 2, 8)


def _grid():
    """(n, kmax, w, overlap, history_mode, fmt): every size with every taper count; the overlap, the history mode and the sample
    format in turn, so that each is seen with each taper count and at small and large sizes."""
    out = []
    for a, n in enumerate(SIZES):
        for b, (kmax, w) in enumerate(TAPERS):
            i = 3 * a + b
            out.append((n, kmax, w, OVERLAPS[i % 2], (i // 2) % 2, FMTS[i % 3]))
    return out


GRID = _grid()
CASE_ID = lambda c: "n%d_k%d_ov%g_hm%d_%s" % (c[0], c[1] + 1, c[3], c[4], c[5])  # noqa: E731


class Case:
    """One (grid case, input): the stream, its float64 eigenspectra, the stand-in's tau -- computed once, shared by the checks."""

    def __init__(self, lib, case, name, frames=FRAMES, seed=11, stride=None, levels=None):
        """stride (and levels): for the inputs of _adaptive_exact.PASS_INPUTS, the frames one pass of the call's grid covers."""
        self.n, self.kmax, self.w, self.overlap, self.hm, self.fmt = case
        self.name = name
        self.tapers, self.sig = lib.make_dpss(self.n, self.kmax, self.w)
        self.lam, self.beta = lib.adaptive_weights(lib.MtmParams(n=self.n, w=self.w, kmax=self.kmax, overlap=self.overlap))
        self.hop = int(self.n * (1.0 - self.overlap))
        if name in X.PASS_INPUTS:
            self.x = X.level_by_pass(name, self.n, self.hop, frames * self.hop + 3, seed, stride, self.fmt, self.w, levels)
        else:
            self.x = X.make_input(name, self.n, frames * self.hop + 3, seed, self.fmt, self.w)
        self.E64, self.s2 = X.eigen64(self.x, self.n, self.overlap, self.tapers, self.hm)
        assert self.E64.shape[0] == frames
        self.E32 = X.eigen32(self.x, self.n, self.overlap, self.tapers, self.hm)[0]
        self.tau = AK.eigen_tau(self.E32, self.E64)

    def stand_in(self, mutate=None, s2_stride=None):
        memo = {}

        def device(iters):
            if iters not in memo:
                memo[iters] = JX.jackknife32(self.x, self.n, self.overlap, self.tapers, self.lam, self.beta, iters, self.hm,
                                             mutate=mutate, s2_stride=s2_stride)[:3]
            return memo[iters]
        return device

    def weights(self, device, iters):
        """The reference weights of the call with `iters`: lambda for 0, else weights64 from the device's own psd of iters - 1."""
        if iters == 0:
            return JX.lambda_weights(self.lam, self.E64.shape)
        return JX.weights64(device(iters - 1)[0], self.E64, self.lam, self.beta, self.s2, self.n)

    def float64_weights(self, iters):
        """The weights of the same call from float64 alone (the conditions on a case are decided from these)."""
        if iters == 0:
            return JX.lambda_weights(self.lam, self.E64.shape)
        S = X.adaptive64(self.E64, self.lam, self.beta, self.s2, self.n, iters - 1)[0] if iters > 1 else X.start64(self.E64)
        return JX.weights64(S, self.E64, self.lam, self.beta, self.s2, self.n)


def case_conditions(c):
    """The conditions on a case, from float64 alone; returns the excluded share per ITERS."""
    shares = []
    cw = int(np.ceil(c.w))
    for iters in ITERS:
        share, mask = JK.excluded_share(c.E64, c.float64_weights(iters), c.tau)
        shares.append(share)
        if c.name in NOISE_LIKE:
            assert share <= JK.NOISE_SHARE, (c.name, iters, share)
        if c.name in TONES:
            cb = c.n // 8
            assert not mask[:, cb - 2 * cw:cb + 2 * cw + 2].any(), (c.name, iters, "a carrier bin below the floor")
            assert not mask[:, X.line_bin(c.n, c.w)].any(), (c.name, iters, "the weak line's bin below the floor")
    return shares


def check_case(c, device, rel=1.0):
    """The rule on the calls with iters 0, 2 and 8 of device(iters) -> (psd, dof, logvar) as numpy rows, the iters = 0 row and its
    degrees of freedom against float64, and iters = 1 held to 'non-negative or +inf, never NaN'.  Returns the record line."""
    K = c.kmax + 1
    fr, sh = [], []
    for iters in ITERS:
        f, s = JK.rule(device(iters)[2], c.E64, c.weights(device, iters), c.tau, rel=rel)
        fr.append(f)
        sh.append(s)
    lv1 = np.asarray(device(1)[2], np.float64)
    assert not np.isnan(lv1).any() and (lv1 >= 0).all()
    # iters = 0: the eigenvalue-weighted mean and its degrees of freedom
    psd0, dof0 = np.asarray(device(0)[0], np.float64), np.asarray(device(0)[1], np.float64)
    l64 = np.asarray(c.lam, np.float32).astype(np.float64)
    S0 = (l64[None, :, None] * c.E64).sum(axis=1) / l64.sum()
    A = AK.amplitude(c.E64)[:, None]
    fa = AK._ratio(np.abs(np.sqrt(psd0) - np.sqrt(S0)), c.tau * A + rel * AK.REL_AMP * np.sqrt(S0))
    assert fa <= 1.0, ("iters = 0 row", fa)
    nu0 = 2.0 * l64.sum() ** 2 / (l64 * l64).sum()
    assert np.isfinite(dof0).all() and np.abs(dof0 - nu0).max() <= rel * AK.REL_DOF * nu0 and 2.0 <= nu0 <= 2.0 * K
    if c.name == "silence":
        for iters in ITERS:
            assert all((np.asarray(r) == 0).all() for r in (device(iters)[0], device(iters)[2]))
    if c.name == "silent_frame":
        quiet = np.flatnonzero(c.s2 == 0)
        assert len(quiet) >= 1 and (np.asarray(device(8)[2])[quiet] == 0).all() and (np.asarray(device(0)[2])[quiet] == 0).all()
    return "n=%-5d K=%d w=%.1f ov=%-4g hm=%d %-3s %-12s tau %.3g  REL_LOG 2^%d  fraction of the bound, iters 0 / 2 / 8: %.3f %.3f %.3f  " \
           "excluded share: %.2g %.2g %.2g  iters = 0 row: %.3f" % (c.n, K, c.w, c.overlap, c.hm, c.fmt, c.name, c.tau,
                                                                   int(np.log2(JK.REL_LOG)), fr[0], fr[1], fr[2], sh[0], sh[1], sh[2], fa)


# ---- 1. the definition in float64
def test_two_tapers_closed_form():
    rng = np.random.default_rng(3)
    E = rng.exponential(size=(7, 2, 33)) * 10.0 ** rng.uniform(-20, 2, size=(7, 1, 33))
    w = rng.uniform(0.1, 1.0, size=(7, 2, 33))
    _, lv, smin = JX.jackknife64(E, w)
    want = 0.25 * (np.log(E[:, 1]) - np.log(E[:, 0])) ** 2
    assert np.allclose(lv, want, rtol=1e-9, atol=1e-24)
    assert np.allclose(smin, E.min(axis=1), rtol=1e-12)


def test_degenerate_cases_in_float64_and_float32():
    E = np.zeros((3, 4, 5))
    w = np.ones((3, 4, 5))
    S, lv, _ = JX.jackknife64(E, w)
    assert (S == 0).all() and (lv == 0).all()                                  # silence
    E[1, 2, :] = 3.0                                                           # one taper alone holds the power: S_(2) = 0
    S, lv, _ = JX.jackknife64(E, w)
    assert (lv[1] == np.inf).all() and (lv[0] == 0).all() and (lv[2] == 0).all() and (S[1] > 0).all()
    rng = np.random.default_rng(5)
    E = rng.exponential(size=(4, 5, 9)) * (rng.uniform(size=(4, 5, 9)) > 0.4)   # zeros sprinkled in
    for wts in (np.ones(E.shape), rng.uniform(size=E.shape), (rng.uniform(size=E.shape) > 0.5) + 0.0):
        wts[:, 0] = 1.0
        lv = JX.jackknife64(E, wts)[1]
        assert not np.isnan(lv).any() and (lv >= 0).all()


def _trigamma(k):
    return np.pi ** 2 / 6.0 - sum(1.0 / (m * m) for m in range(1, k))


@pytest.mark.parametrize("K,mean_ratio", ((5, 1.12), (8, 1.07)))
def test_coverage_on_exponential_eigenspectra(lib, K, mean_ratio):
    rng = np.random.default_rng(1991)
    E = rng.exponential(size=(200000, K, 1))
    S, lv, _ = JX.jackknife64(E, np.ones(E.shape))
    t = lib.jackknife_factor(lib.MtmParams(n=1024, w=4.5, kmax=K - 1), 0.95)
    half = t * np.sqrt(lv)
    covered = float((np.abs(np.log(S)) <= half).mean())
    ratio = float(lv.mean() / _trigamma(K))
    print("K = %d: the interval at 0.95 covers ln 1 in %.4f of 200000 draws; mean logvar = %.3f trigamma(K)" % (K, covered, ratio))
    assert 0.92 <= covered <= 0.97, covered
    assert abs(ratio - mean_ratio) <= 0.02, ratio


# ---- 3. the stand-in on the GPU grid
@pytest.mark.parametrize("case", GRID, ids=CASE_ID)
def test_stand_in_passes_the_rule_within_a_quarter(lib, case):
    for name in INPUTS:
        c = Case(lib, case, name)
        case_conditions(c)
        print(check_case(c, c.stand_in(), rel=0.25))


# ---- 3b. inputs keyed to the grid's passes: tests/test_adaptive_criterion.py's PASS_GRID and streams
def pass_case(lib, case, name, nbatch=1):
    """(Case, the passes of its call) of a level_by_pass stream of the two-pass frame count of its size."""
    import _grid_passes as G
    frames = G.TWO_PASS_FRAMES[case[0]]
    p = G.passes("spectro16a", case[0], frames, nbatch)
    return Case(lib, case, name, frames=frames, stride=p.stride), p


def _pass_criterion():
    from test_adaptive_criterion import PASS_CRITERION
    return PASS_CRITERION


@pytest.mark.parametrize("case,name", _pass_criterion(), ids=lambda v: v if isinstance(v, str) else CASE_ID(v))
def test_sigma2_of_the_frame_one_pass_earlier_is_rejected(lib, case, name):
    """level_by_pass: from float64 alone the excluded share of the noise-based streams stays within NOISE_SHARE (1e-3 level
    included, at every size: nothing had to be dropped); the stand-in passes the rule within a quarter of REL_LOG; the stand-in
    whose weights come from sigma2 of the frame one grid pass earlier is rejected.

    By WHICH assertion of the device test it is rejected depends on the case.  With five and eight tapers and sound in the later
    pass, by the logvar rule at iters 2 and 8 (iters = 0 has no sigma2 in it).  With TWO tapers logvar is 1/4 (ln E_1 - ln E_0)^2
    whatever the weights (test_two_tapers_closed_form), and a silent frame's logvar is 0 whatever they are: there the rule on
    logvar cannot see sigma2, and what rejects the stand-in is the other half of the device test -- psd and dof are the bits of
    adaptive(), whose rows tests/test_gpu_adaptive.py holds to the chained rule on the same stream.  Both are tried here, and
    which one fired is printed."""
    c, p = pass_case(lib, case, name)
    assert p.npasses == 2

    def chained_rule(device):
        """The chained rule of tests/_adaptive_check.py on the stand-in's psd and dof rows (m = 1 and 7: given S, no widening)."""
        for m in (1, 7):
            AK.chained(device(m)[0], device(m + 1)[0], device(m + 1)[1], c.E64, c.lam, c.beta, c.s2, c.n, c.tau)
    for iters in ITERS:
        share, _ = JK.excluded_share(c.E64, c.float64_weights(iters), c.tau)
        print("%s %s iters %d: excluded share %.2g" % (CASE_ID(case), name, iters, share))
        if name.startswith("noise"):
            assert share <= JK.NOISE_SHARE, (name, iters, share)
    print(check_case(c, c.stand_in(), rel=0.25))
    quiet = np.flatnonzero(c.s2 == 0)
    assert all((np.asarray(c.stand_in()(it)[2])[quiet] == 0).all() for it in ITERS)
    chained_rule(c.stand_in())
    fired = []
    for what, rule in (("logvar rule", lambda d: check_case(c, d)), ("chained rule on psd / dof", chained_rule)):
        try:
            rule(c.stand_in(s2_stride=p.stride))
        except AssertionError:
            fired.append(what)
    print("stale sigma2 %s %s: rejected by %s" % (CASE_ID(case), name, fired))
    assert "chained rule on psd / dof" in fired
    assert "logvar rule" in fired or c.kmax == 1 or name.endswith("gap") or c.fmt == "u8"


# ---- 4. mutations
MUTATION_GRID = (256, 4, 2.5, 0.75, 0, "f32")                  # five tapers: an odd count has the zero partner row
MUTATION_INPUTS = {m: ("line", "noise") for m in JX.MUTATIONS}
MUTATION_INPUTS["total_minus_term"] = ("line", "dc")
# (mutation, input): what the rule cannot reject, with the reason; test_mutations_the_rule_cannot_reject holds each to be so
_FLOOR_OF_WEIGHTS = "the weights stay above lambda_j (beta_0 / beta_j)^2, so the cancellation stays inside REL_LOG"
UNREJECTED = {("total_minus_term", "line"): _FLOOR_OF_WEIGHTS, ("total_minus_term", "dc"): _FLOOR_OF_WEIGHTS}


def _rejected(c, mutation):
    """Whether the rule rejects the mutated stand-in at any of the grid's sweep counts (the unmutated one passes at all)."""
    good, bad = c.stand_in(), c.stand_in(mutate=mutation)
    hit = []
    for iters in ITERS:
        w = c.weights(good, iters)                               # (psd is not mutated: the chain is the stand-in's own)
        JK.rule(good(iters)[2], c.E64, w, c.tau)
        try:
            JK.rule(bad(iters)[2], c.E64, w, c.tau)
        except AssertionError:
            hit.append(iters)
    return hit


@pytest.mark.parametrize("mutation", JX.MUTATIONS)
def test_rule_rejects_mutation(lib, mutation):
    for name in MUTATION_INPUTS[mutation]:
        if (mutation, name) in UNREJECTED:
            continue
        hit = _rejected(Case(lib, MUTATION_GRID, name, frames=9), mutation)
        print("%s on %s: rejected at iters %s" % (mutation, name, hit))
        assert hit, (mutation, name)


def test_mutations_the_rule_cannot_reject(lib):
    """Reported, not hidden: each entry of UNREJECTED is a mutation the rule lets through on that input, at every sweep count."""
    for (mutation, name), why in UNREJECTED.items():
        hit = _rejected(Case(lib, MUTATION_GRID, name, frames=9), mutation)
        print("NOT REJECTED: %s on %s -- %s" % (mutation, name, why))
        assert not hit, (mutation, name, hit)


def test_total_minus_term_on_a_dominant_taper():
    """One taper 75 dB above the others, equal weights: formed as total - term the delete-one estimate without that taper has
    lost every bit in float32, and the rule rejects the row; summed over the K - 1 others it is exact to rounding and passes."""
    f = np.float32
    rng = np.random.default_rng(7)
    K, frames, bins = 5, 6, 17
    E = (3e-8 * rng.exponential(size=(frames, K, bins))).astype(f)
    E[:, 2, :] = f(1.0) + rng.uniform(size=(frames, bins)).astype(f)
    Ej, wj = [E[:, j, :] for j in range(K)], [np.ones((frames, bins), f) for _ in range(K)]
    psd = JX._mean32(wj, E)[0]
    E64, w64 = E.astype(np.float64), np.ones(E.shape)
    tau = AK.MARGIN * AK.FLOOR                                   # the eigenspectra are given: the floor of tau
    frac, share = JK.rule(JX.statistic32(Ej, wj, psd), E64, w64, tau, rel=0.25)
    assert share == 0.0
    with pytest.raises(AssertionError):
        JK.rule(JX.statistic32(Ej, wj, psd, mutate="total_minus_term"), E64, w64, tau)
