"""The cross rows' criterion without a GPU (tests/_cross_check.py): the float32 stand-in passes it on held-out draws of every
input, the float64 facts the device test leans on hold, and the rule rejects wrong rows that are close to right ones.

What a peak-normalised 1e-5 (max |got - ref| <= 1e-5 max |ref| per output, the loosest check in use here) lets through is printed
beside every mutation and collected in test_mutations_are_rejected's docstring."""
import numpy as np
import pytest

import _cross_check as K
import _cross_exact as E

# (n, kmax, nw, overlap): two, five and eight tapers
CASES = [(256, 1, 2.0, 0.0), (512, 4, 2.5, 0.3), (1024, 7, 4.0, 0.5)]
NFRAMES = 5


def _hop(n, overlap):
    from _exact import hop_len
    return hop_len(n, overlap)


_memo = {}


def _case(lib, n, kmax, nw, overlap, name, seed):
    key = (n, kmax, overlap, name, seed)
    if key not in _memo:
        tapers, sig = lib.make_dpss(n, kmax, nw)
        xy = E.make_input(name, n, NFRAMES * _hop(n, overlap), seed)
        _memo[key] = (xy, tapers, sig, E.cross64(xy, n, overlap, tapers, sig))
    return _memo[key]


@pytest.mark.parametrize("n,kmax,nw,overlap", CASES)
@pytest.mark.parametrize("name", E.INPUTS)
def test_stand_in_passes_on_held_out_draws(lib, n, kmax, nw, overlap, name):
    xy, tapers, sig, ref = _case(lib, n, kmax, nw, overlap, name, 0)
    tau = K.tau_of(E.cross32(xy, n, overlap, tapers, sig), ref)
    assert K.FLOOR * K.MARGIN <= tau < 1e-5, tau
    for seed in (1, 2):
        xy2, _, _, ref2 = _case(lib, n, kmax, nw, overlap, name, seed)
        K.check(E.cross32(xy2, n, overlap, tapers, sig), ref2, tau, "%s n=%d held-out %d" % (name, n, seed))


@pytest.mark.parametrize("n,kmax,nw,overlap", CASES)
def test_float64_facts(lib, n, kmax, nw, overlap):
    """y = x: coh64 = 1 wherever a > 0.  Silence and a silent channel: coh64 = 0 everywhere.  A delay of three samples: the phase
    of Sxy64 at a mid-band bin of a settled frame is +2 pi k 3 / N (y lags x) to within the estimate's scatter."""
    _, _, _, same = _case(lib, n, kmax, nw, overlap, "same", 0)
    assert (same.sxx > 0).all() and np.abs(same.coh - 1.0).max() < 1e-12
    for name in ("silence", "x_only"):
        _, _, _, ref = _case(lib, n, kmax, nw, overlap, name, 0)
        assert (ref.coh == 0).all()
    _, _, _, d3 = _case(lib, n, kmax, nw, overlap, "delay3", 0)
    k = n // 16
    want = 2 * np.pi * k * 3 / n
    assert 0 < want < np.pi / 2
    got = np.angle(d3.sxy[-1, k])
    assert abs(got - want) < 0.2 and got > 0, (got, want)


@pytest.mark.parametrize("n,kmax,nw,overlap", CASES)
def test_line_premise_in_float64(lib, n, kmax, nw, overlap):
    """Why the device test asserts nothing about WHERE the coherence peaks on the 'line' input.  A common line 40 dB under the
    independent noise of each channel has, in its own bin, a line-to-noise ratio of about -40 dB + 10 log10(N / (4 NW)): -21, -20
    and -19 dB at these sizes, still -7 dB at N = 8192 with NW = 2.5.  A single frame's K-taper coherence of such a bin is that
    of independent noise (mean 1 / K), so in float64 the line's bin is neither the row's largest coh64 nor >= 0.9: measured on the
    last frame, 0.21 against a row maximum of 0.997 at N = 256 (2 tapers), 0.02 against 0.71 at N = 8192 (8 tapers).  With the
    levels the other way round (noise 40 dB under the line) every bin inside the tapers' band 2 NW has coh64 = 1 - O(1e-6) and the
    maximum wanders over +-2 bins with the draw.  So the premise does not hold in float64, the device assertion that leaned on it
    is not made, and the line input is held to the bin-by-bin rule like every other.  What is asserted here is the fact itself."""
    _, _, _, ref = _case(lib, n, kmax, nw, overlap, "line", 0)
    kl = E.line_bin(n)
    settled = ref.coh[2:]
    assert (settled[:, kl] < 0.9).any() and (settled.max(axis=1) > settled[:, kl]).any()


# ---- inputs keyed to the grid's passes (tests/_grid_passes.py): the GPU module's two-pass cases at three sizes
# (n, kmax, nw, overlap): 16, 2 and 1 frames a block
PASS_CASES = [(256, 1, 2.0, 0.5), (2048, 4, 2.5, 0.0), (4096, 1, 2.0, 0.75)]


def _pass_case(lib, n, kmax, nw, overlap, name):
    import _grid_passes as G
    key = ("pass", n, kmax, overlap, name)
    if key not in _memo:
        frames = G.TWO_PASS_FRAMES[n]
        p = G.passes("spectro16cx", n, frames)
        tapers, sig = lib.make_dpss(n, kmax, nw)
        xy = E.make_pass_input(name, n, _hop(n, overlap), frames, 0, p.stride)
        _memo[key] = (xy, tapers, sig, E.cross64(xy, n, overlap, tapers, sig), p)
    return _memo[key]


def silent_x_frames(xy, n, overlap, hist=0):
    return np.flatnonzero((E.silence_bits(xy, n, overlap, hist) & 1) == 0)


def exact_zeros_hold(got, frames):
    return all((np.asarray(a)[frames] == 0).all() for a in (got.sxx, got.coh, got.sxy.real, got.sxy.imag))


@pytest.mark.parametrize("n,kmax,nw,overlap", PASS_CASES)
@pytest.mark.parametrize("name", E.PASS_INPUTS)
def test_state_of_the_frame_one_pass_earlier_is_rejected(lib, n, kmax, nw, overlap, name):
    """On the inputs keyed to the passes: the float32 stand-ins (the module's, and the packed one that separates the channels as
    the kernel does) pass the rule with the module's tau and keep the exact zeros; a stand-in that decides by the SILENCE BITS of
    the frame one grid pass earlier does not.  x_early: it zeroes Sxx of frames that hold x (line 1 of the rule, every bin).
    x_late: it stores the packed transform's rounding where x is silent, so coh != 0 on bins with a b = 0 (fraction inf) and the
    exact zeros are gone.  apart_by_pass has both bits set in every frame, so stale bits change nothing there; what it is for is
    the rest of the carried state -- sums that run on from the frame one pass earlier (a missing reset), or that frame's samples
    (a prefetch that was not renewed): either puts the loud channel's level on a channel 60 dB down."""
    xy, tapers, sig, ref, p = _pass_case(lib, n, kmax, nw, overlap, name)
    assert p.npasses == 2
    tau = K.tau_of(E.cross32(xy, n, overlap, tapers, sig), ref)
    assert K.FLOOR * K.MARGIN <= tau < 1e-5, tau
    honest = E.cross32_packed(xy, n, overlap, tapers, sig)
    K.check(honest, ref, tau, "%s n=%d packed stand-in" % (name, n))
    quiet = silent_x_frames(xy, n, overlap)
    assert exact_zeros_hold(honest, quiet) and exact_zeros_hold(ref, quiet)
    bits = E.silence_bits(xy, n, overlap)
    if name == "apart_by_pass":
        assert (bits == 3).all() and len(quiet) == 0
        run_on = [np.concatenate([a[:p.stride], a[p.stride:] + a[:len(a) - p.stride]]) for a in honest[:3]]
        for what, got in (("sums that run on", E.Cross(*run_on, E._coh(*run_on))),
                          ("samples not renewed", E.Cross(*(E.one_pass_earlier(a, p.stride) for a in honest)))):
            f = K.fraction(got, ref, tau)
            print("stale %-20s %s n=%d fraction of the bound %.3g" % (what, name, n, f))
            assert f > 100.0, (what, f)
        # the levels do what the input is for: the frames of pass 1 have the channels the other way round, 60 dB apart
        px, py = ref.sxx.sum(axis=1), ref.syy.sum(axis=1)
        inner = lambda a, b: slice(a + n // _hop(n, overlap), b)           # (past the frames that overlap into the other pass)
        assert (px[inner(0, p.stride)] > 1e5 * py[inner(0, p.stride)]).all() and (py[inner(p.stride, None)] > 1e5 * px[inner(p.stride, None)]).all()
        return
    assert len(quiet) >= p.fpb and ((bits & 1) != 0).sum() >= p.fpb
    assert len(set(p.pass_of[quiet])) == 1                                  # silence is one pass's; the other holds x
    stale = E.cross32_packed(xy, n, overlap, tapers, sig, bits=E.one_pass_earlier(bits, p.stride))
    f = K.fraction(stale, ref, tau)
    print("stale silence bits %s n=%d fraction of the bound %.3g, exact zeros %s" % (name, n, f, exact_zeros_hold(stale, quiet)))
    assert f > 1.0, f
    if name == "x_late":
        assert not exact_zeros_hold(stale, quiet)
    else:
        miss = np.abs(np.sqrt(stale.sxx) - np.sqrt(ref.sxx)) > tau * np.sqrt((ref.sxx + ref.syy).sum(axis=1, keepdims=True))
        assert miss[p.stride + n // _hop(n, overlap):].mean() > 0.9          # nearly every bin of the frames that hold x


def _replace(ref, **kw):
    return ref._replace(**kw)


def _mutations(lib, n, kmax, nw, overlap):
    xy, tapers, sig, ref = _case(lib, n, kmax, nw, overlap, "line", 0)
    kl = E.line_bin(n)
    out = {}
    out["sxy conjugated"] = _replace(ref, sxy=np.conj(ref.sxy))
    out["channels exchanged"] = E.Cross(ref.syy, ref.sxx, np.conj(ref.sxy), ref.coh)
    out["last taper dropped"] = E.cross64(xy, n, overlap, tapers, sig, ntap=kmax)
    out["unit weights"] = E.cross64(xy, n, overlap, tapers, sig, weights=np.ones(kmax + 1))
    fr = ref                                     # y + 1e-5 x, carried through in float64: the float32 input cannot hold it
    sxy_leak = fr.sxy + 1e-5 * fr.sxx
    syy_leak = fr.syy + 2e-5 * fr.sxy.real + 1e-10 * fr.sxx
    out["1e-5 leak of x into y"] = E.Cross(fr.sxx, syy_leak, sxy_leak, E._coh(fr.sxx, syy_leak, sxy_leak))
    unw = E.cross64(xy, n, overlap, tapers, sig, weights=np.ones(kmax + 1))
    out["coh from unweighted sums"] = _replace(ref, coh=unw.coh)
    out["sxy of the adjacent frame"] = _replace(ref, sxy=np.roll(ref.sxy, 1, axis=0))
    coh12 = ref.coh.copy()
    coh12[:, kl] = np.minimum(coh12[:, kl] * 1.2, 1.0)
    out["coh scaled by 1.2 at the line"] = _replace(ref, coh=coh12)
    tau = K.tau_of(E.cross32(xy, n, overlap, tapers, sig), ref)
    return ref, tau, out


def _peak_1e5_passes(got, ref):
    for g, r in zip(got, ref):
        if np.abs(np.asarray(g) - r).max() > 1e-5 * np.abs(r).max():
            return False
    return True


@pytest.mark.parametrize("n,kmax,nw,overlap", CASES)
def test_mutations_are_rejected(lib, n, kmax, nw, overlap):
    """Each wrong row set misses the rule on every line case.  Fractions of the bound at N = 256 / 512 / 1024: the 1e-5 leak is
    the narrowest at 4.5 / 2.3 / 1.4 (the bound is relative to the frame's total amplitude A, which grows with N against a bin's
    own), every other mutation is beyond 100.  A peak-normalised 1e-5 lets none of the eight through on these inputs either (the
    leak moves Sxy by 1e-5 Sxx, which is more than 1e-5 of the peak of |Sxy| between nearly independent channels): what the rule
    adds over it is the bound in the weak bins, which whole-row mutations do not exercise."""
    ref, tau, muts = _mutations(lib, n, kmax, nw, overlap)
    K.check(ref, ref, tau, "float64 itself")
    for what, got in muts.items():
        f = K.fraction(got, ref, tau)
        print("mutation %-32s n=%-5d fraction of the bound %10.3g   peak-normalised 1e-5 %s" %
              (what, n, f, "lets it through" if _peak_1e5_passes(got, ref) else "rejects it"))
        assert f > 1.0, (what, n, f)
