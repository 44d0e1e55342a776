"""Spectrogram.adaptive on the GPU: every bin of every frame under the rules of tests/_adaptive_check.py, the bit-for-bit
equalities of the entry's forms, its refusals, and the weak line beside a carrier that the fixed-weight row does not show.

The smallest shapes where the kernel can go wrong: every supported N with 2, 5 and 8 tapers (an odd count ends with a lone taper),
overlaps 0, 0.5, 0.75 and an odd hop, the three sample formats at an odd sample offset, both history modes, and enough frames that
a block's frame groups end with a partly filled one and the first frames reach into history.  Every case's fraction of its bound
goes to the file GLFER_ADAPTIVE_ROWS_OUT names (profiles/adaptive_rows.txt is such a run).

Past one pass of the persistent grid (tests/_grid_passes.py): every size once more with 71 units of work on a grid of 64, on noise
and on level_by_pass streams (tests/_adaptive_exact.py: sigma2 steps by 60 dB, or to and from silence, where a block goes from one
frame group to its next), then 64 and 40 streams sharing the grid over three and two passes, bit for bit.  Their record lines begin
with 'past-one-pass' (profiles/rows_past_one_pass.txt)."""
import os

import numpy as np
import pytest

import _adaptive_check as K
import _adaptive_exact as X
import _grid_passes as G
from test_adaptive_criterion import LINE_KMAX, LINE_SIZES, LINE_W, PASS_GRID, full_frames, line_found, pass_inputs_of, pass_stream
from test_adaptive_host import device_entry_refusals

pytestmark = pytest.mark.gpu

SIZES = (256, 512, 1024, 2048, 4096)
TAPERS = ((1, 2.0), (4, 2.5), (7, 4.5))                       # (kmax, w): K = 2, 5, 8
OVERLAPS = (0.0, 0.5, 0.75, 0.3)                              # 0.3: a hop that is no sixteenth of N
FMTS = ("f32", "s16", "u8")
FRAMES = {256: 19, 512: 11, 1024: 9, 2048: 7, 4096: 6}        # a partly filled last group of 4096 / N frames
TONES = ("line", "line_on_bin", "edge_tones")
OTHERS = tuple(i for i in X.INPUTS if i not in ("noise", "line"))
RECORDS = []


def _grid():
    out = []
    for a, n in enumerate(SIZES):
        for b, (kmax, w) in enumerate(TAPERS):
            i = 3 * a + b
            # noise and the line at every case, the other inputs in turn: each is seen at three or more shapes
            inputs = ("noise", "line", OTHERS[(2 * i) % len(OTHERS)], OTHERS[(2 * i + 1) % len(OTHERS)])
            out.append((n, kmax, w, OVERLAPS[i % 4], (i // 2) % 2, FMTS[i % 3], inputs))
    return out


def _params(lib, n, kmax, w, overlap, hm, fmt):
    return lib.MtmParams(n=n, overlap=overlap, w=w, kmax=kmax, history_mode=hm,
                         sample_format={"f32": lib.SAMPLES_F32, "s16": lib.SAMPLES_S16, "u8": lib.SAMPLES_U8}[fmt])


def _to_device(x32, fmt, offset=3):
    """The stream in its sample format on the GPU, at an odd sample offset inside a larger allocation."""
    import torch
    q = X.quantise(x32, fmt)
    buf = torch.zeros(len(q) + offset + 5, dtype=torch.from_numpy(q[:1]).dtype, device="cuda:0")
    buf[offset:offset + len(q)] = torch.from_numpy(q).to("cuda:0")
    return buf[offset:offset + len(q)]


@pytest.fixture(scope="module", autouse=True)
def _records_file():
    yield
    path = os.environ.get("GLFER_ADAPTIVE_ROWS_OUT")
    if path and RECORDS:
        with open(path, "w") as f:
            f.write("\n".join(RECORDS) + "\n")


@pytest.mark.parametrize("case", _grid(), ids=lambda c: "n%d_k%d_ov%g_hm%d_%s" % (c[0], c[1] + 1, c[3], c[4], c[5]))
def test_rows_under_both_rules(lib, case):
    n, kmax, w, overlap, hm, fmt, inputs = case
    tapers, sig = lib.make_dpss(n, kmax, w)
    lam, beta = lib.adaptive_weights(_params(lib, n, kmax, w, overlap, hm, fmt))
    sp = lib.Spectrogram(_params(lib, n, kmax, w, overlap, hm, fmt))
    nframes = FRAMES[n]
    for name in inputs:
        x = X.make_input(name, n, nframes * sp.hop + 3, 11, fmt, w)
        E64, s2 = X.eigen64(x, n, overlap, tapers, hm)
        assert E64.shape[0] == nframes
        _, dof32_1, E32 = X.adaptive32(x, n, overlap, tapers, lam, beta, 1, hm)
        tau = K.eigen_tau(E32, E64)
        widen = K.start_dof_widen(dof32_1, E64, lam, beta, s2, n)
        xd = _to_device(x, fmt)
        memo = {}

        def device(iters):
            if iters not in memo:
                r = sp.adaptive(xd, iters=iters)
                memo[iters] = (r.psd.cpu().numpy(), r.dof.cpu().numpy())
            return memo[iters]
        fa = fd = 0.0
        for m in (0, 1, 7, 31) if name in TONES else (0, 1, 7):
            a, d = K.chained(None if m == 0 else device(m)[0], device(m + 1)[0], device(m + 1)[1], E64, lam, beta, s2, n, tau,
                             dof_widen=widen)
            fa, fd = max(fa, a), max(fd, d)
        rec = "n=%-5d K=%d w=%.1f ov=%-4g hm=%d %-3s %-13s tau %.3g  chained: amp %.3f dof %.3f (m=0 dof term x %.2f)" % (
            n, kmax + 1, w, overlap, hm, fmt, name, tau, fa, fd, widen)
        if name in X.NOISE_LIKE:
            psd32 = X.adaptive32(x, n, overlap, tapers, lam, beta, 8, hm)[0]
            taup, want = K.end_to_end_tau(psd32, E32, E64, lam, beta, s2, n, 8)
            rec += "  end-to-end: tau' %.3g, %.3f" % (taup, K.end_to_end(device(8)[0], want, E64, taup))
        if name == "silence":
            assert (device(8)[0] == 0).all() and np.isfinite(device(8)[1]).all()
        if name == "silent_frame":
            quiet = np.flatnonzero(s2 == 0)
            assert len(quiet) >= 1 and (device(8)[0][quiet] == 0).all() and np.isfinite(device(8)[1][quiet]).all()
        print(rec)
        RECORDS.append(rec)
    sp.close()


# ---- past one pass of the grid: 71 units of work on a grid of 64, seven blocks run a second frame group (tests/_grid_passes.py)
def _pass_params():
    return [(i, name) for i in range(len(PASS_GRID)) for name in ("noise",) + pass_inputs_of(i)]


@pytest.mark.parametrize("i,name", _pass_params(), ids=lambda v: v if isinstance(v, str) else "n%d_k%d" % (PASS_GRID[v][0], PASS_GRID[v][1] + 1))
def test_rows_past_one_pass_under_both_rules(lib, i, name):
    """Every bin of every frame of both passes: the chained rule at m = 0, 1, 7 on noise and on two level_by_pass streams per
    size (sigma2 of a frame and of the one its block handled a pass earlier differ by 60 dB, or one of them is silence), the
    end-to-end rule on noise; psd == 0 and a finite dof in the silent frames."""
    case = PASS_GRID[i]
    n, kmax, w, overlap, hm, fmt = case
    x, p = pass_stream(case, name)
    assert p.grid == 64 and p.npasses == 2
    tapers, sig = lib.make_dpss(n, kmax, w)
    lam, beta = lib.adaptive_weights(_params(lib, *case))
    E64, s2 = X.eigen64(x, n, overlap, tapers, hm)
    assert E64.shape[0] == len(p.pass_of)
    _, dof32_1, E32 = X.adaptive32(x, n, overlap, tapers, lam, beta, 1, hm)
    tau = K.eigen_tau(E32, E64)
    widen = K.start_dof_widen(dof32_1, E64, lam, beta, s2, n)
    sp = lib.Spectrogram(_params(lib, *case))
    xd = _to_device(x, fmt)
    memo = {}

    def device(iters):
        if iters not in memo:
            r = sp.adaptive(xd, iters=iters)
            memo[iters] = (r.psd.cpu().numpy(), r.dof.cpu().numpy())
        return memo[iters]
    fa = fd = 0.0
    for m in (0, 1, 7):
        a, d = K.chained(None if m == 0 else device(m)[0], device(m + 1)[0], device(m + 1)[1], E64, lam, beta, s2, n, tau, dof_widen=widen)
        fa, fd = max(fa, a), max(fd, d)
    rec = "past-one-pass n=%-5d K=%d w=%.1f ov=%-4g hm=%d %-3s %-13s tau %.3g  chained: amp %.3f dof %.3f (m=0 dof term x %.2f)" % (
        n, kmax + 1, w, overlap, hm, fmt, name, tau, fa, fd, widen)
    if name == "noise":
        psd32 = X.adaptive32(x, n, overlap, tapers, lam, beta, 8, hm)[0]
        taup, want = K.end_to_end_tau(psd32, E32, E64, lam, beta, s2, n, 8)
        rec += "  end-to-end: tau' %.3g, %.3f" % (taup, K.end_to_end(device(8)[0], want, E64, taup))
    else:
        quiet = np.flatnonzero(s2 == 0)
        assert len(quiet) >= p.fpb or "gap" not in name
        for it in (1, 8):
            assert (device(it)[0][quiet] == 0).all() and np.isfinite(device(it)[1]).all()
    sp.close()
    print(rec)
    RECORDS.append(rec)


@pytest.mark.parametrize("nb", [G.BATCH_MULTIPLE_OF_8, G.BATCH_OTHER])
@pytest.mark.parametrize("i", (0, 3, 4))
def test_batch_past_one_pass_bit_for_bit(lib, i, nb):
    """N = 256 (16 frames a block), 2048 (128 lanes a frame) and 4096: 64 streams share the grid at 32 workgroups each, a multiple
    of 8, and make three passes; 40 streams at 52, no multiple of 8, make two.  The streams lie one pass apart in one level_by_pass
    buffer laid out for the BATCH's pass boundaries, so that stream b begins with level b mod 3 of its order and all of
    1 -> 1e-3 -> 0, 1e-3 -> 0 -> 1 and 0 -> 1 -> 1e-3 appear.  Every stream's rows are the bits of the single-stream call (the
    two-pass launch held to float64 above), and the first, the middle and the last stream's the bits of range calls of at most 60
    units of work, each a single pass."""
    import torch
    case = PASS_GRID[i]
    n, kmax, w, overlap, hm, fmt = case
    frames = G.TWO_PASS_FRAMES[n]
    p = G.passes("spectro16a", n, frames, nb)
    assert p.npasses >= (3 if nb == G.BATCH_MULTIPLE_OF_8 else 2) and (p.grid % 8 == 0) == (nb == G.BATCH_MULTIPLE_OF_8)
    sp = lib.Spectrogram(_params(lib, *case))
    S = frames * sp.hop + 3
    name = pass_inputs_of(i)[nb % 2]
    x = X.level_by_pass(name, n, sp.hop, (nb - 1) * p.stride * sp.hop + S, 17, p.stride, fmt, w)
    big = _to_device(x, fmt)
    v = big.as_strided((nb, S), (p.stride * sp.hop, 1), big.storage_offset())
    got = sp.adaptive_batch(v, iters=8)
    assert got.psd.shape == (nb, frames, n // 2 + 1)
    for b in range(nb):
        one = sp.adaptive(v[b], iters=8)
        assert _same(got.psd[b], one.psd) and _same(got.dof[b], one.dof), b
    for b in (0, nb // 2, nb - 1):
        for first in range(0, frames, 60 * p.fpb):
            cnt = min(60 * p.fpb, frames - first)
            part = sp.adaptive(v[b], first_frame=first, nframes=cnt, iters=8)
            assert _same(part.psd, got.psd[b, first:first + cnt]) and _same(part.dof, got.dof[b, first:first + cnt]), (b, first)
    sp.close()


@pytest.mark.parametrize("n", LINE_SIZES)
def test_weak_line_beside_a_carrier(lib, n):
    """The cases tests/test_adaptive_criterion.py proved in float64: the adaptive row shows the weak line as its largest bin outside
    the carrier's +-2 ceil(w) bins, the fixed-weight row of run() on the same plan does not."""
    fmt = FMTS[SIZES.index(n) % 3]
    for name, overlap in (("line", 0.5), ("line_on_bin", 0.75)):
        sp = lib.Spectrogram(_params(lib, n, LINE_KMAX, LINE_W, overlap, 0, fmt))
        x = X.make_input(name, n, 8 * sp.hop + 3, 5, fmt, LINE_W)
        xd = _to_device(x, fmt)
        S = sp.adaptive(xd, iters=8, want=("psd",)).psd.cpu().numpy()
        F = sp.run(xd).cpu().numpy()
        for f in full_frames(n, overlap, S.shape[0]):
            assert line_found(S[f], n, LINE_W), (name, f)
            assert not line_found(F[f], n, LINE_W), (name, f)
        sp.close()


def _plan_and_stream(lib, n=1024, kmax=4, w=2.5, overlap=0.75, hm=0, fmt="s16", frames=13, name="line", seed=3):
    sp = lib.Spectrogram(_params(lib, n, kmax, w, overlap, hm, fmt))
    x = X.make_input(name, n, frames * sp.hop + 5, seed, fmt, w)
    return sp, x, _to_device(x, fmt)


def _same(a, b):
    import torch
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("n,kmax,w", ((256, 4, 2.5), (2048, 7, 4.5), (4096, 1, 2.0)))
def test_frame_range_and_repeat_bit_for_bit(lib, n, kmax, w):
    sp, x, xd = _plan_and_stream(lib, n=n, kmax=kmax, w=w, frames=23 if n == 256 else 9)
    full = sp.adaptive(xd, iters=5)
    again = sp.adaptive(xd, iters=5)
    assert _same(full.psd, again.psd) and _same(full.dof, again.dof)            # iters = m obtained twice
    nf = full.psd.shape[0]
    for first, cnt in ((0, 1), (2, nf - 2), (nf - 3, 3), (1, 4)):
        part = sp.adaptive(xd, first_frame=first, nframes=cnt, iters=5)
        assert _same(part.psd, full.psd[first:first + cnt]) and _same(part.dof, full.dof[first:first + cnt]), (first, cnt)
    sp.close()


@pytest.mark.parametrize("fmt", FMTS)
def test_batch_of_unlike_streams_bit_for_bit(lib, fmt):
    import torch
    sp = lib.Spectrogram(_params(lib, 512, 4, 2.5, 0.5, 1, fmt))
    ns = 11 * sp.hop + 7
    xs = [X.make_input(name, 512, ns, 21 + i, fmt, 2.5) for i, name in enumerate(("noise", "line", "silence", "impulses", "dc"))]
    q = np.stack([X.quantise(x, fmt) for x in xs])
    wide = torch.zeros((len(xs), ns + 9), dtype=torch.from_numpy(q[:1]).dtype, device="cuda:0")   # stride(0) above the length
    wide[:, 1:1 + ns] = torch.from_numpy(q).to("cuda:0")
    batch = wide[:, 1:1 + ns]
    got = sp.adaptive_batch(batch, iters=6)
    for b in range(len(xs)):
        one = sp.adaptive(batch[b].contiguous(), iters=6)
        assert _same(got.psd[b], one.psd) and _same(got.dof[b], one.dof), b
    part = sp.adaptive_batch(batch, first_frame=3, nframes=5, iters=6, want=("dof",))
    assert part.psd is None and _same(part.dof, got.dof[:, 3:8].contiguous())
    sp.close()


def test_pitched_rows_between_sentinels_and_want_subsets(lib):
    import torch
    sp, x, xd = _plan_and_stream(lib, n=1024, kmax=7, w=4.5, overlap=0.5, hm=1, fmt="f32", frames=9, name="two_level")
    full = sp.adaptive(xd, iters=8)
    nf, bins, pitch = full.psd.shape[0], sp.n // 2 + 1, sp.n // 2 + 1 + 11
    for want in (("psd",), ("dof",), ("dof", "psd")):
        r = sp.adaptive(xd, iters=8, want=want)
        assert (r.psd is None) == ("psd" not in want) and (r.dof is None) == ("dof" not in want)
        assert r.psd is None or _same(r.psd, full.psd)
        assert r.dof is None or _same(r.dof, full.dof)
    sent = -7.5
    bp = torch.full((nf, pitch), sent, device="cuda:0")
    bd = torch.full((nf, pitch), sent, device="cuda:0")
    r = sp.adaptive(xd, iters=8, out={"psd": bp[:, :bins], "dof": bd[:, :bins]})
    assert _same(bp[:, :bins].contiguous(), full.psd) and _same(bd[:, :bins].contiguous(), full.dof)
    assert (bp[:, bins:] == sent).all() and (bd[:, bins:] == sent).all()
    sp.close()


def test_captured_graph_replay_bit_for_bit(lib):
    import torch
    sp, x, xd = _plan_and_stream(lib, n=2048, kmax=4, w=2.5, overlap=0.5, hm=0, fmt="f32", frames=7, name="noise")
    eager = sp.adaptive(xd, iters=8)
    out = {"psd": torch.zeros_like(eager.psd), "dof": torch.zeros_like(eager.dof)}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        sp.adaptive(xd, iters=8, out=out)                                       # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    out["psd"].zero_()
    out["dof"].zero_()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        sp.adaptive(xd, iters=8, out=out)
    g.replay()
    torch.cuda.synchronize()
    assert _same(out["psd"], eager.psd) and _same(out["dof"], eager.dof)
    sp.close()


def test_refusals_with_plans(lib):
    assert device_entry_refusals(lib) == 11
    sp = lib.Spectrogram(lib.MtmParams(n=512, w=2.5, kmax=4))
    with pytest.raises(lib.GlferHipError):
        sp.adaptive(_to_device(np.zeros(4 * 512, np.float32), "f32"), iters=65)
    sp.close()
