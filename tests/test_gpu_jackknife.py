"""Spectrogram.jackknife on the GPU: every bin of every frame under the rule of tests/_jackknife_check.py on the grid
tests/test_jackknife_criterion.py proved the stand-in on, the bit-for-bit equalities of the entry's forms, its refusals, and the
interval helper.

The grid: every built N -- 256 (16 lanes a frame, 16 frames a block) to 2048 and 4096 (a frame spans 2 and 4 wavefronts) -- with
2, 5 (odd: the lone taper) and 8 tapers, 37 frames (a partly filled last frame group), overlaps 0 and 75 %, f32 / s16 / u8 at an odd
sample offset, both history modes, sweep counts 0, 2 and 8 (1 and 7 for the chain), seven inputs.  Every case's fraction of its
bound and its excluded share go to the file GLFER_JACKKNIFE_ROWS_OUT names (profiles/jackknife_rows.txt is such a run).

Past one pass of the persistent grid: tests/test_gpu_adaptive.py's two-pass cases and shared-grid batches for this entry; their
record lines begin with 'past-one-pass' (profiles/rows_past_one_pass.txt)."""
import os

import numpy as np
import pytest

import _adaptive_exact as X
import _grid_passes as G
from test_adaptive_criterion import PASS_GRID, pass_inputs_of
from test_jackknife_criterion import CASE_ID, GRID, INPUTS, Case, check_case, pass_case
from test_jackknife_host import device_entry_refusals

pytestmark = pytest.mark.gpu

FMTS = ("f32", "s16", "u8")
RECORDS = []


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


def _same(a, b):
    import torch
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.fixture(scope="module", autouse=True)
def _records_file():
    yield
    path = os.environ.get("GLFER_JACKKNIFE_ROWS_OUT")
    if path and RECORDS:
        with open(path, "w") as f:
            f.write("\n".join(RECORDS) + "\n")


@pytest.mark.parametrize("case", GRID, ids=CASE_ID)
def test_rows_under_the_rule(lib, case):
    n, kmax, w, overlap, hm, fmt = case
    assert lib.jackknife_supported(_params(lib, *case))
    sp = lib.Spectrogram(_params(lib, *case))
    for name in INPUTS:
        c = Case(lib, case, name)
        xd = _to_device(c.x, fmt)
        memo = {}

        def device(iters):
            if iters not in memo:
                r = sp.jackknife(xd, iters=iters)
                memo[iters] = (r.psd.cpu().numpy(), r.dof.cpu().numpy(), r.logvar.cpu().numpy())
                if iters >= 1:                                   # psd and dof: the bits of adaptive() at the same sweep count
                    a = sp.adaptive(xd, iters=iters)
                    assert _same(r.psd, a.psd) and _same(r.dof, a.dof), (name, iters)
            return memo[iters]
        rec = check_case(c, device)
        print(rec)
        RECORDS.append(rec)
    sp.close()


# ---- past one pass of the grid: tests/test_gpu_adaptive.py's cases through check_case
def _pass_params():
    return [(i, name) for i in range(len(PASS_GRID)) for name in ("noise",) + pass_inputs_of(i)]


@pytest.mark.parametrize("i,name", _pass_params(), ids=lambda v: v if isinstance(v, str) else CASE_ID(PASS_GRID[v]))
def test_rows_past_one_pass_under_the_rule(lib, i, name):
    """71 units of work on a grid of 64: every bin of every frame of both passes under the rule at iters 0, 2 and 8 (and 0 and 8
    are the sweep counts the issue names), psd and dof the bits of adaptive() -- whose rows tests/test_gpu_adaptive.py holds to the
    chained rule on the same streams: with two tapers, and in silent frames, that equality is what sees a stale sigma2
    (tests/test_jackknife_criterion.py)."""
    case = PASS_GRID[i]
    assert lib.jackknife_supported(_params(lib, *case))
    if name in X.PASS_INPUTS:
        c, p = pass_case(lib, case, name)
    else:
        c, p = Case(lib, case, name, frames=G.TWO_PASS_FRAMES[case[0]]), G.passes("spectro16a", case[0], G.TWO_PASS_FRAMES[case[0]])
    assert p.grid == 64 and p.npasses == 2
    sp = lib.Spectrogram(_params(lib, *case))
    xd = _to_device(c.x, case[5])
    memo = {}

    def device(iters):
        if iters not in memo:
            r = sp.jackknife(xd, iters=iters)
            memo[iters] = (r.psd.cpu().numpy(), r.dof.cpu().numpy(), r.logvar.cpu().numpy())
            if iters >= 1:
                a = sp.adaptive(xd, iters=iters)
                assert _same(r.psd, a.psd) and _same(r.dof, a.dof), (name, iters)
        return memo[iters]
    rec = "past-one-pass " + check_case(c, device)
    quiet = np.flatnonzero(c.s2 == 0)
    for it in (0, 8):
        assert (device(it)[0][quiet] == 0).all() and (device(it)[2][quiet] == 0).all() and np.isfinite(device(it)[1]).all()
    sp.close()
    print(rec)
    RECORDS.append(rec)


@pytest.mark.parametrize("nb", [G.BATCH_MULTIPLE_OF_8, G.BATCH_OTHER])
@pytest.mark.parametrize("i", (0, 3, 4))
def test_batch_past_one_pass_bit_for_bit(lib, i, nb):
    """tests/test_gpu_adaptive.py::test_batch_past_one_pass_bit_for_bit for the jackknife entry, iters 0 and 8: three passes on
    grids of 32 (a multiple of 8) with 64 streams, two on grids of 52 with 40; streams one pass apart in one level_by_pass buffer;
    every stream against the single-stream two-pass call, three streams against range calls of a single pass each."""
    import torch  # noqa: F401
    case = PASS_GRID[i]
    n, kmax, w, overlap, hm, fmt = case
    frames = G.TWO_PASS_FRAMES[n]
    p = G.passes("spectro16a", n, frames, nb)
    assert p.npasses >= (3 if nb == G.BATCH_MULTIPLE_OF_8 else 2) and (p.grid % 8 == 0) == (nb == G.BATCH_MULTIPLE_OF_8)
    sp = lib.Spectrogram(_params(lib, *case))
    S = frames * sp.hop + 3
    name = pass_inputs_of(i)[(nb + 1) % 2]
    big = _to_device(X.level_by_pass(name, n, sp.hop, (nb - 1) * p.stride * sp.hop + S, 19, p.stride, fmt, w), fmt)
    v = big.as_strided((nb, S), (p.stride * sp.hop, 1), big.storage_offset())
    for iters in (0, 8):
        got = sp.jackknife_batch(v, iters=iters)
        assert got.logvar.shape == (nb, frames, n // 2 + 1)
        for b in range(nb):
            assert _all_same(lib.Jackknife(*(t[b] for t in got)), sp.jackknife(v[b], iters=iters)), (iters, b)
        for b in (0, nb // 2, nb - 1):
            for first in range(0, frames, 60 * p.fpb):
                cnt = min(60 * p.fpb, frames - first)
                part = sp.jackknife(v[b], first_frame=first, nframes=cnt, iters=iters)
                assert _all_same(part, lib.Jackknife(*(t[b, first:first + cnt].contiguous() for t in got))), (iters, b, first)
    sp.close()


def _plan_and_stream(lib, n=1024, kmax=4, w=2.5, overlap=0.75, hm=0, fmt="s16", frames=13, name="line", seed=3):
    sp = lib.Spectrogram(_params(lib, n, kmax, w, overlap, hm, fmt))
    x = X.make_input(name, n, frames * sp.hop + 5, seed, fmt, w)
    return sp, x, _to_device(x, fmt)


def _all_same(a, b):
    return _same(a.psd, b.psd) and _same(a.dof, b.dof) and _same(a.logvar, b.logvar)


@pytest.mark.parametrize("n,kmax,w", ((256, 4, 2.5), (2048, 7, 4.5), (4096, 1, 2.0)))
def test_frame_range_and_repeat_bit_for_bit(lib, n, kmax, w):
    sp, x, xd = _plan_and_stream(lib, n=n, kmax=kmax, w=w, frames=37 if n == 256 else 9)
    for iters in (0, 5):
        full = sp.jackknife(xd, iters=iters)
        again = sp.jackknife(xd, iters=iters)                                    # two calls in a row
        assert _all_same(full, again)
        nf = full.psd.shape[0]
        for first, cnt in ((0, 1), (2, nf - 2), (nf - 3, 3), (1, 4)):
            part = sp.jackknife(xd, first_frame=first, nframes=cnt, iters=iters)
            assert _all_same(part, lib.Jackknife(*(t[first:first + cnt].contiguous() for t in full))), (iters, first, cnt)
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
    for iters in (0, 6):
        got = sp.jackknife_batch(batch, iters=iters)
        for b in range(len(xs)):
            one = sp.jackknife(batch[b].contiguous(), iters=iters)
            assert _all_same(lib.Jackknife(*(t[b] for t in got)), one), (iters, b)
        part = sp.jackknife_batch(batch, first_frame=3, nframes=5, iters=iters, want=("logvar",))
        assert part.psd is None and part.dof is None and _same(part.logvar, got.logvar[:, 3:8].contiguous())
    sp.close()


def test_pitched_rows_between_sentinels_and_want_subsets(lib):
    import torch
    sp, x, xd = _plan_and_stream(lib, n=1024, kmax=7, w=4.5, overlap=0.5, hm=1, fmt="f32", frames=9, name="two_level")
    full = sp.jackknife(xd, iters=8)
    nf, bins, pitch = full.psd.shape[0], sp.n // 2 + 1, sp.n // 2 + 1 + 11
    fields = lib.Jackknife._fields
    for mask in range(1, 8):                                                     # every subset of the three outputs
        want = tuple(f for i, f in enumerate(fields) if mask >> i & 1)
        r = sp.jackknife(xd, iters=8, want=want[::-1])
        for f in fields:
            assert (getattr(r, f) is None) == (f not in want), (want, f)
            assert getattr(r, f) is None or _same(getattr(r, f), getattr(full, f)), (want, f)
    sent = -7.5
    bufs = {f: torch.full((nf, pitch), sent, device="cuda:0") for f in fields}
    sp.jackknife(xd, iters=8, out={f: b[:, :bins] for f, b in bufs.items()})
    for f, b in bufs.items():
        assert _same(b[:, :bins].contiguous(), getattr(full, f)), f
        assert (b[:, bins:] == sent).all(), f
    sp.close()


def test_captured_graph_replay_bit_for_bit(lib):
    import torch
    sp, x, xd = _plan_and_stream(lib, n=2048, kmax=4, w=2.5, overlap=0.5, hm=0, fmt="f32", frames=7, name="noise")
    eager = sp.jackknife(xd, iters=8)
    out = {f: torch.zeros_like(t) for f, t in eager._asdict().items()}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        sp.jackknife(xd, iters=8, out=out)                                      # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    for t in out.values():
        t.zero_()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        sp.jackknife(xd, iters=8, out=out)
    g.replay()
    torch.cuda.synchronize()
    assert all(_same(out[f], getattr(eager, f)) for f in out)
    sp.close()


def test_interval_contains_the_float64_row_on_noise(lib):
    """A sanity check of the interval helper, not a statistical claim: with eight tapers and iters = 0 the interval at 0.95 around
    the device's row contains the float64 eigenvalue-weighted mean of the same bin, in every bin."""
    case = (1024, 7, 4.5, 0.0, 0, "f32")
    params = _params(lib, *case)
    c = Case(lib, case, "noise", frames=9)
    sp = lib.Spectrogram(params)
    jk = sp.jackknife(_to_device(c.x, "f32"), iters=0)
    lo, hi = lib.jackknife_interval(jk, params, 0.95)
    assert lo.is_cuda and hi.is_cuda and lo.shape == jk.psd.shape == hi.shape
    l64 = np.asarray(c.lam, np.float32).astype(np.float64)
    S = (l64[None, :, None] * c.E64).sum(axis=1) / l64.sum()
    lo, hi, psd = lo.cpu().numpy().astype(np.float64), hi.cpu().numpy().astype(np.float64), jk.psd.cpu().numpy()
    assert (lo <= S).all() and (S <= hi).all() and (lo <= psd).all() and (psd <= hi).all()
    t = lib.jackknife_factor(params, 0.95)
    assert np.allclose(np.log(hi / lo), 2.0 * t * np.sqrt(jk.logvar.cpu().numpy().astype(np.float64)), rtol=1e-4, atol=1e-5)
    sp.close()


def test_refusals_with_plans(lib):
    assert device_entry_refusals(lib) == 11
    sp = lib.Spectrogram(lib.MtmParams(n=512, w=2.5, kmax=4))
    with pytest.raises(lib.GlferHipError):
        sp.jackknife(_to_device(np.zeros(4 * 512, np.float32), "f32"), iters=65)
    with pytest.raises(lib.GlferHipError):
        sp.jackknife(_to_device(np.zeros(4 * 512, np.float32), "f32"), iters=-1)
    with pytest.raises(lib.GlferHipError):
        sp.adaptive(_to_device(np.zeros(4 * 512, np.float32), "f32"), iters=0)     # the adaptive entry keeps refusing 0
    sp.close()
