"""Spectrogram.cross on the GPU: the auto-spectra, the cross-spectrum and the coherence of two interleaved channels, bin by bin
against float64 (tests/_cross_check.py's rule, tau from the float32 stand-in on the CPU), over every size the kernel is built for
(each its own translation unit, frames per block and prefetch depth), two, five and eight tapers, the four overlaps, the three
sample formats, both history modes and nine inputs; then bit for bit: batches against the loop, frame ranges against the whole run,
pitched outputs between sentinels, every subset of outputs against the all-four call, the refusals with real plans, one capture
and replay.

The 'line' input (a common line 40 dB under each channel's own noise) is held to the rule like the others; nothing is asserted about
where its coherence peaks, because in float64 it does not peak at the line (tests/test_cross_criterion.py::test_line_premise_in_float64).

Past one pass of the persistent grid (tests/_grid_passes.py): every size once more with 71 units of work on a grid of 64 -- seven
blocks run a second frame group, the last one partly filled -- on noise and on the inputs keyed to the pass boundaries
(tests/_cross_exact.py: x_late, x_early, apart_by_pass), bin by bin against float64 with exact zeros where x has no sample; then 64
and 40 streams sharing the grid over three and two passes and more, bit for bit against those two-pass calls and against range
calls of a single pass.  What a kernel that kept a frame group's state for its next would fail there is shown without a GPU in
tests/test_cross_criterion.py::test_state_of_the_frame_one_pass_earlier_is_rejected.

Lines starting with 'cross-rows' (run with -s) are the record kept in profiles/cross_rows.txt; those that go on with 'past-one-pass',
in profiles/rows_past_one_pass.txt."""
import collections
import functools
import itertools

import numpy as np
import pytest

import _cross_check as K
import _cross_exact as E
import _grid_passes as G
from _exact import hop_len
from test_cross_host import device_entry_refusals

pytestmark = pytest.mark.gpu
SENTINEL = -7.25
ALL = ("sxx", "syy", "sxy", "coh")
SIZES = (256, 512, 1024, 2048, 4096, 8192)
TAPERS = ((1, 2.0), (4, 2.5), (7, 4.0))                  # (kmax, nw): two, five and eight tapers
OVERLAPS = (0.0, 0.3, 0.5, 0.75)

Case = collections.namedtuple("Case", "n kmax nw ovl fmt hist frames name")


def _cases():
    out = []
    for s, n in enumerate(SIZES):
        fpb = max(1, 256 // (n // 16))                  # frames per block of the kernel at this size
        for i, name in enumerate(E.INPUTS):
            kmax, nw = TAPERS[(i + s) % 3]
            # never a multiple of the block's frames, so the clamp runs; more than one block at least once per size
            frames = fpb + 5 if i == 0 and fpb > 1 else (5 if (i + s) % 2 else 7)
            out.append(Case(n, kmax, nw, OVERLAPS[(i + 2 * s) % 4], "f32", 0, frames, name))
        for j, fmt in enumerate(("s16", "u8")):
            kmax, nw = TAPERS[(j + s + 1) % 3]
            out.append(Case(n, kmax, nw, OVERLAPS[(j + s) % 4], fmt, 0, 5, "noise"))
        kmax, nw = TAPERS[s % 3]
        out.append(Case(n, kmax, nw, OVERLAPS[1 + s % 3], ("f32", "s16", "u8")[s % 3], 1, 7, "delay3"))
    return out


CASES = _cases()


def _id(c):
    return "n%d-k%d-o%g-%s-h%d-f%d-%s" % (c.n, c.kmax + 1, c.ovl, c.fmt, c.hist, c.frames, c.name)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _plan(lib, c):
    fmt = {"f32": lib.SAMPLES_F32, "s16": lib.SAMPLES_S16, "u8": lib.SAMPLES_U8}[c.fmt]
    return lib.Spectrogram(lib.MtmParams(n=c.n, overlap=c.ovl, w=c.nw, kmax=c.kmax, history_mode=c.hist, sample_format=fmt))


_inputs = {}


def _input(c, seed=0):
    """(the stream in the plan's format, its float32 values), made once per case and left unchanged."""
    key = (c.n, c.ovl, c.fmt, c.frames, c.name, seed)
    if key not in _inputs:
        raw = E.quantise(E.make_input(c.name, c.n, c.frames * hop_len(c.n, c.ovl), seed), c.fmt)
        _inputs[key] = (raw, E.to_float32(raw, c.fmt))
    return _inputs[key]


def _host(res):
    return E.Cross(*(None if t is None else t.cpu().numpy() for t in res))


def _bits(x):
    import torch
    if x.is_complex():
        x = torch.view_as_real(x)
    return x.contiguous().view(torch.int32)


def _same(a, b):
    import torch
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _same_all(a, b):
    return all((x is None and y is None) or _same(x, y) for x, y in zip(a, b))


# ---- accuracy, bin by bin -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", CASES, ids=_id)
def test_rows_bin_by_bin(lib, torch_cuda, c):
    torch = torch_cuda
    raw, xy32 = _input(c)
    sp = _plan(lib, c)
    tapers, sig = sp.tapers()
    ref = E.cross64(xy32, c.n, c.ovl, tapers, sig, c.hist)
    tau = K.tau_of(E.cross32(xy32, c.n, c.ovl, tapers, sig, c.hist), ref)          # from the CPU alone
    got = _host(sp.cross(torch.from_numpy(raw).cuda(), want=ALL))
    torch.cuda.synchronize()
    sp.close()
    assert got.sxx.shape == (c.frames, c.n // 2 + 1) and got.sxy.dtype == np.complex64
    assert (got.sxy.imag[:, 0] == 0).all() and (got.sxy.imag[:, -1] == 0).all()    # exact zeros at DC and Nyquist
    K.check(got, ref, tau, _id(c))
    if c.name == "silence":
        for a in (got.sxx, got.syy, got.coh, got.sxy.real, got.sxy.imag):
            assert (a == 0).all()
    if c.name == "x_only":
        assert (got.coh == 0).all() and (got.syy == 0).all()
    if c.name == "delay3" and c.hist == 0:
        k = c.n // 16                                    # mid-band: 2 pi k 3 / N = 3 pi / 8
        for f in range(2, c.frames):                     # settled frames
            assert np.angle(ref.sxy[f, k]) > 0 and np.angle(got.sxy[f, k]) > 0, (f, np.angle(ref.sxy[f, k]), np.angle(got.sxy[f, k]))


# ---- past one pass of the grid ------------------------------------------------------------------------------------------
# 71 units of work on a grid of 64 (tests/_grid_passes.py): seven blocks run a second frame group, the last one partly filled
# where a block holds several frames.  Every size with noise and the three inputs keyed to the passes; taper counts, overlaps and
# formats in turn; history_mode = 1 once per size.
PASS_NAMES = ("noise",) + E.PASS_INPUTS


def _pass_cases():
    out = []
    for s, n in enumerate(SIZES):
        for i, name in enumerate(PASS_NAMES):
            kmax, nw = TAPERS[(i + s) % 3]
            fmt = (("f32", "s16", "u8")[s % 3], "f32", ("u8", "f32", "s16")[s % 3], ("f32", "s16")[s % 2])[i]
            out.append(Case(n, kmax, nw, OVERLAPS[(i + 2 * s) % 4], fmt, int(i == s % 3), G.TWO_PASS_FRAMES[n], name))
    return out


PASS_CASES = _pass_cases()


@functools.lru_cache(maxsize=None)
def _pass_reference(lib, c):
    """(raw stream, float64 rows, tau, the frames silent in x) of a case past one pass: computed once, on the CPU alone."""
    hop = hop_len(c.n, c.ovl)
    stride = G.passes("spectro16cx", c.n, c.frames).stride
    xy = E.make_pass_input(c.name, c.n, hop, c.frames, 0, stride) if c.name in E.PASS_INPUTS else E.make_input(c.name, c.n, c.frames * hop, 0)
    raw = E.quantise(xy, c.fmt)
    xy32 = E.to_float32(raw, c.fmt)
    tapers, sig = lib.make_dpss(c.n, c.kmax, c.nw)
    ref = E.cross64(xy32, c.n, c.ovl, tapers, sig, c.hist)
    tau = K.tau_of(E.cross32(xy32, c.n, c.ovl, tapers, sig, c.hist), ref)
    return raw, ref, tau, np.flatnonzero((E.silence_bits(xy32, c.n, c.ovl, c.hist) & 1) == 0)


def _check_pass_rows(got, ref, tau, quiet, what):
    assert (got.sxy.imag[:, 0] == 0).all() and (got.sxy.imag[:, -1] == 0).all()
    K.check(got, ref, tau, what)
    for a in (got.sxx, got.coh, got.sxy.real, got.sxy.imag):                       # exact zeros where x has no sample
        assert (a[quiet] == 0).all(), what
    loud = np.setdiff1d(np.arange(len(got.sxx)), quiet)
    assert (got.sxx[loud] > 0).any(axis=1).all(), what


def test_the_pass_cases_cover_the_grid():
    assert {(c.n, c.name) for c in PASS_CASES} == {(n, name) for n in SIZES for name in PASS_NAMES}
    assert {c.kmax for c in PASS_CASES} == {1, 4, 7} and {c.ovl for c in PASS_CASES} == set(OVERLAPS)
    assert {c.fmt for c in PASS_CASES} == {"f32", "s16", "u8"} and {c.hist for c in PASS_CASES} == {0, 1}
    assert not any(c.fmt == "u8" and c.name == "apart_by_pass" for c in PASS_CASES)
    for c in PASS_CASES:
        p = G.passes("spectro16cx", c.n, c.frames)
        assert p.grid == 64 and p.npasses == 2 and G.passes("spectro16cx", c.n, c.frames - 3).npasses == 2


@pytest.mark.parametrize("c", PASS_CASES, ids=_id)
def test_rows_past_one_pass_bin_by_bin(lib, torch_cuda, c):
    """Every bin of every frame of both passes against float64; the x_early case of every size once more from first_frame = 3, so
    that the second pass runs with frame0 != 0, against the same float64 rows."""
    torch = torch_cuda
    raw, ref, tau, quiet = _pass_reference(lib, c)
    sp = _plan(lib, c)
    d = torch.from_numpy(raw).cuda()
    got = _host(sp.cross(d, want=ALL))
    assert got.sxx.shape == (c.frames, c.n // 2 + 1)
    _check_pass_rows(got, ref, tau, quiet, "past-one-pass " + _id(c))
    if c.name == "x_early":
        part = _host(sp.cross(d, first_frame=3, want=ALL))
        assert part.sxx.shape == (c.frames - 3, c.n // 2 + 1)
        _check_pass_rows(part, E.Cross(*(a[3:] for a in ref)), tau, quiet[quiet >= 3] - 3, "past-one-pass first_frame=3 " + _id(c))
    sp.close()


def _chunks(total, size):
    return [(a, min(size, total - a)) for a in range(0, total, size)]


@pytest.mark.parametrize("nb", [G.BATCH_MULTIPLE_OF_8, G.BATCH_OTHER])
@pytest.mark.parametrize("n,kmax,nw,ovl,fmt", [(256, 4, 2.5, 0.5, "f32"), (2048, 1, 2.0, 0.75, "s16"), (8192, 7, 4.0, 0.5, "f32")])
def test_batch_past_one_pass_bit_for_bit(lib, torch_cuda, n, kmax, nw, ovl, fmt, nb):
    """64 streams share the grid at 32 (N = 8192: 16) workgroups each, a multiple of 8, and make three (five) passes; 40 streams at
    52 (26), no multiple of 8, make two (three).  The streams are cut from one apart_by_pass buffer laid out for the BATCH's pass
    boundaries, one pass apart: neighbours begin with the levels the other way round.  Every stream's rows are the bits of the
    single-stream call (the two-pass launch test_rows_past_one_pass_bin_by_bin holds to float64), and for the first, the middle and
    the last stream the bits of range calls of at most 60 units of work, each a single pass."""
    torch = torch_cuda
    c = Case(n, kmax, nw, ovl, fmt, 0, G.TWO_PASS_FRAMES[n], "apart_by_pass")
    p = G.passes("spectro16cx", n, c.frames, nb)
    assert p.npasses >= (3 if nb == G.BATCH_MULTIPLE_OF_8 else 2) and (p.grid % 8 == 0) == (nb == G.BATCH_MULTIPLE_OF_8)
    hop = hop_len(n, ovl)
    total = (nb - 1) * p.stride + c.frames
    big = torch.from_numpy(E.quantise(E.make_pass_input(c.name, n, hop, total, 5, p.stride), fmt)).cuda()
    S = c.frames * hop
    v = big.as_strided((nb, S, 2), (p.stride * hop * 2, 2, 1))
    sp = _plan(lib, c)
    got = sp.cross_batch(v, want=ALL)
    assert got.coh.shape == (nb, c.frames, n // 2 + 1)
    for b in range(nb):
        assert _same_all([t[b] for t in got], sp.cross(v[b], want=ALL)), b
    for b in (0, nb // 2, nb - 1):
        for first, cnt in _chunks(c.frames, 60 * p.fpb):
            assert G.passes("spectro16cx", n, cnt).npasses == 1
            part = sp.cross(v[b], first_frame=first, nframes=cnt, want=ALL)
            assert _same_all(part, [t[b, first:first + cnt] for t in got]), (b, first, cnt)
    sp.close()


# ---- bit for bit ------------------------------------------------------------------------------------------------------
BIT_CASES = [Case(256, 4, 2.5, 0.5, "f32", 0, 21, "noise"), Case(1024, 7, 4.0, 0.3, "s16", 0, 7, "line"),
             Case(4096, 1, 2.0, 0.75, "u8", 1, 5, "noise"), Case(8192, 4, 2.5, 0.0, "f32", 0, 5, "delay3")]
bit_cases = pytest.mark.parametrize("c", BIT_CASES, ids=_id)


@bit_cases
@pytest.mark.parametrize("nb", [1, 2, 5])
def test_batch_equals_loop_of_single_calls(lib, torch_cuda, c, nb):
    """Streams a pitch larger than S apart: entry b of the batch is cross() of stream b."""
    torch = torch_cuda
    sp = _plan(lib, c)
    ns = c.frames * hop_len(c.n, c.ovl)
    raws = [_input(c, seed)[0] for seed in range(nb)]
    buf = torch.zeros((nb, ns + 37, 2), dtype=torch.from_numpy(raws[0]).dtype, device="cuda")
    for b in range(nb):
        buf[b, :ns] = torch.from_numpy(raws[b]).cuda()
    got = sp.cross_batch(buf[:, :ns], want=ALL)
    for b in range(nb):
        one = sp.cross(torch.from_numpy(raws[b]).cuda(), want=ALL)
        assert _same_all([t[b] for t in got], one), b
    sp.close()


@bit_cases
def test_frame_ranges_equal_the_whole_run(lib, torch_cuda, c):
    torch = torch_cuda
    sp = _plan(lib, c)
    d = torch.from_numpy(_input(c)[0]).cuda()
    whole = sp.cross(d, want=ALL)
    for first, cnt in ((0, 1), (1, 3), (c.frames - 2, 2), (2, c.frames - 2)):
        part = sp.cross(d, first_frame=first, nframes=cnt, want=ALL)
        assert _same_all(part, [t[first:first + cnt] for t in whole]), (first, cnt)
    sp.close()


@bit_cases
def test_pitched_outputs_between_sentinels(lib, torch_cuda, c):
    """Pitched outputs: the same bins, the padding and the guards before and after keep their bytes."""
    torch = torch_cuda
    sp = _plan(lib, c)
    d = torch.from_numpy(_input(c)[0]).cuda()
    dense = sp.cross(d, want=ALL)
    bins, guard = c.n // 2 + 1, 1024
    pitch, xpitch = bins + 11, bins + 5
    bufs, views = {}, {}
    for name in ALL:
        p, dt = (xpitch, torch.complex64) if name == "sxy" else (pitch, torch.float32)
        bufs[name] = torch.full((guard + c.frames * p + guard,), SENTINEL, dtype=dt, device="cuda")
        views[name] = bufs[name][guard:guard + c.frames * p].view(c.frames, p)
    got = sp.cross(d, want=ALL, out={k: v[:, :bins] for k, v in views.items()})
    torch.cuda.synchronize()
    for name in ALL:
        assert getattr(got, name).data_ptr() == views[name].data_ptr()
        assert _same(views[name][:, :bins], getattr(dense, name)), name
        assert bool((views[name][:, bins:] == SENTINEL).all()), name
        assert bool((bufs[name][:guard] == SENTINEL).all()) and bool((bufs[name][-guard:] == SENTINEL).all()), name
    sp.close()


@bit_cases
def test_every_subset_of_outputs_equals_the_all_four_call(lib, torch_cuda, c):
    torch = torch_cuda
    sp = _plan(lib, c)
    d = torch.from_numpy(_input(c)[0]).cuda()
    full = sp.cross(d, want=ALL)
    for r in range(1, 4):
        for want in itertools.combinations(ALL, r):
            part = sp.cross(d, want=want)
            for name in ALL:
                if name in want:
                    assert _same(getattr(part, name), getattr(full, name)), (want, name)
                else:
                    assert getattr(part, name) is None
    dflt = sp.cross(d)
    assert dflt.sxx is None and dflt.syy is None and _same(dflt.coh, full.coh) and _same(dflt.sxy, full.sxy)
    cplx = sp.cross(torch.view_as_complex(d), want=ALL) if c.fmt == "f32" else full     # complex64 [S]: x in the real part
    assert _same_all(cplx, full)
    sp.close()


# ---- refusals, graph capture ------------------------------------------------------------------------------------------
def test_device_entry_refusals_with_real_plans(lib, torch_cuda):
    assert device_entry_refusals(lib) == 10


def test_wrapper_refuses_wrong_plans_and_inputs(lib, torch_cuda):
    torch = torch_cuda
    sp = lib.Spectrogram(lib.MtmParams(n=1024, overlap=0.5, w=2.5, kmax=4, sample_format=lib.SAMPLES_S16))
    good = torch.zeros((4096, 2), dtype=torch.int16, device="cuda")
    assert sp.cross(good).coh.shape == (8, 513)
    for bad in (torch.zeros((4096, 2), dtype=torch.float32, device="cuda"), torch.zeros((4096, 3), dtype=torch.int16, device="cuda"),
                torch.zeros(8192, dtype=torch.int16, device="cuda")):
        with pytest.raises(AssertionError):
            sp.cross(bad)
    with pytest.raises(lib.GlferHipError):
        sp.cross(good, first_frame=6, nframes=3)                          # a frame past the stream
    sp.close()
    for params in (lib.FftParams(n=1024, window_type=0, overlap=0.5), lib.MtmParams(n=1024, w=2.0, kmax=0),
                   lib.MtmParams(n=16384, w=2.5, kmax=4)):
        other = lib.Spectrogram(params)
        with pytest.raises(lib.GlferHipError):
            other.cross(torch.zeros((4 * params.n, 2), dtype=torch.float32, device="cuda"))
        other.close()


def test_graph_capture_and_replay(lib, torch_cuda):
    """One capture of cross on a non-default stream, replayed: the eager rows."""
    torch = torch_cuda
    c = Case(4096, 4, 2.5, 0.5, "f32", 0, 7, "line")
    sp = _plan(lib, c)
    d = torch.from_numpy(_input(c)[0]).cuda()
    eager = sp.cross(d, want=ALL)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    bins = c.n // 2 + 1
    outs = {k: torch.full((c.frames, bins), SENTINEL, dtype=torch.complex64 if k == "sxy" else torch.float32, device="cuda") for k in ALL}
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        sp.cross(d, want=ALL, out=outs)
    torch.cuda.synchronize()
    for o in outs.values():
        o.fill_(SENTINEL)
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    assert _same_all([outs[k] for k in ALL], eager)
    sp.close()
