"""Spectrogram.cross_welch on the GPU: segment-averaged auto-spectra, cross-spectrum and coherence of two interleaved channels, bin
by bin against float64 (tests/_cross_check.py's rule, tau from the float32 stand-in on the CPU: tests/_welch_exact.py), over every
size the kernel is built for, FFT plans of three windows and multitaper plans of one, two and five tapers, L in {2, 3, 8} with
step in {1, L, L + 2}, the four overlaps, the three sample formats, both history modes and nine inputs, and one long accumulation;
the exact zeros of silent channels; what the rows mean (a delay's phase, a weak common line's peak); then bit for bit: one segment
against Spectrogram.cross, row ranges, moving rows against block rows, batches against the loop, pitched outputs between
sentinels, every subset of outputs, the complex view, one capture and replay; and the refusals with real plans.

Past one pass of the persistent grid (tests/_grid_passes.py; rows are the work here): N = 256, 2048 and 8192 with 71 units of rows
on a grid of 64, Hanning plans with (L, step) = (3, 1) and (3, 5) and a two-taper plan with (2, 2), on noise and on the inputs keyed
to the pass boundaries -- x_late / x_early leave a row of pass 1 with x in one segment alone --; then 64 and 40 streams sharing the
grid, bit for bit against those calls and against row ranges of a single pass.

Lines starting with 'cross-rows' (run with -s) are the record kept in profiles/welch_cross_rows.txt; those that go on with
'past-one-pass', in profiles/rows_past_one_pass.txt."""
import itertools

import numpy as np
import pytest

import _cross_check as K
import _cross_exact as E
import _grid_passes as G
import _welch_exact as W
from _exact import hop_len
from test_welch_host import check_welch_rows, device_entry_refusals

pytestmark = pytest.mark.gpu
SENTINEL = -7.25
ALL = ("sxx", "syy", "sxy", "coh")
CASES = W.cases()


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _plan(lib, c):
    return lib.Spectrogram(W.params_of(lib, c.n, c.kind, c.ovl, c.fmt, c.hist))


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


def test_the_cases_cover_the_grid():
    """Every (L, step) of {2, 3, 8} x {1, L, L + 2}, the MTM (kmax, L) pairs, the windows, overlaps, formats and history modes;
    per size a row count above the block's frames, and none a multiple of them."""
    fft = [c for c in CASES if c.kind[0] == "fft" and c.segments <= 8]
    assert {(c.segments, (c.step == 1) + 2 * (c.step == c.segments) + 3 * (c.step == c.segments + 2)) for c in fft} == \
        {(s, k) for s in (2, 3, 8) for k in (1, 2, 3)}
    assert {(c.kind[1], c.segments) for c in CASES if c.kind[0] == "mtm"} == {(0, 3), (1, 2), (4, 3)}
    assert {c.kind[1] for c in CASES if c.kind[0] == "fft"} == {"rectangular", "hanning", "blackman"}
    assert {c.ovl for c in CASES} == set(W.OVERLAPS) and {c.fmt for c in CASES} == set(W.FMTS) and {c.hist for c in CASES} == {0, 1}
    for n in W.SIZES:
        mine = [c for c in CASES if c.n == n]
        fpb = W.frames_per_block(n)
        assert {c.name for c in mine} == set(E.INPUTS)
        assert {c.kind[0] for c in mine} == {"fft", "mtm"}
        assert any(c.rows > fpb for c in mine)
        assert fpb == 1 or all(c.rows % fpb for c in mine)
    assert any(c.segments == 64 and c.n == 256 and c.rows == 3 for c in CASES)


# ---- accuracy, bin by bin -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", CASES, ids=W.case_id)
def test_rows_bin_by_bin(lib, torch_cuda, c):
    torch = torch_cuda
    raw, _ = W.case_input(c)
    p64, p32 = W.case_per_frame(lib, c)
    ref = W.welch64(p64, c.segments, c.step)
    tau = K.tau_of(W.welch32(p32, c.segments, c.step), ref)                       # from the CPU alone
    sp = _plan(lib, c)
    assert sp.welch_rows(len(raw), c.segments, c.step) == c.rows
    got = _host(sp.cross_welch(torch.from_numpy(raw).cuda(), c.segments, c.step, want=ALL))
    torch.cuda.synchronize()
    sp.close()
    assert got.sxx.shape == (c.rows, c.n // 2 + 1) and got.sxy.dtype == np.complex64
    assert (got.sxy.imag[:, 0] == 0).all() and (got.sxy.imag[:, -1] == 0).all()    # exact zeros at DC and Nyquist
    K.check(got, ref, tau, W.case_id(c))
    if c.name == "silence":
        for a in (got.sxx, got.syy, got.coh, got.sxy.real, got.sxy.imag):
            assert (a == 0).all()
    if c.name == "x_only":
        assert (got.coh == 0).all() and (got.syy == 0).all() and (got.sxy == 0).all() and (got.sxx > 0).any()
    if c.name == "delay3" and c.hist == 0:
        k = c.n // 16                                    # mid-band: 2 pi k 3 / N = 3 pi / 8
        for r in range(c.rows):
            if r * c.step >= 2:                          # settled rows: every frame of theirs has its history
                assert np.angle(ref.sxy[r, k]) > 0 and np.angle(got.sxy[r, k]) > 0, (r, np.angle(ref.sxy[r, k]), np.angle(got.sxy[r, k]))


@pytest.mark.parametrize("n", [256, 4096])
def test_a_channel_silent_in_one_segment_only_is_not_zeroed(lib, torch_cuda, n):
    """x holds no sample in segment 0 of each row and noise in the others: the row's bits are the OR over its segments, so its
    spectra are those of the other segments -- held to the rule, and not the zeros of a silent channel."""
    torch = torch_cuda
    c = W.Case(n, W.KINDS[2], 0.0, "f32", 0, 3, 3, 5 if n == 256 else 2, "noise")
    xy = W.case_input(c)[1].copy()
    for r in range(c.rows):
        xy[r * 3 * n:(r * 3 + 1) * n, 0] = 0.0
    tapers, sig = W.tables_of(lib, n, c.kind)
    ref = W.welch64(E.cross64(xy, n, 0.0, tapers, sig), 3, 3)
    tau = K.tau_of(W.welch32(E.cross32(xy, n, 0.0, tapers, sig), 3, 3), ref)
    sp = _plan(lib, c)
    got = _host(sp.cross_welch(torch.from_numpy(xy).cuda(), 3, want=ALL))
    sp.close()
    K.check(got, ref, tau, "x silent in segment 0 n=%d" % n)
    assert (got.sxx > 0).all() and (got.coh > 0).any() and (np.abs(got.sxy) > 0).any()


# ---- past one pass of the grid ------------------------------------------------------------------------------------------
PASS_CASES = W.pass_cases()


@pytest.mark.parametrize("c", PASS_CASES, ids=W.case_id)
def test_rows_past_one_pass_bin_by_bin(lib, torch_cuda, c):
    """71 units of ROWS on a grid of 64: seven blocks run a second row group.  x_late / x_early put a row into pass 1 that holds
    x in one of its segments alone (tests/test_welch_criterion.py), so the OR over a row's segments is taken in a later pass."""
    from test_welch_criterion import pass_case_bits
    torch = torch_cuda
    assert G.passes("spectro16cx", c.n, c.rows).npasses == 2
    raw, xy32 = W.case_input(c)
    p64, p32 = W.case_per_frame(lib, c)
    ref = W.welch64(p64, c.segments, c.step)
    tau = K.tau_of(W.welch32(p32, c.segments, c.step), ref)                       # from the CPU alone
    sp = _plan(lib, c)
    d = torch.from_numpy(raw).cuda()
    got = _host(sp.cross_welch(d, c.segments, c.step, want=ALL))
    assert got.sxx.shape == (c.rows, c.n // 2 + 1)
    bits, quiet = pass_case_bits(c, xy32)

    def held(got, ref, bits, quiet, what):
        assert (got.sxy.imag[:, 0] == 0).all() and (got.sxy.imag[:, -1] == 0).all()
        K.check(got, ref, tau, what)
        for a in (got.sxx, got.coh, got.sxy.real, got.sxy.imag):                   # exact zeros where x has no sample in any segment
            assert (a[quiet] == 0).all(), what
        assert (got.sxx[(bits & 1) != 0] > 0).any(axis=1).all(), what
    held(got, ref, bits, quiet, "past-one-pass " + W.case_id(c))
    if c.name == "x_early":
        # once more from row 2 (first_frame = 2 step): frame0 + fblk * step + seg with frame0 != 0 in the second pass, two passes
        # still, against the same float64 rows
        assert G.passes("spectro16cx", c.n, c.rows - 2).npasses == 2
        part = _host(sp.cross_welch(d, c.segments, c.step, first_frame=2 * c.step, want=ALL))
        assert part.sxx.shape == (c.rows - 2, c.n // 2 + 1)
        held(part, E.Cross(*(a[2:] for a in ref)), bits[2:], quiet[quiet >= 2] - 2, "past-one-pass first_frame=%d %s" % (2 * c.step, W.case_id(c)))
    sp.close()


@pytest.mark.parametrize("nb", [G.BATCH_MULTIPLE_OF_8, G.BATCH_OTHER])
@pytest.mark.parametrize("n,kind,ovl,fmt,segments,step", [(256, W.KINDS[2], 0.5, "f32", 3, 1), (2048, W.KINDS[3], 0.75, "s16", 2, 2),
                                                           (8192, W.KINDS[2], 0.5, "f32", 3, 1)])
def test_batch_past_one_pass_bit_for_bit(lib, torch_cuda, n, kind, ovl, fmt, segments, step, nb):
    """tests/test_gpu_cross.py::test_batch_past_one_pass_bit_for_bit for rows: the streams lie one pass of ROWS (stride * step
    frames) apart in one apart_by_pass buffer; every stream against the single-stream two-pass call, three streams against row
    ranges of at most 60 units of work."""
    torch = torch_cuda
    c = W.Case(n, kind, ovl, fmt, 0, segments, step, G.TWO_PASS_FRAMES[n], "apart_by_pass")
    p = G.passes("spectro16cx", n, c.rows, nb)
    assert p.npasses >= (3 if nb == G.BATCH_MULTIPLE_OF_8 else 2) and (p.grid % 8 == 0) == (nb == G.BATCH_MULTIPLE_OF_8)
    hop = hop_len(n, ovl)
    total = (nb - 1) * p.stride * step + W.frames_of(c)
    big = torch.from_numpy(E.quantise(E.make_pass_input(c.name, n, hop, total, 5, p.stride, segments, step), fmt)).cuda()
    S = W.frames_of(c) * hop
    v = big.as_strided((nb, S, 2), (p.stride * step * hop * 2, 2, 1))
    sp = _plan(lib, c)
    got = sp.cross_welch_batch(v, segments, step, want=ALL)
    assert got.coh.shape == (nb, c.rows, n // 2 + 1)
    for b in range(nb):
        assert _same_all([t[b] for t in got], sp.cross_welch(v[b], segments, step, want=ALL)), b
    for b in (0, nb // 2, nb - 1):
        for r0 in range(0, c.rows, 60 * p.fpb):
            cnt = min(60 * p.fpb, c.rows - r0)
            part = sp.cross_welch(v[b], segments, step, first_frame=r0 * step, nrows=cnt, want=ALL)
            assert _same_all(part, [t[b, r0:r0 + cnt] for t in got]), (b, r0, cnt)
    sp.close()


# ---- what the rows mean -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1024, 8192])
def test_line10_peaks_at_the_line(lib, torch_cuda, n):
    """A common line 10 dB under each channel's noise, sixteen averaged segments: the device's largest coherence of every row is at
    the line's bin (float64's premise: tests/test_welch_criterion.py::test_line_premise_in_float64), and the rows pass the rule."""
    torch = torch_cuda
    c = W.line10_case(n)
    raw, _ = W.case_input(c)
    p64, p32 = W.case_per_frame(lib, c)
    ref = W.welch64(p64, c.segments, c.step)
    tau = K.tau_of(W.welch32(p32, c.segments, c.step), ref)
    sp = _plan(lib, c)
    got = _host(sp.cross_welch(torch.from_numpy(raw).cuda(), c.segments, want=ALL))      # step=None: the block average
    sp.close()
    assert got.coh.shape == (3, n // 2 + 1)
    K.check(got, ref, tau, W.case_id(c))
    assert (got.coh.argmax(axis=1) == E.line_bin(n)).all(), (got.coh.argmax(axis=1), E.line_bin(n))


# ---- bit for bit ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,kmax,nw,ovl,fmt,hist,frames", [(256, 4, 2.5, 0.5, "f32", 0, 21), (1024, 7, 4.0, 0.3, "s16", 0, 7),
                                                            (4096, 1, 2.0, 0.75, "u8", 1, 5), (8192, 4, 2.5, 0.0, "f32", 0, 5)])
def test_one_segment_equals_cross(lib, torch_cuda, n, kmax, nw, ovl, fmt, hist, frames):
    """A multitaper plan with segments = 1, step = 1: the bits of Spectrogram.cross, all four outputs, ranges included."""
    torch = torch_cuda
    c = W.Case(n, ("mtm", kmax, nw), ovl, fmt, hist, 1, 1, frames, "noise")
    sp = _plan(lib, c)
    d = torch.from_numpy(W.case_input(c)[0]).cuda()
    want = sp.cross(d, want=ALL)
    got = sp.cross_welch(d, 1, 1, want=ALL)
    assert got.sxx.shape == (frames, n // 2 + 1) and _same_all(got, want)
    part = sp.cross_welch(d, 1, 1, first_frame=1, nrows=frames - 2, want=ALL)
    assert _same_all(part, [t[1:frames - 1] for t in want])
    sp.close()


BIT_CASES = [W.Case(256, W.KINDS[2], 0.5, "f32", 0, 3, 2, 21, "noise"), W.Case(1024, W.KINDS[5], 0.3, "s16", 0, 3, 3, 5, "line"),
             W.Case(2048, W.KINDS[4], 0.75, "u8", 1, 2, 4, 3, "noise"), W.Case(4096, W.KINDS[0], 0.75, "u8", 1, 8, 1, 3, "noise"),
             W.Case(8192, W.KINDS[3], 0.0, "f32", 0, 2, 1, 3, "delay3")]
bit_cases = pytest.mark.parametrize("c", BIT_CASES, ids=W.case_id)


@bit_cases
@pytest.mark.parametrize("nb", [1, 2, 5])
def test_batch_equals_loop_of_single_calls(lib, torch_cuda, c, nb):
    """Streams a pitch larger than S apart: entry b of the batch is cross_welch() of stream b."""
    torch = torch_cuda
    sp = _plan(lib, c)
    ns = W.frames_of(c) * hop_len(c.n, c.ovl)
    raws = [W.case_input(c, seed)[0] for seed in range(nb)]
    buf = torch.zeros((nb, ns + 37, 2), dtype=torch.from_numpy(raws[0]).dtype, device="cuda")
    for b in range(nb):
        buf[b, :ns] = torch.from_numpy(raws[b]).cuda()
    got = sp.cross_welch_batch(buf[:, :ns], c.segments, c.step, want=ALL)
    assert got.coh.shape == (nb, c.rows, c.n // 2 + 1)
    for b in range(nb):
        one = sp.cross_welch(torch.from_numpy(raws[b]).cuda(), c.segments, c.step, want=ALL)
        assert _same_all([t[b] for t in got], one), b
    sp.close()


@bit_cases
def test_row_ranges_equal_the_whole_run(lib, torch_cuda, c):
    """first_frame / nrows: row i of a run from frame a = r step is row r + i of the whole run."""
    torch = torch_cuda
    sp = _plan(lib, c)
    d = torch.from_numpy(W.case_input(c)[0]).cuda()
    whole = sp.cross_welch(d, c.segments, c.step, want=ALL)
    assert whole.coh.shape[0] == c.rows
    for r0, cnt in ((0, 1), (1, c.rows - 1), (c.rows - 1, 1), (1, None)):
        part = sp.cross_welch(d, c.segments, c.step, first_frame=r0 * c.step, nrows=cnt, want=ALL)
        cnt = c.rows - r0 if cnt is None else cnt
        assert _same_all(part, [t[r0:r0 + cnt] for t in whole]), (r0, cnt)
    sp.close()


@bit_cases
def test_moving_rows_equal_block_rows(lib, torch_cuda, c):
    """Row r of (L, step = 1, first = a) is row 0 of (L, step = L, first = a + r): a row is a function of its own frames alone."""
    torch = torch_cuda
    sp = _plan(lib, c)
    d = torch.from_numpy(W.case_input(c)[0]).cuda()
    L, a = c.segments, 1
    moving = sp.cross_welch(d, L, 1, first_frame=a, want=ALL)
    assert moving.coh.shape[0] == W.frames_of(c) - a - L + 1 >= 2
    for r in range(moving.coh.shape[0]):
        block = sp.cross_welch(d, L, L, first_frame=a + r, nrows=1, want=ALL)
        assert _same_all(block, [t[r:r + 1] for t in moving]), r
    sp.close()


@bit_cases
def test_pitched_outputs_between_sentinels(lib, torch_cuda, c):
    """Pitched outputs: the same bins, the padding and the guards before and after keep their bytes."""
    torch = torch_cuda
    sp = _plan(lib, c)
    d = torch.from_numpy(W.case_input(c)[0]).cuda()
    dense = sp.cross_welch(d, c.segments, c.step, want=ALL)
    bins, guard = c.n // 2 + 1, 1024
    pitch, xpitch = bins + 11, bins + 5
    bufs, views = {}, {}
    for name in ALL:
        p, dt = (xpitch, torch.complex64) if name == "sxy" else (pitch, torch.float32)
        bufs[name] = torch.full((guard + c.rows * p + guard,), SENTINEL, dtype=dt, device="cuda")
        views[name] = bufs[name][guard:guard + c.rows * p].view(c.rows, p)
    got = sp.cross_welch(d, c.segments, c.step, want=ALL, out={k: v[:, :bins] for k, v in views.items()})
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
    d = torch.from_numpy(W.case_input(c)[0]).cuda()
    full = sp.cross_welch(d, c.segments, c.step, want=ALL)
    for r in range(1, 4):
        for want in itertools.combinations(ALL, r):
            part = sp.cross_welch(d, c.segments, c.step, want=want)
            for name in ALL:
                if name in want:
                    assert _same(getattr(part, name), getattr(full, name)), (want, name)
                else:
                    assert getattr(part, name) is None
    dflt = sp.cross_welch(d, c.segments, c.step)
    assert dflt.sxx is None and dflt.syy is None and _same(dflt.coh, full.coh) and _same(dflt.sxy, full.sxy)
    if c.fmt == "f32":                                   # complex64 [S]: x in the real part
        assert _same_all(sp.cross_welch(torch.view_as_complex(d), c.segments, c.step, want=ALL), full)
    sp.close()


# ---- refusals, graph capture ------------------------------------------------------------------------------------------
def test_device_entry_refusals_with_real_plans(lib, torch_cuda):
    assert device_entry_refusals(lib) == 9
    assert check_welch_rows(lib) == 2


def test_wrapper_refuses_wrong_plans_and_inputs(lib, torch_cuda):
    torch = torch_cuda
    sp = lib.Spectrogram(lib.FftParams(n=1024, window_type=0, overlap=0.5, sample_format=lib.SAMPLES_S16))
    good = torch.zeros((8192, 2), dtype=torch.int16, device="cuda")                 # sixteen frames
    assert sp.cross_welch(good, 4).coh.shape == (4, 513) and sp.welch_rows(8192, 4) == 4 and sp.welch_rows(8192, 4, 1, 2) == 11
    assert sp.cross_welch(good, 17).coh.shape == (0, 513)                           # fewer frames than segments: no rows
    with pytest.raises(lib.GlferHipError):
        sp.cross(good)                                                              # the per-frame entry still refuses an FFT plan
    with pytest.raises(lib.GlferHipError):
        sp.cross_welch(good, 1)                                                     # one window, one segment
    with pytest.raises(lib.GlferHipError):
        sp.cross_welch(good, 4, nrows=5)                                            # a row past the stream
    with pytest.raises(lib.GlferHipError):
        sp.cross_welch(good, 4, 0)
    with pytest.raises(AssertionError):
        sp.cross_welch(torch.zeros((8192, 2), dtype=torch.float32, device="cuda"), 4)
    sp.close()
    other = lib.Spectrogram(lib.FftParams(n=16384, window_type=0))
    with pytest.raises(lib.GlferHipError):
        other.cross_welch(torch.zeros((4 * 16384, 2), dtype=torch.float32, device="cuda"), 2)
    other.close()


def test_graph_capture_and_replay(lib, torch_cuda):
    """One capture of cross_welch on a non-default stream, replayed: the eager rows."""
    torch = torch_cuda
    c = W.Case(4096, W.KINDS[2], 0.5, "f32", 0, 3, 2, 3, "line")
    sp = _plan(lib, c)
    d = torch.from_numpy(W.case_input(c)[0]).cuda()
    eager = sp.cross_welch(d, c.segments, c.step, want=ALL)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    bins = c.n // 2 + 1
    outs = {k: torch.full((c.rows, bins), SENTINEL, dtype=torch.complex64 if k == "sxy" else torch.float32, device="cuda") for k in ALL}
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        sp.cross_welch(d, c.segments, c.step, want=ALL, out=outs)
    torch.cuda.synchronize()
    for o in outs.values():
        o.fill_(SENTINEL)
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    assert _same_all([outs[k] for k in ALL], eager)
    sp.close()
