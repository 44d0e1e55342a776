"""The drift search on the device (drift_sums, drift_sums_batch, Spectrogram.run_drift): every output is bit for bit the float32
restatement of tests/_drift_exact.py, NaN results compared as NaN.  The cases are tests/_drift_cases.py's -- the smallest shapes
at which the kernel can go wrong (tile 256 bins, register groups of 8 / 32 / 64 drifts, halo max(-dmin, dmax)) --, and
tests/test_drift_criterion.py shows on the same inputs that this comparison rejects the wrong kernels one could write."""
import ctypes
import itertools
import os

import numpy as np
import pytest

import _drift_cases as K
import _drift_exact as X
from _signals import synth

pytestmark = pytest.mark.gpu

FIELDS = ("sums", "best", "drift")
SENTINEL = {"sums": 7777.0, "best": 7777.0, "drift": -999}
OK, E_ARG = 0, -1


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def device_rows(torch, case):
    """the case's rows on the device as the entries take them: [F][bins] with stride(0) = pitch (the padding holds 1e30)"""
    return torch.from_numpy(K.make_rows(case)).cuda()[:, :case.bins]


def guarded(torch, lead, nblocks, D, bins):
    """the three outputs between sentinel rows: (buffers by name, the views to write)"""
    bufs, outs = {}, {}
    for name in FIELDS:
        shape = tuple(lead) + ((nblocks + 2, D, bins) if name == "sums" else (nblocks + 2, bins))
        dtype = torch.int16 if name == "drift" else torch.float32
        bufs[name] = torch.full(shape, SENTINEL[name], dtype=dtype, device="cuda")
        outs[name] = bufs[name][1:-1] if not lead else None
    return bufs, outs


def check(got, want, what):
    for name, g, w in zip(FIELDS, got, want):
        assert g is not None, (what, name)
        g = g.cpu().numpy()
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name, g.shape, w.shape)
        assert X.same_bits(g, w), (what, name, int(np.sum(g != w)))


@pytest.mark.parametrize("case", K.CASES, ids=lambda c: c.name)
def test_case_is_the_restatement_bit_for_bit(lib, torch, case):
    rows = device_rows(torch, case)
    want = K.reference(case)
    nblocks, D = X.blocks(case.F, case.T, case.step), case.dmax - case.dmin + 1
    assert want[0].shape == (nblocks, D, case.bins)
    bufs, outs = guarded(torch, (), nblocks, D, case.bins)
    got = lib.drift_sums(rows, case.T, case.step, case.dmin, case.dmax, want=FIELDS, out=outs)
    torch.cuda.synchronize()
    check(got, want, case.name)
    for name in FIELDS:                                          # the rows before and behind the outputs survive
        assert bool((bufs[name][0] == SENTINEL[name]).all()) and bool((bufs[name][-1] == SENTINEL[name]).all()), name
    again = lib.drift_sums(rows, case.T, case.step, case.dmin, case.dmax, want=FIELDS)      # repeated: the same bits
    check(again, want, case.name + " again")


@pytest.mark.parametrize("name", ["b5_T16_full", "b257_T65_three_passes_pitched", "b300_T16_nine_drifts", "nan"])
def test_every_subset_of_the_outputs_gives_the_same_bits(lib, torch, name):
    case = K.BY_NAME[name]
    rows, want = device_rows(torch, case), dict(zip(FIELDS, K.reference(case)))
    for r in (1, 2):
        for subset in itertools.combinations(FIELDS, r):
            got = lib.drift_sums(rows, case.T, case.step, case.dmin, case.dmax, want=subset)
            for f in FIELDS:
                if f in subset:
                    assert X.same_bits(getattr(got, f).cpu().numpy(), want[f]), (subset, f)
                else:
                    assert getattr(got, f) is None, (subset, f)


def test_defaults_are_disjoint_blocks_and_the_full_range(lib, torch):
    case = K.BY_NAME["const"]                                    # step = T = 16, -15 .. 15
    got = lib.drift_sums(device_rows(torch, case), case.T)
    _, best, drift = K.reference(case)
    assert got.sums is None and X.same_bits(got.best.cpu().numpy(), best) and X.same_bits(got.drift.cpu().numpy(), drift)


def test_rows_one_short_of_a_block_leave_the_outputs_untouched(lib, torch):
    case = K.BY_NAME["b65_T16_down_pitched"]
    rows = device_rows(torch, case)[:case.T - 1]
    got = lib.drift_sums(rows, case.T, case.step, case.dmin, case.dmax, want=FIELDS)
    assert got.sums.shape == (0, 16, 65) and got.best.shape == (0, 65) and got.drift.shape == (0, 65)
    bufs, _ = guarded(torch, (), 1, 16, 65)
    one = lib.api.lib().glfer_hip_drift_device
    assert one(rows.data_ptr(), case.T - 1, 65, case.pitch, case.T, case.step, 0, case.dmin, case.dmax, bufs["sums"].data_ptr(),
               bufs["best"].data_ptr(), bufs["drift"].data_ptr(), None) == OK
    assert one(rows.data_ptr(), case.T - 1, 65, case.pitch, case.T, case.step, 1, case.dmin, case.dmax, bufs["sums"].data_ptr(),
               bufs["best"].data_ptr(), bufs["drift"].data_ptr(), None) == E_ARG
    torch.cuda.synchronize()
    for name in FIELDS:
        assert bool((bufs[name] == SENTINEL[name]).all()), name


def test_three_unlike_streams_a_stride_apart_equal_three_single_calls(lib, torch):
    """noise, the NaN case's rows and silence as one batch: F = 32 rows of 65 bins each, pitched and two rows further apart"""
    T, step, dmin, dmax, bins, F = 16, 5, -15, 15, 65, 32
    parts = [K.make_rows(K.BY_NAME[n])[:F, :bins] for n in ("inf", "nan", "silence")]
    buf = torch.full((3, F + 2, bins + 4), float(K.PAD), dtype=torch.float32, device="cuda")
    rows = buf[:, :F, :bins]
    for b, part in enumerate(parts):
        rows[b] = torch.from_numpy(np.ascontiguousarray(part)).cuda()
    got = lib.drift_sums_batch(rows, T, step, dmin, dmax, want=FIELDS)
    torch.cuda.synchronize()
    for b, part in enumerate(parts):
        want = X.drift_all(part, bins, T, step, dmin, dmax)
        check(tuple(g[b] for g in got), want, "stream %d" % b)
        check(lib.drift_sums(rows[b], T, step, dmin, dmax, want=FIELDS), want, "single %d" % b)
    only = lib.drift_sums_batch(rows, T, step, dmin, dmax)          # best and drift alone
    assert only.sums is None and torch.equal(only.best[~only.best.isnan()], got.best[~got.best.isnan()]) and torch.equal(only.drift, got.drift)
    with pytest.raises(ValueError, match="apart"):
        lib.drift_sums_batch(buf[:1, :F, :bins].expand(3, F, bins), T)


def test_a_captured_graph_replays_the_eager_bits(lib, torch):
    case = K.BY_NAME["b257_T65_three_passes_pitched"]
    rows, want = device_rows(torch, case), K.reference(case)
    nblocks, D = want[0].shape[0], want[0].shape[1]
    outs = {"sums": torch.zeros((nblocks, D, case.bins), dtype=torch.float32, device="cuda"),
            "best": torch.zeros((nblocks, case.bins), dtype=torch.float32, device="cuda"),
            "drift": torch.zeros((nblocks, case.bins), dtype=torch.int16, device="cuda")}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            lib.drift_sums(rows, case.T, case.step, case.dmin, case.dmax, want=FIELDS, out=outs)
    torch.cuda.current_stream().wait_stream(side)
    for _ in range(2):
        for o in outs.values():
            o.zero_()
        g.replay()
        torch.cuda.synchronize()
        check(tuple(outs[f] for f in FIELDS), want, "replay")


# ---- run_drift: the plan's rows through scratch, in pieces
def _plans(lib):
    return [("fft256", lambda: lib.Spectrogram(lib.FftParams(n=256, window_type=lib.WINDOWS["hanning"], overlap=0.0))),
            ("mtm1024", lambda: lib.Spectrogram(lib.MtmParams(n=1024, overlap=0.5, w=2.5, kmax=5))),
            ("lmp256", lambda: lib.Spectrogram(lib.LmpParams(n=256, overlap=0.0, avg=4)))]


@pytest.mark.parametrize("which", [0, 1, 2], ids=["fft256", "mtm1024", "lmp256"])
def test_run_drift_is_run_then_drift_sums_whatever_the_cut(lib, torch, which):
    sp = _plans(lib)[which][1]()
    L = lib.api.lib()
    T, step, first, nblocks = 16, 11, 5, 12                      # frames 5 .. 5 + 11 * 11 + 16 = 142 of 150: off the frame grid at both ends
    x = torch.from_numpy(synth(150 * sp.hop, seed=3 + which)).cuda()
    span = (nblocks - 1) * step + T
    rows = sp.run(x, first_frame=first, nframes=span)
    want = lib.drift_sums(rows[:, :sp.bins], T, step, want=FIELDS)
    got = sp.run_drift(x, T, step, first_frame=first, nblocks=nblocks, want=FIELDS)
    torch.cuda.synchronize()
    for f in FIELDS:
        assert torch.equal(getattr(got, f), getattr(want, f)), (f, "one piece")
    whole = sp.run_drift(x, T, step, first_frame=first)           # every block behind first_frame
    assert whole.best.shape[0] == lib.drift_blocks(150 - first, T, step) >= nblocks and whole.sums is None
    assert torch.equal(whole.best[:nblocks], want.best) and torch.equal(whole.drift[:nblocks], want.drift)
    row_bytes = sp.pitch * 4
    try:
        # half the cap holds the rows of three blocks (and the 62 that complete the end groups): four pieces; then one block a piece
        for cap in (2 * (2 * step + T + 62) * row_bytes + 8, 0):
            L.glfer_hip_scratch_limit(cap)
            cut = sp.run_drift(x, T, step, first_frame=first, nblocks=nblocks, want=FIELDS)
            torch.cuda.synchronize()
            for f in FIELDS:
                assert torch.equal(getattr(cut, f), getattr(want, f)), (f, cap)
    finally:
        L.glfer_hip_scratch_limit(int(os.environ.get("GLFER_SCRATCH_CAP_MB", 16 << 10)) << 20)   # what the library started with
    # blocks or a first frame past the stream
    with pytest.raises(ValueError, match="nblocks"):
        sp.run_drift(x, T, step, first_frame=first, nblocks=nblocks + 2)
    with pytest.raises(ValueError, match="first_frame"):
        sp.run_drift(x, T, step, first_frame=151)
    sp.close()


def test_spectrogram_drift_argument_rules(lib, torch):
    L = lib.api.lib()
    spec = L.glfer_hip_spectrogram_drift_device
    sp = lib.Spectrogram(lib.FftParams(n=256, window_type=0))
    h, p = sp._h, 4096                                           # p: any non-NULL value, nothing below reaches the device
    ns = 256 * 64
    assert spec(h, p, ns, 0, 1, 16, 1, 0, 0, p, p, p, None) == E_ARG                  # frames
    assert spec(h, p, ns, 0, 16, 0, 1, -15, 15, p, p, p, None) == E_ARG               # step
    assert spec(h, p, ns, 0, 16, 16, 0, -16, 15, None, None, None, None) == E_ARG     # dmin, before "nothing to do"
    assert spec(h, None, 0, 0, 16, 16, 0, -15, 15, None, None, None, None) == OK
    assert spec(h, None, ns, 0, 16, 16, 4, -15, 15, p, p, p, None) == E_ARG           # NULL stream
    assert spec(h, p, ns, 0, 16, 16, 4, -15, 15, None, None, None, None) == E_ARG     # no output
    assert spec(h, p, ns, 0, 16, 16, 5, -15, 15, p, p, p, None) == E_ARG              # frames past the stream
    assert spec(h, p, ns, 49, 16, 16, 1, -15, 15, p, p, p, None) == E_ARG
    assert spec(h, p, ns, 65, 16, 16, 1, -15, 15, p, p, p, None) == E_ARG
    assert spec(h, p, ns, 0, 16, 1 << 62, 3, -15, 15, p, p, p, None) == E_ARG         # a span that wraps
    # a stream that is being captured: refused before anything is taken (the rows entries are not: see the graph test)
    x = torch.from_numpy(synth(ns, seed=1)).cuda()
    best = torch.zeros((4, sp.bins), dtype=torch.float32, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            best.zero_()
            rc = spec(h, x.data_ptr(), ns, 0, 16, 16, 4, -15, 15, None, best.data_ptr(), None, ctypes.c_void_p(side.cuda_stream))
    torch.cuda.current_stream().wait_stream(side)
    assert rc == E_ARG
    sp.close()


@pytest.mark.parametrize("c", K.DETECT, ids=lambda c: "T%d_b%d_A%g_d%d" % (c.T, c.bins, c.A, c.d0))
def test_a_drifting_line_is_found_on_the_device(lib, torch, c):
    rows = K.detect_rows(c).astype(np.float32)
    got = lib.drift_sums(torch.from_numpy(rows).cuda(), c.T)      # disjoint blocks, the full range
    torch.cuda.synchronize()
    best, drift = got.best.cpu().numpy(), got.drift.cpu().numpy()
    K.detect_check(c, best, drift)
    want = X.drift_all(rows, c.bins, c.T, c.T, -(c.T - 1), c.T - 1)
    assert X.same_bits(best, want[1]) and X.same_bits(drift, want[2])
