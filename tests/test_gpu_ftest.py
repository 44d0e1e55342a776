"""GPU parity tests (-m gpu) for the harmonic F-test entry (glfer_hip_mtm_ftest_device, Spectrogram.ftest) on each of
its three routes -- spectrum by spectrum with ftest_kernel (N < 256), one taper per round (FT = 1) and two sequences per
transform separated through the mirror bins (FT = 2) -- at every block size, in the three sample formats, with mean
removal, both history modes, frame ranges, streams longer than one pass of the grid, the entry's refusals and what the
call leaves of the plan.

Every comparison with the oracle goes through tests/_ftest_check.py::check_ftest (the rule of test_ftest_vs_oracle, TOL
1e-5, no bin left out but Nyquist, which is asserted non-finite), the bound weighed by float64 num / den
(tests/_exact.py::ftest64).  The cases are tests/_ftest_cases.py's; tests/test_ftest_criterion.py runs the oracle against
float64 arithmetic on every one of them without a GPU.  GLFER_FTEST_PAIRED is read on every call, so the in-launch form
is chosen per test: 'single' = 0 (FT = 1), 'paired' = 1 (FT = 2), 'default' = unset (paired from N = 2048).

Lines starting with 'ftest-parity' (run with -s) are the record kept in profiles/ftest_parity.txt.
"""
import ctypes as C

import numpy as np
import pytest

import _ftest_cases as K
from _ftest_check import check_ftest
from _signals import rel_err

pytestmark = pytest.mark.gpu
TOL = 1e-5
SENTINEL = 0x5A5A5A5A                     # (3.76e16 as a float: no F row holds it)
PAD = 96                                  # guard floats either side of an output placed inside a larger buffer


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _select(monkeypatch, form):
    if form == "default":
        monkeypatch.delenv("GLFER_FTEST_PAIRED", raising=False)
    else:
        monkeypatch.setenv("GLFER_FTEST_PAIRED", {"single": "0", "paired": "1"}[form])


def _with_forms(cases, forms=("default", "single", "paired")):
    """Below N = 256 there is one route; from there on the in-launch forms asked for."""
    out = []
    for c in cases:
        for form in (forms if c.n >= 256 else ("default",)):
            out.append(pytest.param(c, form, id="%s-%s" % (K.case_id(c), form)))
    return out


def _plan(lib, c, **kw):
    fmt = {"f32": lib.SAMPLES_F32, "s16": lib.SAMPLES_S16, "u8": lib.SAMPLES_U8}[c.fmt]
    return lib.Spectrogram(lib.MtmParams(n=c.n, overlap=c.ovl, w=c.nw, kmax=c.kmax, sub_mean=c.sub_mean,
                                         history_mode=c.history_mode, sample_format=fmt, **kw))


def _upload(torch, raw, offset=0):
    """The stream on the device; offset > 0: that many samples into its allocation."""
    if not offset:
        return torch.from_numpy(raw).cuda()
    host = np.concatenate([np.full(offset, 77, raw.dtype), raw])
    return torch.from_numpy(host).cuda()[offset:]


def _float64_rows(num, den):
    rows = num / den
    rows[:, -1] = np.inf
    return rows


def _judge(group, c, form, got, oracle, rows=slice(None)):
    """got against the oracle's rows `rows` of the case through check_ftest; prints the record line."""
    _, _, want, num, den = K.reference(oracle, c)
    want, num, den = want[rows], num[rows], den[rows]
    assert got.shape == want.shape
    frac = check_ftest(got, want, num, den, c.kmax, tol=TOL)
    own = check_ftest(_float64_rows(num, den), want, num, den, c.kmax, tol=TOL)
    print("ftest-parity %s %-50s %-8s device/oracle %.4f  oracle/float64 %.4f" % (group, K.case_id(c), form, frac, own))
    return frac


def _ftest_into(lib, torch, sp, dx, first, nframes, mu_live=1):
    """The C entry itself, its output placed PAD floats into a buffer pre-filled with a sentinel: (rc, rows, guards intact)."""
    count = nframes * sp.bins
    buf = torch.full((PAD + count + PAD,), SENTINEL, dtype=torch.int32, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = lib.api.lib().glfer_hip_mtm_ftest_device(sp._h, C.c_void_p(dx.data_ptr()), dx.numel(), first, nframes,
                                                  C.c_void_p(buf.data_ptr() + 4 * PAD), mu_live, st)
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    intact = bool(np.all(host[:PAD] == SENTINEL) and np.all(host[PAD + count:] == SENTINEL))
    return rc, host[PAD:PAD + count].view(np.float32).reshape(nframes, sp.bins), intact


# ---- (a) every size, every form ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,form", _with_forms(K.SIZE_CASES))
def test_every_size_and_form(lib, oracle, torch_cuda, monkeypatch, c, form):
    _select(monkeypatch, form)
    raw = K.reference(oracle, c)[0]
    got = _plan(lib, c).ftest(_upload(torch_cuda, raw)).cpu().numpy()
    _judge("a", c, form, got, oracle)


# ---- (b) mu never written: the oracle's rows exactly -------------------------------------------------------------------
@pytest.mark.parametrize("c,form", _with_forms(K.SIZE_CASES))
def test_dead_mu_rows_are_the_oracles(lib, oracle, torch_cuda, monkeypatch, c, form):
    """The reference build without FFTW (mtm.c:173): numerator 0, so F = +0.0 wherever the denominator is not 0 and 0/0 at
    Nyquist.  One sequence fewer than the live call: the other parity of the paired form's sequence count."""
    _select(monkeypatch, form)
    raw, xf = K.reference(oracle, c)[:2]
    _, want = oracle.spectrogram_mtm_ftest(xf, c.n, c.ovl, c.nw, c.kmax, mu_live=0)
    half = c.n // 2
    assert np.all(want[:, :half].view(np.uint32) == 0) and np.isnan(want[:, half]).all()
    got = _plan(lib, c).ftest(_upload(torch_cuda, raw), mu_live=False).cpu().numpy()
    assert got.shape == want.shape
    assert np.array_equal(got[:, :half].view(np.uint32), want[:, :half].view(np.uint32))
    assert np.isnan(got[:, half]).all()
    print("dead mu, Nyquist bit patterns: device %s oracle %s" % (sorted({hex(v) for v in got[:, half].view(np.uint32)}),
                                                                   sorted({hex(v) for v in want[:, half].view(np.uint32)})))
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


# ---- (c) the two in-launch forms against each other --------------------------------------------------------------------
@pytest.mark.parametrize("c", K.MUTUAL_CASES, ids=K.case_id)
def test_forms_against_each_other(lib, oracle, torch_cuda, monkeypatch, c):
    """Each passes against the oracle by itself; their mutual distance by the same rule (not bit-identical: the paired form
    adds Z[k] and conj Z[N-k]).  The N = 16384 case is the one that found hn sharing its transform UNSCALED with taper 0:
    mu then carried the rounding of a spectrum ~ sqrt(sum U0^2) times its size, the paired rows were 1.09 of the bound from
    the oracle at frame 0, bin 2073 (one-taper form: 0.54, the oracle's own distance from float64) and 10 - 30 times the
    one-taper form's fraction everywhere else; with hn brought to a taper's size by a power of two (glfer_hip.cpp, the paired
    tables) the two forms are 0.02 of the bound apart."""
    _, _, _, num, den = K.reference(oracle, c)
    dx = _upload(torch_cuda, K.reference(oracle, c)[0])
    sp = _plan(lib, c)
    rows = {}
    for form in ("single", "paired"):
        _select(monkeypatch, form)
        rows[form] = sp.ftest(dx).cpu().numpy()
        _judge("c", c, form, rows[form], oracle)
    frac = check_ftest(rows["paired"], rows["single"], num, den, c.kmax, tol=TOL)
    print("ftest-parity c %-50s paired/single %.4f of the bound, %d of %d values differ" % (
        K.case_id(c), frac, int((rows["paired"][:, :-1] != rows["single"][:, :-1]).sum()), rows["single"][:, :-1].size))


# ---- (d) 16-bit and 8-bit samples --------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,form", _with_forms(K.FORMAT_CASES, ("single", "paired")))
def test_integer_sample_formats(lib, oracle, torch_cuda, monkeypatch, c, form):
    """The oracle on pcm_s16_to_float / pcm_u8_to_float of the same integers; some streams start an odd number of samples
    into their allocation (16-bit pairs off a 4-byte boundary)."""
    _select(monkeypatch, form)
    raw = K.reference(oracle, c)[0]
    assert raw.dtype == (np.int16 if c.fmt == "s16" else np.uint8)
    dx = _upload(torch_cuda, raw, K.FORMAT_OFFSETS.get(K.case_id(c), 0))
    _judge("d", c, form, _plan(lib, c).ftest(dx).cpu().numpy(), oracle)


# ---- (e) mean removal --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,form", _with_forms(K.MEAN_CASES, ("single", "paired")))
def test_mean_removal(lib, oracle, torch_cuda, monkeypatch, c, form):
    _select(monkeypatch, form)
    raw = K.reference(oracle, c)[0]
    _judge("e", c, form, _plan(lib, c).ftest(_upload(torch_cuda, raw)).cpu().numpy(), oracle)


# ---- (f) history and ranges --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,form", _with_forms(K.HISTORY_CASES, ("single", "paired")))
def test_history_zeroed_in_every_frame(lib, oracle, torch_cuda, monkeypatch, c, form):
    _select(monkeypatch, form)
    assert c.history_mode == lib.HISTORY_ZERO_ALWAYS
    raw = K.reference(oracle, c)[0]
    _judge("f", c, form, _plan(lib, c).ftest(_upload(torch_cuda, raw)).cpu().numpy(), oracle)


@pytest.mark.parametrize("cf,form", [pytest.param(cf, form, id="%s-first%d-%s" % (K.case_id(cf[0]), cf[1], form))
                                     for cf in K.RANGE_CASES for form in (("single", "paired") if cf[0].n >= 256 else ("default",))])
def test_frame_range_inside_the_stream(lib, oracle, torch_cuda, monkeypatch, cf, form):
    """first_frame > 0 and the launch ending before the stream does, through the C entry, the output inside a larger
    buffer: the oracle's rows of those frames, and not a float written before row 0 or after the last row."""
    c, first = cf
    _select(monkeypatch, form)
    raw = K.reference(oracle, c)[0]
    nframes = c.frames - first - 3
    assert nframes > 0
    sp = _plan(lib, c)
    dx = _upload(torch_cuda, raw)
    rc, got, intact = _ftest_into(lib, torch_cuda, sp, dx, first, nframes)
    assert rc == 0
    assert not np.any(got.view(np.uint32) == SENTINEL), "a value of the range was not written"
    assert intact, "the entry wrote outside [row 0, last row]"
    _judge("f", c, form, got, oracle, rows=slice(first, first + nframes))
    # the Python mirror: the same rows
    assert np.array_equal(sp.ftest(dx, first_frame=first, nframes=nframes).cpu().numpy().view(np.uint32), got.view(np.uint32))


# ---- (g) streams longer than one pass of the grid ----------------------------------------------------------------------
@pytest.mark.parametrize("c", K.LONG_CASES, ids=K.case_id)
def test_long_streams_every_frame(lib, oracle, torch_cuda, monkeypatch, c):
    """N = 16: two frame groups of the epilogue route.  N = 256 (FT = 1) and N = 2048 (FT = 2): work > grid in launch16_fmt,
    so the persistent blocks take a second block of frames, and the last block is partly filled.  All frames checked."""
    _select(monkeypatch, "default")
    raw = K.reference(oracle, c)[0]
    _judge("g", c, "default", _plan(lib, c).ftest(_upload(torch_cuda, raw)).cpu().numpy(), oracle)


# ---- (h) refusals ------------------------------------------------------------------------------------------------------
def test_refusals(lib, oracle, torch_cuda):
    E_ARG = -1                                                      # GLFER_E_ARG (include/glfer_hip.h)
    torch = torch_cuda
    # an MTM plan above the entry's range
    big = lib.Spectrogram(lib.MtmParams(n=32768, overlap=0.0, w=2.0, kmax=2))
    dx = torch.zeros(2 * 32768, device="cuda")
    rc, rows, intact = _ftest_into(lib, torch, big, dx, 0, 2)
    assert rc == E_ARG and intact and np.all(rows.view(np.uint32) == SENTINEL)
    with pytest.raises(lib.GlferHipError, match="bad argument"):
        big.ftest(dx)
    # a plan that is not MTM
    per = lib.Spectrogram(lib.FftParams(n=1024, window_type=0, overlap=0.0))
    dx = torch.zeros(4 * 1024, device="cuda")
    rc, rows, intact = _ftest_into(lib, torch, per, dx, 0, 4)
    assert rc == E_ARG and intact and np.all(rows.view(np.uint32) == SENTINEL)
    # a frame range one past the stream's whole hops; the whole range itself is taken
    c = K.case(1024, 0.5, 2.5, 4, 12)
    raw = K.reference(oracle, c)[0]
    sp = _plan(lib, c)
    dx = _upload(torch, raw)
    assert dx.numel() // sp.hop == c.frames and dx.numel() % sp.hop != 0
    for first, nframes in ((0, c.frames + 1), (1, c.frames), (c.frames, 1), (c.frames + 1, 1)):
        rc, rows, intact = _ftest_into(lib, torch, sp, dx, first, nframes)
        assert rc == E_ARG and intact and np.all(rows.view(np.uint32) == SENTINEL), (first, nframes)
    with pytest.raises(lib.GlferHipError, match="bad argument"):
        sp.ftest(dx, first_frame=1, nframes=c.frames)
    rc, rows, intact = _ftest_into(lib, torch, sp, dx, 0, c.frames)
    assert rc == 0 and intact
    _judge("h", c, "default", rows, oracle)
    # no frames: GLFER_OK, nothing written
    count = 3 * sp.bins
    buf = torch.full((count,), SENTINEL, dtype=torch.int32, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for first in (0, 5, c.frames):
        rc = lib.api.lib().glfer_hip_mtm_ftest_device(sp._h, C.c_void_p(dx.data_ptr()), dx.numel(), first, 0, C.c_void_p(buf.data_ptr()), 1, st)
        torch.cuda.synchronize()
        assert rc == 0 and bool((buf == SENTINEL).all())


# ---- (i) what the call leaves of the plan ------------------------------------------------------------------------------
@pytest.mark.parametrize("c,form", _with_forms(K.PLAN_CASES, ("single", "paired")))
def test_plan_after_the_call(lib, oracle, torch_cuda, monkeypatch, c, form):
    """run after ftest still gives the oracle's PSD rows; ftest after run gives the bits of ftest on a fresh plan."""
    _select(monkeypatch, form)
    raw, xf = K.reference(oracle, c)[:2]
    psd_w, _ = oracle.spectrogram_mtm_ftest(xf, c.n, c.ovl, c.nw, c.kmax, sub_mean=1 if c.sub_mean else 0, mu_live=1)
    dx = _upload(torch_cuda, raw)
    sp = _plan(lib, c)
    fresh = sp.ftest(dx).cpu().numpy()
    _judge("i", c, form, fresh, oracle)
    psd = sp.run(dx).cpu().numpy()
    assert max(max(rel_err(a, b)) for a, b in zip(psd, psd_w)) < TOL
    assert np.array_equal(sp.ftest(dx).cpu().numpy().view(np.uint32), fresh.view(np.uint32))
    other = _plan(lib, c)
    psd2 = other.run(dx).cpu().numpy()
    assert np.array_equal(psd2.view(np.uint32), psd.view(np.uint32))
    assert np.array_equal(other.ftest(dx).cpu().numpy().view(np.uint32), fresh.view(np.uint32))
    assert np.array_equal(other.ftest(dx, mu_live=False).cpu().numpy()[:, :-1].view(np.uint32), np.zeros_like(fresh[:, :-1]).view(np.uint32))
    assert np.array_equal(other.ftest(dx).cpu().numpy().view(np.uint32), fresh.view(np.uint32))        # (after a dead call too)


@pytest.mark.parametrize("form", ["single", "paired"])
def test_f_rows_stay_dense_on_a_pitched_plan(lib, oracle, torch_cuda, monkeypatch, form):
    """cfg.psd_pitch = 2112 at N = 4096: the PSD rows are 2112 floats apart, the F rows N/2 + 1 as the entry documents."""
    _select(monkeypatch, form)
    c = K.PLAN_CASES[-1]
    assert c.n == 4096
    raw, xf = K.reference(oracle, c)[:2]
    dx = _upload(torch_cuda, raw)
    sp = _plan(lib, c, psd_pitch=2112)
    assert sp.pitch == 2112 and sp.bins == 2049
    rc, got, intact = _ftest_into(lib, torch_cuda, sp, dx, 0, c.frames)
    assert rc == 0 and intact and not np.any(got.view(np.uint32) == SENTINEL)
    _judge("i", c, form + "-pitch", got, oracle)
    assert np.array_equal(got.view(np.uint32), _plan(lib, c).ftest(dx).cpu().numpy().view(np.uint32))
    psd = sp.run(dx).cpu().numpy()
    psd_w = oracle.spectrogram_mtm(xf, c.n, c.ovl, c.nw, c.kmax)
    assert psd.shape == (c.frames, 2112)
    assert max(max(rel_err(a[:2049], b)) for a, b in zip(psd, psd_w)) < TOL
