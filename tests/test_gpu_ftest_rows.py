"""GPU tests (-m gpu): the harmonic F rows bin by bin against float64, on every route of the F entry.

tests/test_gpu_ftest.py holds the F rows to the oracle under tests/_ftest_check.py, whose bound is weighed by a frame's largest num
and den: at a weak line beside a strong carrier it is larger than the line's F.  Here every bin below Nyquist of every frame is
held to tests/_ftest_rows_check.py's rule against tests/_exact.py::ftest64,

    | sqrt(got[k]) - f[k] | * b[k]  <=  tau * ( A + f[k] * ( T + A / sqrt(kmax) ) ),      tau = 4 * max(tau_f32, 2**-24)

with tau_f32 from the float32 stand-in on the CPU, never from the device or the oracle; the Nyquist column non-finite; a silent
frame the oracle's NaN pattern.  On `line` inputs the line's bin must hold the device's largest F outside the carrier's bins in
every settled frame.  The cases are tests/_ftest_rows_cases.py's; tests/test_ftest_rows_criterion.py shows on the CPU what the rule
accepts and rejects.  Routes: the per-bin epilogue (N < 256), one sequence per transform (GLFER_FTEST_PAIRED=0), two per transform
separated through the mirror bins (=1), and the default (paired from N = 2048); GLFER_FTEST_PAIRED is read on every call.

Lines starting with 'ftest-rows' (run with -s) are the record kept in profiles/ftest_rows.txt.
"""
import numpy as np
import pytest

import _ftest_rows_cases as K
from _ftest_rows_check import check_ftest_rows
from _rows_cases import mean2_condition

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _select(monkeypatch, form):
    if form in ("default", "epilogue"):
        monkeypatch.delenv("GLFER_FTEST_PAIRED", raising=False)
    else:
        monkeypatch.setenv("GLFER_FTEST_PAIRED", {"single": "0", "paired": "1"}[form])


def _with_forms(cases, forms=("default", "single", "paired")):
    """Below N = 256 there is one route; from there on the in-launch forms asked for."""
    return [pytest.param(c, form, id="%s-%s" % (K.case_id(c), form)) for c in cases for form in (forms if c.n >= 256 else ("epilogue",))]


def _plan(lib, oracle, c):
    fmt = {"f32": lib.SAMPLES_F32, "s16": lib.SAMPLES_S16, "u8": lib.SAMPLES_U8}[c.fmt]
    sp = lib.Spectrogram(lib.MtmParams(n=c.n, overlap=c.ovl, w=c.nw, kmax=c.kmax, sub_mean=c.sub_mean, history_mode=c.history_mode,
                                       sample_format=fmt))
    assert np.array_equal(sp.tapers()[0], K.tapers(oracle, c.n, c.kmax, c.nw))          # (the float64 parts are taken under the plan's tables)
    return sp


def _upload(torch, raw, offset=0):
    """The stream on the device; offset > 0: that many samples into its allocation."""
    if not offset:
        return torch.from_numpy(raw).cuda()
    return torch.from_numpy(np.concatenate([np.full(offset, 77, raw.dtype), raw])).cuda()[offset:]


def _judge(group, c, form, got, oracle, rows=slice(None)):
    """The rule on the device's rows `rows` of the case, the line's bin where the case has one, and the record line."""
    r = K.reference(oracle, c)
    want, num, den, tot = r.want[rows], r.num[rows], r.den[rows], r.tot[rows]
    assert got.shape == want.shape and got.dtype == np.float32
    what = "%s %s" % (K.case_id(c), form)
    with np.errstate(all="ignore"):
        worst, fr, k = check_ftest_rows(got, want, num, den, tot, c.kmax, r.tau, what)
    line = ""
    if c.signal in K.LINE_KINDS:
        first = rows.start or 0
        settled = [f - first for f in K.settled_frames(c) if first <= f < first + len(got)]
        out = ~K.excluded(c)
        for f in settled:
            top = int(np.flatnonzero(out)[np.argmax(got[f, :c.n // 2][out])])
            assert top == K.line_bin(c.n), "%s: frame %d: the largest F outside the carrier's bins is at bin %d (%g), the line's bin %d holds %g" % (
                what, f + first, top, got[f, top], K.line_bin(c.n), got[f, K.line_bin(c.n)])
        line = "  line bin %d largest in %d settled frames, least F %.4g" % (
            K.line_bin(c.n), len(settled), min(got[f, K.line_bin(c.n)] for f in settled) if settled else np.nan)
    print("ftest-rows %s %-9s N %-5d %-8s %-48s tau_f32 %.3e (paired stand-in %.3e) tau %.3e  device %.4f of the bound at frame %d bin %d%s" % (
        group, form, c.n, c.signal, K.case_id(c), r.tau_single, r.tau_paired, r.tau, worst, fr + (rows.start or 0) if fr >= 0 else -1, k, line))
    return worst


# ---- (a) every size, every form ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,form", _with_forms(K.SIZE_CASES + K.LONG_CASES))
def test_every_size_and_form(lib, oracle, torch_cuda, monkeypatch, c, form):
    _select(monkeypatch, form)
    raw = K.reference(oracle, c).raw
    _judge("a", c, form, _plan(lib, oracle, c).ftest(_upload(torch_cuda, raw)).cpu().numpy(), oracle)


# ---- (c) variations on `line` -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,form", _with_forms(K.FORMAT_CASES, ("single", "paired")))
def test_integer_samples_at_an_odd_offset(lib, oracle, torch_cuda, monkeypatch, c, form):
    _select(monkeypatch, form)
    raw = K.reference(oracle, c).raw
    assert raw.dtype == (np.int16 if c.fmt == "s16" else np.uint8)
    _judge("c-format", c, form, _plan(lib, oracle, c).ftest(_upload(torch_cuda, raw, K.FORMAT_OFFSET)).cpu().numpy(), oracle)


@pytest.mark.parametrize("c,form", _with_forms(K.MEAN_CASES, ("single", "paired")))
def test_mean_removal(lib, oracle, torch_cuda, monkeypatch, c, form):
    """sub_mean = 1 on `line` over a DC level; sub_mean = 2 on `line`, where every hop's mean is small against its rms and
    include/glfer_hip.h defines the in-kernel sums as the reference's rows."""
    _select(monkeypatch, form)
    r = K.reference(oracle, c)
    assert c.sub_mean == lib.SUBMEAN_EXACT or mean2_condition(c, r.xf)
    _judge("c-mean%d" % c.sub_mean, c, form, _plan(lib, oracle, c).ftest(_upload(torch_cuda, r.raw)).cpu().numpy(), oracle)


@pytest.mark.parametrize("c,form", _with_forms(K.HISTORY_CASES, ("single", "paired")))
def test_history_zeroed_in_every_frame(lib, oracle, torch_cuda, monkeypatch, c, form):
    _select(monkeypatch, form)
    assert c.history_mode == lib.HISTORY_ZERO_ALWAYS
    raw = K.reference(oracle, c).raw
    _judge("c-history", c, form, _plan(lib, oracle, c).ftest(_upload(torch_cuda, raw)).cpu().numpy(), oracle)


@pytest.mark.parametrize("cf,form", [pytest.param(cf, form, id="%s-first%d-%s" % (K.case_id(cf[0]), cf[1], form))
                                     for cf in K.RANGE_CASES for form in (("single", "paired") if cf[0].n >= 256 else ("epilogue",))])
def test_frame_range_inside_the_stream(lib, oracle, torch_cuda, monkeypatch, cf, form):
    c, first = cf
    _select(monkeypatch, form)
    raw = K.reference(oracle, c).raw
    nframes = c.frames - first - 3
    assert nframes > 0
    got = _plan(lib, oracle, c).ftest(_upload(torch_cuda, raw), first_frame=first, nframes=nframes).cpu().numpy()
    _judge("c-range", c, form, got, oracle, rows=slice(first, first + nframes))


# ---- (d) the other entries --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["single", "paired"])
def test_rows_and_f_entry(lib, oracle, torch_cuda, monkeypatch, form):
    _select(monkeypatch, form)
    c = K.ROWS_FTEST_CASE
    raw = K.reference(oracle, c).raw
    _, ft = _plan(lib, oracle, c).rows_ftest(_upload(torch_cuda, raw))
    _judge("d-rows_ftest", c, form, ft.cpu().numpy(), oracle)


@pytest.mark.parametrize("form", ["single", "paired"])
def test_batch_of_unlike_streams(lib, oracle, torch_cuda, monkeypatch, form):
    _select(monkeypatch, form)
    raws = [K.reference(oracle, c).raw for c in K.BATCH_MEMBERS]
    assert len({len(x) for x in raws}) == 1
    got = _plan(lib, oracle, K.BATCH_CASE).ftest_batch(torch_cuda.from_numpy(np.stack(raws)).cuda()).cpu().numpy()
    for b, c in enumerate(K.BATCH_MEMBERS):
        _judge("d-batch", c, form, got[b], oracle)


@pytest.mark.parametrize("form", ["single", "paired"])
def test_ragged_call_of_unlike_streams(lib, oracle, torch_cuda, monkeypatch, form):
    _select(monkeypatch, form)
    raws = [K.reference(oracle, c).raw for c in K.RAGGED_MEMBERS]
    assert len({len(x) for x in raws}) == len(raws)
    got = _plan(lib, oracle, K.RAGGED_CASE).ftest_list([torch_cuda.from_numpy(x).cuda() for x in raws])
    for b, c in enumerate(K.RAGGED_MEMBERS):
        _judge("d-ragged", c, form, got[b].cpu().numpy(), oracle)
