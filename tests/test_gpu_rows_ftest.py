"""The multitaper rows and the harmonic F rows from one pass over the samples (-m gpu): glfer_hip_mtm_rows_ftest_device /
Spectrogram.rows_ftest and the batch form.

  F rows    the bits of Spectrogram.ftest on the same plan, stream and form -- uint32 views, NaN and the Nyquist column's x/0
            included; no tolerance
  PSD (2)   bin by bin in amplitude against float64 (tests/_rows_check.py, the rule of tests/test_gpu_rows.py); tau comes from
            the float32 stand-in of tests/_exact.py, never from the device
  PSD (3)   per frame against the oracle's psd of the pair: max(1e-5, 1.1 err(oracle, exact))
  batch     every out[b] of both outputs holds the bits of rows_ftest(streams[b])

GLFER_FTEST_PAIRED is read on every call: 'single' = 0 (one sequence per transform), 'paired' = 1 (two, separated through
the mirror bins).  The cases are tests/_rows_ftest_cases.py's; tests/test_rows_ftest_host.py runs the reference alone over
every one of them without a GPU.  Lines starting with 'rows-ftest' (run with -s) are the record.
"""
import ctypes as C

import numpy as np
import pytest

import _ftest_cases as K
import _rows_ftest_cases as R
from _rows_check import check_rows, tau_of
from _signals import synth

pytestmark = pytest.mark.gpu
E_ARG = -1                                # GLFER_E_ARG (include/glfer_hip.h)
SENTINEL = 0x5A5A5A5A                     # (3.76e16 as a float: no row holds it)
PAD = 96                                  # guard floats either side of an output
FORMS = R.FORMS


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _select(monkeypatch, form):
    monkeypatch.setenv("GLFER_FTEST_PAIRED", {"single": "0", "paired": "1"}[form])


_PLANS = {}


def _plan(lib, c, **kw):
    """One plan per configuration for the whole module (the form is read per call)."""
    fmt = {"f32": lib.SAMPLES_F32, "s16": lib.SAMPLES_S16, "u8": lib.SAMPLES_U8}[c.fmt]
    key = (c.n, c.ovl, c.nw, c.kmax, fmt, c.sub_mean, c.history_mode, tuple(sorted(kw.items())))
    if key not in _PLANS:
        _PLANS[key] = lib.Spectrogram(lib.MtmParams(n=c.n, overlap=c.ovl, w=c.nw, kmax=c.kmax, sub_mean=c.sub_mean,
                                                    history_mode=c.history_mode, sample_format=fmt, **kw))
    return _PLANS[key]


def _upload(torch, raw, offset=0):
    if not offset:
        return torch.from_numpy(raw).cuda()
    return torch.from_numpy(np.concatenate([np.full(offset, 77, raw.dtype), raw])).cuda()[offset:]


def _bits(torch, t):
    return t.contiguous().view(torch.int32)


def _guarded(torch, shape):
    """A sentinel-filled buffer with PAD guard floats either side: (whole buffer as int32, the float view of `shape`)."""
    count = int(np.prod(shape))
    buf = torch.full((PAD + count + PAD,), SENTINEL, dtype=torch.int32, device="cuda:0")
    return buf, buf[PAD:PAD + count].view(torch.float32).view(*shape)


def _guards_ok(torch, buf):
    return bool((buf[:PAD] == SENTINEL).all()) and bool((buf[-PAD:] == SENTINEL).all())


def _call(torch, sp, x, first=0, nframes=None, mu_live=True):
    """rows_ftest into guarded buffers; checks the guards, that every F value was written and the PSD floats between bins and
    the pitch were not, and that the F rows are ftest()'s bits.  Returns (psd [nframes][bins] numpy, ftest tensor)."""
    nframes = sp.num_frames(x.numel()) - first if nframes is None else nframes
    assert nframes > 0
    pbuf, psd = _guarded(torch, (nframes, sp.pitch))
    fbuf, ft = _guarded(torch, (nframes, sp.bins))
    got = sp.rows_ftest(x, first_frame=first, nframes=nframes, mu_live=mu_live, out=(psd, ft))
    want = sp.ftest(x, first_frame=first, nframes=nframes, mu_live=mu_live)
    torch.cuda.synchronize()
    assert got[0].data_ptr() == psd.data_ptr() and got[1].data_ptr() == ft.data_ptr()
    assert _guards_ok(torch, pbuf) and _guards_ok(torch, fbuf), "the entry wrote outside its rows"
    assert not bool((_bits(torch, ft) == SENTINEL).any()) and not bool((_bits(torch, psd[:, :sp.bins]) == SENTINEL).any())
    if sp.pitch > sp.bins:
        assert bool((_bits(torch, psd[:, sp.bins:]) == SENTINEL).all()), "floats between bins and the pitch were written"
    assert torch.equal(_bits(torch, ft), _bits(torch, want)), "F rows differ from the F entry's bits"
    return psd[:, :sp.bins].cpu().numpy(), ft


def _judge(group, c, form, got, r, rows=slice(None)):
    """PSD rows under rule (2) and rule (3); prints the record line."""
    exact = r.exact[rows]
    what = "%s %s %s" % (group, K.case_id(c), form)
    dev = tau_of(got, exact)
    print("rows-ftest %-2s %-44s %-10s device tau %.3e bound %.3e fraction %.3f tau_f32 %.3e" % (
        group, K.case_id(c), form, dev, r.tau, dev / r.tau, r.tau_f32), end="")
    check_rows(got, exact, r.tau, what)
    frac = R.check_against_oracle(got, r, rows, what)
    print(" oracle rule %.3f of its bound (oracle/float64 %.3e)" % (frac, r.e_ref))


# ---- (1)-(3) every path, both forms, mu live and dead ------------------------------------------------------------------
@pytest.mark.parametrize("mu_live", [True, False], ids=["mu1", "mu0"])
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("c", R.SIZE_CASES, ids=K.case_id)
def test_every_size_and_form(lib, oracle, torch_cuda, monkeypatch, c, form, mu_live):
    torch = torch_cuda
    _select(monkeypatch, form)
    r = R.reference(oracle, c)
    sp = _plan(lib, c)
    v, sig = sp.tapers()
    ov, osig = oracle.dpss(c.n, c.kmax, c.nw)
    assert np.array_equal(v, ov) and np.array_equal(sig, osig)
    psd, ft = _call(torch, sp, _upload(torch, r.raw), mu_live=mu_live)
    _judge("a", c, "%s-mu%d" % (form, mu_live), psd, r)
    half = c.n // 2
    if mu_live:
        assert bool(torch.isfinite(ft[:, :half]).all()) and not bool(torch.isfinite(ft[:, half]).any())
    else:                                               # (the reference build without FFTW: +0.0 below Nyquist, 0/0 at it)
        assert bool((_bits(torch, ft[:, :half]) == 0).all()) and bool(torch.isnan(ft[:, half]).all())


# ---- (4) everything an F entry can be asked ------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("c", R.FORMAT_CASES, ids=K.case_id)
def test_integer_sample_formats(lib, oracle, torch_cuda, monkeypatch, c, form):
    _select(monkeypatch, form)
    r = R.reference(oracle, c)
    assert r.raw.dtype == (np.int16 if c.fmt == "s16" else np.uint8)
    psd, _ = _call(torch_cuda, _plan(lib, c), _upload(torch_cuda, r.raw, R.FORMAT_OFFSET))
    _judge("d", c, form, psd, r)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("c", R.MEAN_CASES, ids=K.case_id)
def test_mean_removal(lib, oracle, torch_cuda, monkeypatch, c, form):
    _select(monkeypatch, form)
    r = R.reference(oracle, c)
    psd, _ = _call(torch_cuda, _plan(lib, c), _upload(torch_cuda, r.raw))
    _judge("e", c, form, psd, r)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("c", R.HISTORY_CASES, ids=K.case_id)
def test_history_zeroed_in_every_frame(lib, oracle, torch_cuda, monkeypatch, c, form):
    _select(monkeypatch, form)
    assert c.history_mode == lib.HISTORY_ZERO_ALWAYS
    r = R.reference(oracle, c)
    psd, _ = _call(torch_cuda, _plan(lib, c), _upload(torch_cuda, r.raw))
    _judge("f", c, form, psd, r)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("cf", R.RANGE_CASES, ids=lambda cf: "%s-first%d" % (K.case_id(cf[0]), cf[1]))
def test_frame_range_inside_the_stream(lib, oracle, torch_cuda, monkeypatch, cf, form):
    """first_frame > 0 and the launch ending 3 frames before the stream does."""
    c, first = cf
    _select(monkeypatch, form)
    nframes = c.frames - first - 3
    assert nframes > 0
    r = R.reference(oracle, c)
    psd, _ = _call(torch_cuda, _plan(lib, c), _upload(torch_cuda, r.raw), first=first, nframes=nframes)
    _judge("f", c, "%s-first%d" % (form, first), psd, r, rows=slice(first, first + nframes))


@pytest.mark.parametrize("c", R.LONG_CASES, ids=K.case_id)
def test_more_frames_than_one_pass_of_the_grid(lib, oracle, torch_cuda, monkeypatch, c):
    """N = 16: 40 001 frames, two groups of the epilogue route; N = 256 / 2048: past one pass of the persistent grid by a
    prime, the form the launcher chooses by default (one sequence per transform at 256, two at 2048)."""
    monkeypatch.delenv("GLFER_FTEST_PAIRED", raising=False)
    r = R.reference(oracle, c)
    psd, _ = _call(torch_cuda, _plan(lib, c), _upload(torch_cuda, r.raw))
    _judge("g", c, "default", psd, r)


@pytest.mark.parametrize("form", FORMS)
def test_psd_rows_at_the_pitch_f_rows_dense(lib, oracle, torch_cuda, monkeypatch, form):
    """cfg.psd_pitch = 2112 at N = 4096: PSD rows 2112 floats apart with the floats past the bins untouched (_call), F rows
    dense; both the bits of the dense plan's."""
    torch = torch_cuda
    _select(monkeypatch, form)
    c = R.PITCH_CASE
    r = R.reference(oracle, c)
    sp = _plan(lib, c, psd_pitch=R.PITCH)
    assert sp.pitch == R.PITCH and sp.bins == c.n // 2 + 1
    x = _upload(torch, r.raw)
    psd, ft = _call(torch, sp, x)
    _judge("h", c, "%s-pitch" % form, psd, r)
    dpsd, dft = _plan(lib, c).rows_ftest(x)
    assert np.array_equal(dpsd.cpu().numpy().view(np.uint32), psd.view(np.uint32))
    assert torch.equal(_bits(torch, dft), _bits(torch, ft))


# ---- (5) the plan after the call -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("first_f_call", ["ftest", "rows_ftest"])
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("n,sub_mean", [(64, 0), (512, 1), (2048, 0), (4096, 0)])
def test_plan_after_the_call(lib, torch_cuda, monkeypatch, n, sub_mean, form, first_f_call):
    """run() and ftest() return after a rows_ftest call the bits they returned before it, whichever entry made the F tables."""
    torch = torch_cuda
    _select(monkeypatch, form)
    mk = lambda: lib.Spectrogram(lib.MtmParams(n=n, overlap=0.5, w=2.5, kmax=4, sub_mean=sub_mean))
    x = torch.from_numpy(0.8 * synth(11 * (n // 2) + 5, seed=n) + np.float32(0.02)).cuda()
    ref = mk()                                           # a plan that never sees the new entry
    r_want, f_want, d_want = ref.run(x), ref.ftest(x), ref.ftest(x, mu_live=False)
    sp = mk()
    r_before = sp.run(x)
    if first_f_call == "ftest":
        assert torch.equal(_bits(torch, sp.ftest(x)), _bits(torch, f_want))
    psd, ft = sp.rows_ftest(x)
    _, ft0 = sp.rows_ftest(x, mu_live=False)
    torch.cuda.synchronize()
    assert torch.equal(_bits(torch, ft), _bits(torch, f_want)) and torch.equal(_bits(torch, ft0), _bits(torch, d_want))
    assert torch.equal(_bits(torch, r_before), _bits(torch, r_want))
    assert torch.equal(_bits(torch, sp.run(x)), _bits(torch, r_want))
    assert torch.equal(_bits(torch, sp.ftest(x)), _bits(torch, f_want))
    assert torch.equal(_bits(torch, sp.ftest(x, mu_live=False)), _bits(torch, d_want))
    again, _ = sp.rows_ftest(x)
    assert torch.equal(_bits(torch, again), _bits(torch, psd))
    for s in (ref, sp):
        s.close()


# ---- (6) batch equals loop ---------------------------------------------------------------------------------------------------
def _streams(torch, lib, fmt, nb, nsamples, pitch=None, gap=None):
    """[nb, nsamples] view of a [nb, pitch] buffer of the plan's sample type: streams that differ in seed, amplitude and DC
    level; the pitch - nsamples samples after each stream hold `gap`."""
    pitch = pitch or nsamples
    if fmt != lib.SAMPLES_F32:
        pitch += pitch & 1                             # integer samples: an even stream pitch (glfer_hip.h)
    out = np.zeros((nb, pitch), np.float64)
    for b in range(nb):
        amp = 0.4 + 0.6 * ((b * 7919) % 11) / 10.0
        out[b, :nsamples] = amp * synth(nsamples, seed=1000 + b) + 0.05 * (((b * 104729) % 9) - 4)
    if fmt == lib.SAMPLES_F32:
        buf = out.astype(np.float32)
    else:
        buf = np.clip(np.round(out * 20000.0), -32768, 32767).astype(np.int16)
    if gap is not None and pitch > nsamples:
        buf[:, nsamples:] = gap
    return torch.from_numpy(buf).to("cuda:0")[:, :nsamples]


def _check_batch(torch, sp, x, mu_live=True):
    nb = x.size(0)
    nframes = sp.num_frames(x.size(1))
    pbuf, psd = _guarded(torch, (nb, nframes, sp.pitch))
    fbuf, ft = _guarded(torch, (nb, nframes, sp.bins))
    got = sp.rows_ftest_batch(x, mu_live=mu_live, out=(psd, ft))
    torch.cuda.synchronize()
    assert got[0].data_ptr() == psd.data_ptr() and got[1].data_ptr() == ft.data_ptr()
    assert _guards_ok(torch, pbuf) and _guards_ok(torch, fbuf), "the entry wrote outside its rows"
    assert not bool((_bits(torch, ft) == SENTINEL).any()) and not bool((_bits(torch, psd) == SENTINEL).any())
    bad = []
    for b in range(nb):
        wp, wf = sp.rows_ftest(x[b], mu_live=mu_live)
        if not (torch.equal(_bits(torch, psd[b]), _bits(torch, wp)) and torch.equal(_bits(torch, ft[b]), _bits(torch, wf))):
            bad.append(b)
    assert not bad, ("streams whose rows differ from the single entry's", bad[:8])
    for a in range(nb - 1):                            # the streams do differ
        assert not torch.equal(_bits(torch, psd[a]), _bits(torch, psd[a + 1])), a
    assert bool(torch.isfinite(psd).all())


BATCH_SHAPES = {"n64": 17, "n256": 21, "n2048_k3": 9, "n4096": 5}     # shape -> frames per stream


@pytest.mark.parametrize("nb", [3, 37])
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("shape", sorted(BATCH_SHAPES))
def test_batch_equals_loop(lib, torch_cuda, monkeypatch, shape, form, nb):
    """N = 64 goes stream by stream inside the call; the others in the launches of one stream."""
    _select(monkeypatch, form)
    sp = _plan(lib, R.shape_case(shape))
    _check_batch(torch_cuda, sp, _streams(torch_cuda, lib, lib.SAMPLES_F32, nb, BATCH_SHAPES[shape] * sp.hop + sp.hop // 3))


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("kind", ["sub_mean", "s16", "gap"])
def test_batch_variants(lib, torch_cuda, monkeypatch, kind, form):
    """Mean removal through the batch's corrected copies, 16-bit samples, and NaN between the streams (stride(0) > T)."""
    torch = torch_cuda
    _select(monkeypatch, form)
    if kind == "sub_mean":
        sp = _plan(lib, R.shape_case("n2048_k3", sub_mean=1))
        x = _streams(torch, lib, lib.SAMPLES_F32, 5, 9 * sp.hop + 7)
    elif kind == "s16":
        sp = _plan(lib, R.shape_case("n256", fmt="s16"))
        x = _streams(torch, lib, lib.SAMPLES_S16, 5, 21 * sp.hop)
        assert x.stride(0) % 2 == 0
    else:
        sp = _plan(lib, R.shape_case("n4096"))
        nsamples = 5 * sp.hop
        x = _streams(torch, lib, lib.SAMPLES_F32, 5, nsamples, pitch=nsamples + 2 * sp.n + 6, gap=np.float32(np.nan))
        assert x.stride(0) > nsamples
    _check_batch(torch, sp, x)
    _check_batch(torch, sp, x, mu_live=False)


def test_batch_past_one_pass_of_the_shared_grid(lib, torch_cuda, monkeypatch):
    """Three streams of the N = 2048 long count each: every stream has more frames than its share of the grid holds in a pass."""
    monkeypatch.delenv("GLFER_FTEST_PAIRED", raising=False)
    c = [c for c in R.LONG_CASES if c.n == 2048][0]
    sp = _plan(lib, c)
    _check_batch(torch_cuda, sp, _streams(torch_cuda, lib, lib.SAMPLES_F32, 3, c.frames * sp.hop + 3))


# ---- (7) refusals and empty calls ------------------------------------------------------------------------------------------
def test_refusals_and_empty_calls(lib, torch_cuda, monkeypatch):
    torch = torch_cuda
    monkeypatch.delenv("GLFER_FTEST_PAIRED", raising=False)
    L = lib.api.lib()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    vp = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None

    def outs(sp, rows):
        return (torch.full((rows * sp.pitch,), SENTINEL, dtype=torch.int32, device="cuda:0"),
                torch.full((rows * sp.bins,), SENTINEL, dtype=torch.int32, device="cuda:0"))

    def untouched(o):
        torch.cuda.synchronize()
        return bool((o[0] == SENTINEL).all()) and bool((o[1] == SENTINEL).all())

    def single(sp, x, nsamples, first, nframes, o, psd=True, ft=True, stream=True):
        rc = L.glfer_hip_mtm_rows_ftest_device(sp._h, vp(x if stream else None), nsamples, first, nframes, vp(o[0] if psd else None),
                                               vp(o[1] if ft else None), 1, st)
        return rc, untouched(o)

    def batch(sp, x, nb, pitch, nsamples, first, nframes, o, psd=True, ft=True, stream=True):
        rc = L.glfer_hip_mtm_rows_ftest_batch_device(sp._h, vp(x if stream else None), nb, pitch, nsamples, first, nframes,
                                                     vp(o[0] if psd else None), vp(o[1] if ft else None), 1, st)
        return rc, untouched(o)

    n, frames = 1024, 8
    s16 = lib.Spectrogram(lib.MtmParams(n=n, overlap=0.0, w=2.5, kmax=4, sample_format=1))
    x = torch.zeros((4, 2 * frames * n), dtype=torch.int16, device="cuda:0")
    pitch, nsamples = 2 * frames * n, frames * n
    o = outs(s16, 27)
    # a plan that is not MTM, and an MTM plan above the entries' range: before everything but the NULL plan (empty calls too)
    per = lib.Spectrogram(lib.FftParams(n=1024, window_type=0, overlap=0.0))
    big = lib.Spectrogram(lib.MtmParams(n=32768, overlap=0.0, w=2.0, kmax=2))
    xf = torch.zeros((3, 2 * 32768), device="cuda:0")
    for sp_bad in (per, big):
        ob = outs(sp_bad, 6)
        assert single(sp_bad, xf, 2 * 32768, 0, 2, ob) == (E_ARG, True)
        assert single(sp_bad, xf, 2 * 32768, 0, 0, ob) == (E_ARG, True)
        assert batch(sp_bad, xf, 3, 2 * 32768, 2 * 32768, 0, 2, ob) == (E_ARG, True)
        assert batch(sp_bad, xf, 0, 2 * 32768, 2 * 32768, 0, 2, ob) == (E_ARG, True)
    with pytest.raises(lib.GlferHipError, match="bad argument"):
        big.rows_ftest_batch(xf)
    with pytest.raises(lib.GlferHipError, match="bad argument"):
        big.rows_ftest(xf[0])
    # empty calls: GLFER_OK with nothing launched, before the pointer and range checks
    assert single(s16, x, nsamples, 0, 0, o) == (0, True)
    assert single(s16, x, nsamples, frames + 5, 0, o, psd=False, ft=False, stream=False) == (0, True)
    assert batch(s16, x, 0, pitch, nsamples, 0, 4, o) == (0, True)
    assert batch(s16, x, 3, pitch, nsamples, 0, 0, o) == (0, True)
    assert batch(s16, x, 3, pitch - 1, nsamples, frames + 5, 0, o, psd=False, ft=False, stream=False) == (0, True)
    # NULL pointers: both outputs are required
    for kw in ({"stream": False}, {"psd": False}, {"ft": False}):
        assert single(s16, x, nsamples, 0, 4, o, **kw) == (E_ARG, True), kw
        assert batch(s16, x, 3, pitch, nsamples, 0, 4, o, **kw) == (E_ARG, True), kw
    # a frame past the stream
    assert single(s16, x, nsamples, 0, frames + 1, o) == (E_ARG, True)
    assert single(s16, x, nsamples, frames, 1, o) == (E_ARG, True)
    assert batch(s16, x, 3, pitch, nsamples, 0, frames + 1, o) == (E_ARG, True)
    assert batch(s16, x, 3, pitch, nsamples, frames, 1, o) == (E_ARG, True)
    # nframes > 0x7fffffff (inside a stream that long on paper)
    assert single(s16, x, (1 << 32) * n, 0, 1 << 31, o) == (E_ARG, True)
    assert batch(s16, x, 3, pitch, (1 << 32) * n, 0, 1 << 31, o) == (E_ARG, True)
    # an odd stream pitch with s16 samples
    assert batch(s16, x, 3, pitch - 1, nsamples, 0, 4, o) == (E_ARG, True)
    # sizes that overflow size_t
    assert batch(s16, x, 1 << 62, pitch, nsamples, 0, 4, o) == (E_ARG, True)
    # the same calls, well formed: rows written
    assert single(s16, x, nsamples, 0, 4, o) == (0, False)
    o = outs(s16, 27)
    assert batch(s16, x, 3, pitch, nsamples, 0, 4, o) == (0, False)
    for s in (s16, per, big):
        s.close()
