"""GPU tests (-m gpu): the periodogram's non-linear pre-processing -- RA9MB x / (a + x^2) (fft.c:127-136) and the limiter
sign(y) |y|^0.1 (fft.c:151-156) -- bin by bin in amplitude against float64, on every kernel route.

The other tests of this path (tests/test_gpu_round4.py's test_limiter_at_the_usual_tolerance, two golden files, one loop of
test_block_sizes_outside_the_16_point_range) normalise by a row's largest bin at 1e-5; the limiter flattens a frame, its
spectrum is broad, and a drifted branch passes that (tests/test_nonlin_criterion.py shows two).  Here every bin of every frame
is held to tests/test_gpu_rows.py's rule

    | sqrt(got[k]) - sqrt(exact[k]) |  <=  tau * sqrt( sum_k exact[k] ),    tau = 4 * max(tau_f32, 2**-24)

with `exact` the float64 rows and tau_f32 the float32 stand-in's of tests/_nonlin_exact.py, computed on the CPU per case, never
from device output.  Beside it, per frame, the suite's peak-normalised rule against the oracle stays asserted: 1e-5, and from
N = 8192 max(1e-5, 1.1 x err(oracle, exact)).  The cases are tests/_nonlin_cases.py's; that module says how the limiter's jump
at 0 is kept out of them.

Five copies of the gather -> RA9MB -> window -> limiter -> post_scale sequence exist, and the record names the one a launch runs
(tests/_nonlin_cases.py kernel_file, after glfer_hip.cpp's body_route and launch_wave_private):
  spectro_small.hip   N < 256
  spectro16.hip       N = 256 ... 16384, the general form of the packed kernel (two wavefronts per SIMD), whatever GLFER_FORM says
  spectro16w.hip      N = 32768, its general form, ONLY for run(spectrum=True) and under GLFER_FORM=w: test_halfcomplex_spectra
                      and test_the_wave_private_form_at_32768, which gives this copy the formats, offsets, means, zeroed history and
                      frame ranges the other copies get
  spectro_big.hip     N = 32768 by default and every N from 65536, the two-level combine from N = 131072
  stats_kernels.hip   prepare_kernel: Spectrogram.prepare, held to the CPU restatement sample by sample
From N = 32768 both files read the plan's UNSCALED window table; the scale follows the limiter as post_scale.
A plan with mean removal reaches these through the corrected copy of the stream whatever GLFER_MEAN_PREPASS says
(glfer_hip.cpp mean_inkernel_ok: no table form for a non-linear plan): the rows under GLFER_MEAN_PREPASS=1 are asserted to be
the default's bit for bit and are not recorded a second time.

Lines starting with 'nonlin-bin-by-bin' (run with -s) are the record kept in profiles/nonlin_rows.txt.
"""
import numpy as np
import pytest

import _nonlin_cases as N
import _nonlin_exact as NX
import _rows_cases as K
from _rows_check import bound, check_rows, check_spectrum, from_halfcomplex, tau_of, tau_of_spectrum
from _signals import rel_err

pytestmark = pytest.mark.gpu
ENV = ("GLFER_FORM", "GLFER_MEAN_PREPASS", "GLFER_INGEST_CHUNK")
RECORD = "nonlin-bin-by-bin %-2s %-56s %-10s %-17s device tau %.3e bound %.3e fraction %.3f tau_f32 %.3e oracle tau %.3e"


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


@pytest.fixture(autouse=True)
def _default_forms(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)


def _fmt(lib, c):
    return {"f32": lib.SAMPLES_F32, "s16": lib.SAMPLES_S16, "u8": lib.SAMPLES_U8}[c.fmt]


def _plan(lib, oracle, c, sub_mean=None, **kw):
    """The case's plan; its float32 window is the one the float64 rows were made with."""
    sp = lib.Spectrogram(lib.FftParams(n=c.n, window_type=lib.WINDOWS[c.window], overlap=c.ovl, a=c.a, limiter=c.limiter,
                                       sub_mean=c.sub_mean if sub_mean is None else sub_mean, history_mode=c.history_mode,
                                       sample_format=_fmt(lib, c), **kw))
    assert np.array_equal(sp.window(), oracle.window(oracle.WINDOWS[c.window], c.n))
    return sp


def _upload(torch, raw, offset=0):
    """The stream on the device; offset > 0: that many samples into its allocation."""
    if not offset:
        return torch.from_numpy(raw).cuda()
    host = np.concatenate([np.full(offset, 77, raw.dtype), raw])
    return torch.from_numpy(host).cuda()[offset:]


def _judge(group, c, form, got, r, rows=slice(None), w_form=False):
    """Device rows against the float64 rows under (1) and against the oracle under the suite's rule; prints the record line."""
    exact, want = r.exact[rows], r.want[rows]
    got = np.asarray(got)
    assert got.shape == exact.shape, (got.shape, exact.shape)
    what = "%s %s %s" % (group, N.case_id(c), form)
    dev_tau = tau_of(got, exact)
    print(RECORD % (group, N.case_id(c), form, N.kernel_file(c, w_form), dev_tau, r.tau, dev_tau / r.tau, r.tau_f32, r.tau_oracle))
    frac = check_rows(got, exact, r.tau, what)
    for f in range(len(want)):
        if want[f].any():
            e_dev, e_ref = max(rel_err(got[f], want[f])), max(rel_err(want[f], exact[f]))
            assert e_dev <= K.oracle_bound(c, e_ref), (what, f, e_dev, e_ref)
        else:
            assert not got[f].any(), (what, f)                  # silence stays silence
    return frac


def _run(lib, oracle, torch, c, sub_mean=None, offset=0, **kw):
    r = N.reference(oracle, c)
    sp = _plan(lib, oracle, c, sub_mean)
    got = sp.run(_upload(torch, r.raw, offset), **kw).cpu().numpy()
    sp.close()
    return got, r


# ---- (a) every size of every route under the three settings; (b) single samples, single bins, dither, silence ------------
@pytest.mark.parametrize("c", N.SIZE_CASES, ids=N.case_id)
def test_every_size_and_setting(lib, oracle, torch_cuda, c):
    got, r = _run(lib, oracle, torch_cuda, c)
    _judge("a", c, "default", got, r)


@pytest.mark.parametrize("c", N.EDGE_CASES, ids=N.case_id)
def test_single_samples_dither_and_silence(lib, oracle, torch_cuda, c):
    got, r = _run(lib, oracle, torch_cuda, c, offset=1 if c.fmt != "f32" and c.n == 4096 else 0)
    _judge("b", c, "default", got, r)
    if c.signal == "zero":
        assert not r.exact.any() and not got.any()


# ---- (c) 16-bit and 8-bit samples ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", N.FORMAT_CASES, ids=N.case_id)
def test_integer_sample_formats(lib, oracle, torch_cuda, c):
    off = N.FORMAT_OFFSETS.get(N.case_id(c), 0)
    got, r = _run(lib, oracle, torch_cuda, c, offset=off)
    assert r.raw.dtype == (np.int16 if c.fmt == "s16" else np.uint8)
    _judge("c", c, "offset%d" % off, got, r)


# ---- (d) mean removal ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", N.MEAN_CASES, ids=N.case_id)
def test_mean_removal_in_the_references_order(lib, oracle, torch_cuda, monkeypatch, c):
    """sub_mean = 1: the only mean a limiter case is run with -- the reference's own sum, so no sample changes sign at the
    limiter's jump.  A non-linear plan has no table form (mean_inkernel_ok): the launcher's own choice and GLFER_MEAN_PREPASS=1
    are both the corrected copy, and the second must give the first's rows bit for bit."""
    assert N.limiter_condition(c, N.reference(oracle, c).xf)
    got, r = _run(lib, oracle, torch_cuda, c, sub_mean=lib.SUBMEAN_EXACT)
    _judge("d", c, "m1", got, r)
    monkeypatch.setenv("GLFER_MEAN_PREPASS", "1")
    again, _ = _run(lib, oracle, torch_cuda, c, sub_mean=lib.SUBMEAN_EXACT)
    assert np.array_equal(again.view(np.uint32), got.view(np.uint32))


@pytest.mark.parametrize("c", N.MEAN2_CASES, ids=N.case_id)
def test_ra9mb_with_the_in_kernel_sums(lib, oracle, torch_cuda, c):
    """sub_mean = 2 under RA9MB alone, which is smooth, on the inputs whose hop means are small against the rms."""
    assert not c.limiter and K.mean2_condition(c, N.reference(oracle, c).xf)
    got, r = _run(lib, oracle, torch_cuda, c, sub_mean=lib.SUBMEAN_FAST)
    _judge("d", c, "m2", got, r)


# ---- (e) history, frame ranges ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", N.HISTORY_CASES, ids=N.case_id)
def test_history_zeroed_in_every_frame(lib, oracle, torch_cuda, c):
    assert c.history_mode == lib.HISTORY_ZERO_ALWAYS
    got, r = _run(lib, oracle, torch_cuda, c)
    _judge("e", c, "default", got, r)


@pytest.mark.parametrize("cf", N.RANGE_CASES, ids=lambda cf: "%s-first%d" % (N.case_id(cf[0]), cf[1]))
def test_frame_range_inside_the_stream(lib, oracle, torch_cuda, cf):
    c, first = cf
    nframes = c.frames - first - 3
    assert nframes > 0
    got, r = _run(lib, oracle, torch_cuda, c, first_frame=first, nframes=nframes)
    _judge("e", c, "first%d" % first, got, r, rows=slice(first, first + nframes))
    whole, _ = _run(lib, oracle, torch_cuda, c)
    _judge("e", c, "whole", whole, r)


# ---- (f) rows on a pitch, halfcomplex spectra ------------------------------------------------------------------------------
@pytest.mark.parametrize("cp", N.PITCH_CASES, ids=lambda cp: "%s-pitch%d" % (N.case_id(cp[0]), cp[1]))
def test_rows_on_a_pitch(lib, oracle, torch_cuda, cp):
    c, pitch = cp
    r = N.reference(oracle, c)
    dx = _upload(torch_cuda, r.raw)
    sp = _plan(lib, oracle, c, psd_pitch=pitch)
    bins = c.n // 2 + 1
    assert sp.pitch == pitch and sp.bins == bins
    got = sp.run(dx).cpu().numpy()
    assert got.shape == (c.frames, pitch)
    _judge("f", c, "pitch%d" % pitch, got[:, :bins], r)
    dense = _plan(lib, oracle, c).run(dx).cpu().numpy()
    assert np.array_equal(dense.view(np.uint32), got[:, :bins].view(np.uint32))


@pytest.mark.parametrize("c", N.SPECTRUM_CASES, ids=N.case_id)
def test_halfcomplex_spectra(lib, oracle, torch_cuda, c):
    """run(spectrum=True): the spectrum of the pre-processed frame, |got_X[k] - exact_X[k]| / sqrt(N) <= tau sqrt(sum_k P_k), so a
    phase error counts; and the rows of that launch under (1)."""
    raw, xf, exact_X, t32, tau = N.spectrum_reference(oracle, c)
    sp = _plan(lib, oracle, c)
    psd, spec = sp.run(_upload(torch_cuda, raw), spectrum=True)
    got_X = from_halfcomplex(spec.cpu().numpy())
    dev = tau_of_spectrum(got_X, exact_X, c.n)
    prepared = NX.prepared32(xf, c.n, c.ovl, N.window(oracle, c), c.a, c.limiter, c.sub_mean, c.history_mode)
    want_X = from_halfcomplex(np.stack([oracle.rfft_halfcomplex(row) for row in prepared]))
    print(RECORD % ("f", N.case_id(c), "spectrum", N.kernel_file(c, True), dev, tau, dev / tau, t32, tau_of_spectrum(want_X, exact_X, c.n)))
    check_spectrum(got_X, exact_X, c.n, tau, N.case_id(c))
    _judge("f", c, "spec-psd", psd.cpu().numpy(), N.reference(oracle, c), w_form=True)
    sp.close()


# ---- (g) spectro16w.hip's copy beyond spectrum=True: N = 32768 under GLFER_FORM=w -------------------------------------
@pytest.mark.parametrize("cf", N.W_CASES, ids=lambda cf: "%s-first%s" % (N.case_id(cf[0]), cf[1]))
def test_the_wave_private_form_at_32768(lib, oracle, torch_cuda, monkeypatch, cf):
    """By default N = 32768 runs spectro_big.hip; GLFER_FORM=w (read per launch) sends it to spectro16w.hip's general form, whose
    non-linear branch the spectrum=True cases alone would reach in f32 only.  The same case under the default is judged beside
    it (spectro_big.hip); RA9MB alone with mean removal is also run with the in-kernel sums' value, sub_mean = 2."""
    c, first = cf
    assert c.n == 32768
    off = N.W_OFFSETS.get(N.case_id(c), 0)
    kw = {} if first is None else dict(first_frame=first, nframes=c.frames - first - 3)
    rows = slice(None) if first is None else slice(first, c.frames - 3)
    tag = ("offset%d" % off if off else "m1" if c.sub_mean else "whole") if first is None else "first%d" % first
    m = lib.SUBMEAN_EXACT if c.sub_mean else 0
    got, r = _run(lib, oracle, torch_cuda, c, sub_mean=m, offset=off, **kw)
    _judge("g", c, tag, got, r, rows)
    monkeypatch.setenv("GLFER_FORM", "w")
    got, r = _run(lib, oracle, torch_cuda, c, sub_mean=m, offset=off, **kw)
    _judge("g", c, "w-" + tag, got, r, rows, w_form=True)
    if c in N.MEAN2_CASES:
        got, r = _run(lib, oracle, torch_cuda, c, sub_mean=lib.SUBMEAN_FAST)
        _judge("g", c, "w-m2", got, r, w_form=True)


# ---- prepare_kernel, the fifth copy ------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["f32", "s16", "u8"])
@pytest.mark.parametrize("n", [64, 1024, 4096, 32768])
def test_prepare_against_the_cpu_restatement(lib, oracle, torch_cuda, n, fmt):
    """What prepare_audio leaves in inbuf_fft (Spectrogram.prepare) against tests/_nonlin_exact.py's float32 restatement of
    fft.c:127-156: bit for bit without the limiter -- one float division, one float add of a float product, one float multiply;
    with it within the 4 units in the last place that test_prepare_audio_frames allows the device's double log / exp."""
    for setting, ovl, window, signal in ((N.RA_S, 0.5, "blackman", "synth"), (N.RA_L, 0.0, "rectangular", "full"),
                                         (N.LIM, 0.75, "hanning", "weak"), (N.BOTH_L, 0.33, "kaiser", "noise"), (N.BOTH_S, 0.0, "hanning", "tiny" if fmt == "f32" else "lsb1")):
        c = N.nl(n, ovl, window, setting, signal, fmt, frames=5)
        raw, xf = N.make_input(oracle, c)
        sp = _plan(lib, oracle, c)
        got = sp.prepare(_upload(torch_cuda, raw, 3 if n == 1024 else 0)).cpu().numpy()
        sp.close()
        want = NX.prepared32(xf, c.n, c.ovl, N.window(oracle, c), c.a, c.limiter)
        assert got.shape == want.shape == (c.frames, n)
        what = (N.case_id(c), "prepare")
        zero = want == 0
        assert not got[zero].any(), what                        # (Hanning's end point, zero history: log 0 = -inf, exp(-inf) = 0)
        ulps = np.abs(got[~zero].view(np.int32).astype(np.int64) - want[~zero].view(np.int32))
        worst = int(ulps.max()) if ulps.size else 0
        print("nonlin-prepare %-56s stats_kernels.hip worst %d units in the last place of %d samples" % (N.case_id(c), worst, want.size))
        if not c.limiter:
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), what
        else:
            assert worst <= 4, (what, worst)


# ---- the other entries: the single-stream call's rows bit for bit ------------------------------------------------------
FORMS_CASE = N.nl(1024, 0.5, "hanning", N.BOTH_S, "synth", "s16", sub_mean=1, frames=40)


def _streams(oracle, count, c=FORMS_CASE):
    """Whole hops only: an even count of samples, which a batch of integer streams needs between its streams."""
    whole = c.frames * K.X.hop_len(c.n, c.ovl)
    return [K.make_input(oracle, c, seed=100 + b)[0][:whole] for b in range(count)]


def test_batch_ragged_and_channels_are_the_single_stream_rows(lib, oracle, torch_cuda):
    """run_batch, run_ragged and run_channels on 16-bit samples with the limiter, RA9MB and the reference-order mean at N = 1024:
    every stream's rows are run()'s, bit for bit; stream 0's are judged bin by bin."""
    torch, c = torch_cuda, FORMS_CASE
    raws = _streams(oracle, 4)
    sp = _plan(lib, oracle, c)
    singles = [sp.run(torch.from_numpy(x).cuda()).cpu().numpy() for x in raws]
    xf = oracle.pcm_s16_to_float(raws[0])
    exact, f32, want = N.rows_of(oracle, c, xf)
    assert N.limiter_condition(c, xf)
    t32 = tau_of(f32, exact)
    r = K.Ref(raws[0], xf, exact, f32, want, t32, bound(t32), tau_of(want, exact), K.peak_err(want, exact))
    _judge("g", c, "run", singles[0], r)
    batch = sp.run_batch(torch.from_numpy(np.stack(raws)).cuda()).cpu().numpy()
    for b in range(len(raws)):
        assert np.array_equal(batch[b].view(np.uint32), singles[b].view(np.uint32)), ("batch", b)
    # ragged: streams of 40, 17, 1 and 29 hops at even offsets of one buffer, gaps between them
    hops = [40, 17, 1, 29]
    h = sp.hop
    buf = np.full(sum(hops) * h + 64, 77, np.int16)
    offs, lens, at = [], [], 6
    for x, k in zip(raws, hops):
        buf[at:at + k * h] = x[:k * h]
        offs.append(at)
        lens.append(k * h)
        at += k * h + 10
    rows, starts = sp.run_ragged(torch.from_numpy(buf).cuda(), offs, lens)
    rows = rows.cpu().numpy()
    assert list(np.diff(starts)) == hops
    for b, k in enumerate(hops):
        assert np.array_equal(rows[starts[b]:starts[b + 1]].view(np.uint32), singles[b][:k].view(np.uint32)), ("ragged", b)
    # channels: the four streams interleaved, selected out of order and one twice
    inter = np.ascontiguousarray(np.stack(raws, axis=1))
    select = [2, 0, 3, 0, 1]
    chan = sp.run_channels(torch.from_numpy(inter).cuda(), select=select).cpu().numpy()
    for j, b in enumerate(select):
        assert np.array_equal(chan[j].view(np.uint32), singles[b].view(np.uint32)), ("channels", j, b)
    sp.close()


def test_host_entry_over_several_chunks(lib, oracle, torch_cuda, monkeypatch):
    """run_host under the same plan, its ring cut into chunks of 64 frames: run()'s rows bit for bit across the chunk seams (the
    halo carries the previous hops AFTER their mean removal into the next chunk's limiter)."""
    c = FORMS_CASE._replace(frames=300)
    raw = _streams(oracle, 1, c)[0]
    sp = _plan(lib, oracle, c)
    want = sp.run(torch_cuda.from_numpy(raw).cuda()).cpu().numpy()
    monkeypatch.setenv("GLFER_INGEST_CHUNK", "64")
    got = sp.run_host(raw)
    assert got.shape == want.shape == (300, 513)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    sp.close()
