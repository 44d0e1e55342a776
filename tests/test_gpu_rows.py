"""GPU tests (-m gpu): periodogram and multitaper rows of Spectrogram.run, bin by bin in amplitude against float64.

Every parity test of the rows elsewhere in the suite is normalised by a row's LARGEST bin; on tonal input 1e-5 of that is
the size of a noise-floor bin, so such a bin may be wrong by tens of per cent.  Here every bin of every frame is held to

    | sqrt(got[k]) - sqrt(exact[k]) |  <=  tau * sqrt( sum_k exact[k] ),    tau = 4 * max(tau_f32, 2**-24)

(tests/_rows_check.py) with `exact` the float64 rows of tests/_exact.py and tau_f32 what a plain float32 computation of
the same frames reaches -- computed on the CPU per case, never from device output.  Beside it, per frame, the suite's
peak-normalised rule against the oracle stays asserted: 1e-5, and from N = 8192 round 4's max(1e-5, 1.1 x err(oracle, exact)).

The cases are tests/_rows_cases.py's; tests/test_rows_criterion.py runs the stand-in and the oracle over every one of them
without a GPU and shows that the rule rejects subtly wrong rows.  The forms are chosen per test through the environment the
launcher reads per launch: GLFER_FORM=h|w|x, GLFER_Y_TAPERS=full, GLFER_MEAN_PREPASS=1.

Which case reaches which kernel file (glfer_hip.cpp, launch_by_n):
  spectro_small.hip   every case below N = 256
  spectro16h.hip      the periodogram N = 512 ... 16384, its AVG form from frame b0 of the long test_plain_average cases; its
                      multitaper form: N = 8192, and N = 16384 under GLFER_FORM=h
  spectro16.hip       N = 256, even taper counts, first frames (zero history), integer samples off their pairs, spectrum=True,
                      GLFER_FORM=x on the periodogram and on the multitaper from N = 8192
  spectro16xl.hip     odd taper counts at N = 256 ... 2048 (the taper half tables fit the LDS for every count of the matrix
                      but the next line's)
  spectro16x.hip      23 and 25 tapers at N = 1024 (mtm-n1024-...-k22 / -k24)
  spectro16y.hip      odd taper counts at N = 4096: five tapers NW 2.5 the half-table form, GLFER_Y_TAPERS=full and 3 / 9 tapers the full
  spectro16w.hip      the multitaper at N = 16384, GLFER_FORM=w from N = 2048, spectrum=True at N = 32768
  spectro_big.hip     the periodogram from N = 32768, the two-level combine from N = 131072
Past one unit of work per workgroup, and spectro16h.hip's register-walk forms (SHIFT = 2 / 4 / 8: the periodogram at overlap 87.5 / 75 /
50 % without mean removal from work >= 4 x resident on -- no case here is that long): tests/test_gpu_walk.py, same rule;
group (f) below covers spectro_small, spectro16h's plain form at N = 2048, the packed kernel at N = 256 / 2048, spectro16xl at
N = 256 and spectro16y.
Not here: limiter / RA9MB (non-linear: tests/test_gpu_nonlin.py holds them to the same rule), HP-ARMA, LMP, the F-test (own
rules), the host / WAV / worker entries (the same kernels).

Lines starting with 'rows-bin-by-bin' (run with -s) are the record kept in profiles/rows_bin_by_bin.txt.
"""
import numpy as np
import pytest

import _rows_cases as K
from _rows_check import bound, check_rows, check_spectrum, from_halfcomplex, tau_of, tau_of_spectrum
from _rows_device import _plan, _select, _upload
from _signals import rel_err

pytestmark = pytest.mark.gpu
TOL = K.TOL


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _judge(group, c, form, got, r, rows=slice(None)):
    """Device rows against the float64 rows under (1) and against the oracle under the suite's rule; prints the record line."""
    exact, want = r.exact[rows], r.want[rows]
    got = np.asarray(got)
    assert got.shape == exact.shape, (got.shape, exact.shape)
    what = "%s %s %s" % (group, K.case_id(c), form)
    dev_tau = tau_of(got, exact)
    print("rows-bin-by-bin %-2s %-62s %-8s device tau %.3e bound %.3e fraction %.3f tau_f32 %.3e oracle tau %.3e" % (
        group, K.case_id(c), form, dev_tau, r.tau, dev_tau / r.tau, r.tau_f32, r.tau_oracle))
    frac = check_rows(got, exact, r.tau, what)
    for f in range(len(want)):
        if want[f].any():
            e_dev, e_ref = max(rel_err(got[f], want[f])), max(rel_err(want[f], exact[f]))
            assert e_dev <= K.oracle_bound(c, e_ref), (what, f, e_dev, e_ref)
        else:
            assert not got[f].any(), (what, f)                  # silence stays silence
    return frac


def _run(lib, oracle, torch, c, sub_mean=None, offset=0, **kw):
    r = K.reference(oracle, c)
    sp = _plan(lib, oracle, c, sub_mean)
    got = sp.run(_upload(torch, r.raw, offset), **kw).cpu().numpy()
    sp.close()
    return got, r


def _forms_of(c):
    """The forms glfer_hip.cpp's body_route really tells apart for the case's plan, beside the launcher's own choice:
    periodogram: spectro16h from N = 512 by default, x = the packed kernel, w = spectro16w from N = 2048;
    multitaper: below N = 8192 GLFER_FORM=h and x change nothing (no real-input tables; x leaves the shared-odd forms on),
    w = spectro16w from N = 2048; N = 8192: spectro16h by default, w, x = packed; N = 16384: spectro16w by default, h, x;
    GLFER_Y_TAPERS=full only where the plan has half tables (five tapers, NW = 2.5, N = 4096)."""
    if c.n < 512 or c.n > 16384:
        return ("default",)
    if c.est == "fft":
        return ("default", "x") + (("w",) if c.n >= 2048 else ())
    if c.n < 2048:
        return ("default",)
    if c.n == 8192:
        return ("default", "w", "x")
    if c.n == 16384:
        return ("default", "h", "x")
    return ("default", "w") + (("full",) if (c.n, c.kmax, c.nw) == (4096, 4, 2.5) else ())


def _with_forms(cases):
    return [pytest.param(c, form, id="%s-%s" % (K.case_id(c), form)) for c in cases for form in _forms_of(c)]


# ---- (a) the periodogram at every block size -------------------------------------------------------------------------
@pytest.mark.parametrize("c", K.FFT_SIZE_CASES, ids=K.case_id)
def test_periodogram_every_size(lib, oracle, torch_cuda, monkeypatch, c):
    _select(monkeypatch, "default")
    got, r = _run(lib, oracle, torch_cuda, c)
    _judge("a", c, "default", got, r)


# ---- (b) every window ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", K.FFT_WINDOW_CASES, ids=K.case_id)
def test_periodogram_every_window(lib, oracle, torch_cuda, monkeypatch, c):
    _select(monkeypatch, "default")
    got, r = _run(lib, oracle, torch_cuda, c)
    _judge("b", c, "default", got, r)


# ---- (c) the multitaper at every block size, in every form a size has ------------------------------------------------
@pytest.mark.parametrize("c,form", _with_forms(K.MTM_SIZE_CASES))
def test_multitaper_every_size_and_form(lib, oracle, torch_cuda, monkeypatch, c, form):
    _select(monkeypatch, form)
    got, r = _run(lib, oracle, torch_cuda, c)
    _judge("c", c, form, got, r)


# ---- (d) the periodogram's forms; tones on the edge bins ---------------------------------------------------------------
@pytest.mark.parametrize("c,form", _with_forms(K.FFT_FORM_CASES))
def test_periodogram_forms(lib, oracle, torch_cuda, monkeypatch, c, form):
    _select(monkeypatch, form)
    got, r = _run(lib, oracle, torch_cuda, c)
    _judge("d", c, form, got, r)


@pytest.mark.parametrize("c", K.EDGE_CASES, ids=K.case_id)
def test_tones_on_the_edge_bins(lib, oracle, torch_cuda, monkeypatch, c):
    """Bin 1, bin N/2 - 1 and Nyquist hold the row's power: DC and Nyquist come out of the real-input and paired forms'
    mirror-bin separation with the rounding of that power."""
    _select(monkeypatch, "default")
    got, r = _run(lib, oracle, torch_cuda, c)
    _judge("d", c, "default", got, r)
    if c.est == "fft":                                          # (five tapers spread a tone over 2 NW bins: no single strongest bin)
        half = c.n // 2
        k = {"bin_lo": 1, "bin_hi": half - 1, "alt": half}[c.signal]
        assert (np.argmax(r.exact, axis=1) == k).all() and (np.argmax(got, axis=1) == k).all()


# ---- (e) history, frame ranges ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", K.HISTORY_CASES, ids=K.case_id)
def test_history_zeroed_in_every_frame(lib, oracle, torch_cuda, monkeypatch, c):
    _select(monkeypatch, "default")
    assert c.history_mode == lib.HISTORY_ZERO_ALWAYS
    got, r = _run(lib, oracle, torch_cuda, c)
    _judge("e", c, "default", got, r)


@pytest.mark.parametrize("cf", K.RANGE_CASES, ids=lambda cf: "%s-first%d" % (K.case_id(cf[0]), cf[1]))
def test_frame_range_inside_the_stream(lib, oracle, torch_cuda, monkeypatch, cf):
    """A launch that starts and ends inside the stream and inside the kernels' frame groups; the whole stream too, whose
    first frames reach back before sample 0."""
    c, first = cf
    _select(monkeypatch, "default")
    nframes = c.frames - first - 3
    assert nframes > 0
    got, r = _run(lib, oracle, torch_cuda, c, first_frame=first, nframes=nframes)
    _judge("e", c, "first%d" % first, got, r, rows=slice(first, first + nframes))
    whole, _ = _run(lib, oracle, torch_cuda, c)
    _judge("e", c, "whole", whole, r)


# ---- (f) more frames than one pass of the grid -------------------------------------------------------------------------
@pytest.mark.parametrize("c", K.LONG_CASES, ids=K.case_id)
def test_long_streams_every_frame(lib, oracle, torch_cuda, monkeypatch, c):
    _select(monkeypatch, "default")
    got, r = _run(lib, oracle, torch_cuda, c)
    _judge("f", c, "default", got, r)


def test_long_stream_of_the_interleaved_form(lib, oracle, torch_cuda, monkeypatch):
    """spectro16y.hip takes 16 384 frames a pass: 20 481 frames (hop = frame, so a frame's row is the row of its own N
    samples as a stream), the head, the seam of the passes and the ragged end checked bin by bin."""
    _select(monkeypatch, "default")
    c = K.LONG_Y
    raw, xf = K.make_input(oracle, c)
    sp = _plan(lib, oracle, c)
    got = sp.run(_upload(torch_cuda, raw))
    assert got.shape[0] == c.frames and bool(torch_cuda.isfinite(got).all())
    for a, b in K.LONG_Y_CUTS:
        cut = c._replace(frames=b - a)
        sub = xf[a * c.n:b * c.n]
        exact, f32, want = K.rows_of(oracle, cut, sub)
        t32 = tau_of(f32, exact)
        r = K.Ref(sub, sub, exact, f32, want, t32, bound(t32), tau_of(want, exact), K.peak_err(want, exact))
        _judge("f", cut, "cut%d" % a, got[a:b].cpu().numpy(), r)
    sp.close()


# ---- (g) 16-bit and 8-bit samples, dither, silence ---------------------------------------------------------------------
@pytest.mark.parametrize("c", K.FORMAT_CASES, ids=K.case_id)
def test_integer_sample_formats(lib, oracle, torch_cuda, monkeypatch, c):
    _select(monkeypatch, "default")
    off = K.FORMAT_OFFSETS.get(K.case_id(c), 0)
    got, r = _run(lib, oracle, torch_cuda, c, offset=off)
    assert r.raw.dtype == (np.int16 if c.fmt == "s16" else np.uint8)
    _judge("g", c, "offset%d" % off, got, r)


@pytest.mark.parametrize("c", K.LSB_CASES, ids=K.case_id)
def test_dither_and_silence(lib, oracle, torch_cuda, monkeypatch, c):
    _select(monkeypatch, "default")
    got, r = _run(lib, oracle, torch_cuda, c, offset=1 if c.fmt != "f32" and c.n == 4096 else 0)
    _judge("g", c, "default", got, r)
    if c.signal == "zero":
        assert not r.exact.any() and not got.any()


# ---- (h) mean removal --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["default", "prepass"])
@pytest.mark.parametrize("c", K.MEAN_CASES, ids=K.case_id)
def test_mean_removal_in_the_references_order(lib, oracle, torch_cuda, monkeypatch, c, form):
    """sub_mean = 1: the hop means handed to the kernels as a table, and through the corrected copy."""
    _select(monkeypatch, form)
    got, r = _run(lib, oracle, torch_cuda, c, sub_mean=lib.SUBMEAN_EXACT)
    _judge("h", c, "m1-" + form, got, r)


@pytest.mark.parametrize("c", K.MEAN2_CASES, ids=K.case_id)
def test_mean_removal_with_the_in_kernel_sums(lib, oracle, torch_cuda, monkeypatch, c):
    """sub_mean = 2 where include/glfer_hip.h gives it the reference's rows: hop means small against the rms."""
    _select(monkeypatch, "default")
    assert K.mean2_condition(c, K.reference(oracle, c).xf)
    got, r = _run(lib, oracle, torch_cuda, c, sub_mean=lib.SUBMEAN_FAST)
    _judge("h", c, "m2", got, r)


# ---- (i) rows on a pitch, batches, spectra, the moving average ---------------------------------------------------------
@pytest.mark.parametrize("cp", K.PITCH_CASES, ids=lambda cp: "%s-pitch%d" % (K.case_id(cp[0]), cp[1]))
def test_rows_on_a_pitch(lib, oracle, torch_cuda, monkeypatch, cp):
    c, pitch = cp
    _select(monkeypatch, "default")
    r = K.reference(oracle, c)
    dx = _upload(torch_cuda, r.raw)
    sp = _plan(lib, oracle, c, psd_pitch=pitch)
    bins = c.n // 2 + 1
    assert sp.pitch == pitch and sp.bins == bins
    got = sp.run(dx).cpu().numpy()
    assert got.shape == (c.frames, pitch)
    _judge("i", c, "pitch%d" % pitch, got[:, :bins], r)
    dense = _plan(lib, oracle, c).run(dx).cpu().numpy()
    assert np.array_equal(dense.view(np.uint32), got[:, :bins].view(np.uint32))


@pytest.mark.parametrize("c", K.BATCH_CASES, ids=K.case_id)
def test_batch_of_streams(lib, oracle, torch_cuda, monkeypatch, c):
    """Five streams of different kinds in one call: stream 0, the middle one and the last bin by bin."""
    _select(monkeypatch, "default")
    members = [c._replace(signal=s) for s in K.BATCH_SIGNALS]
    raws = [K.make_input(oracle, m)[0] for m in members]
    d = torch_cuda.from_numpy(np.stack(raws)).cuda()
    sp = _plan(lib, oracle, c)
    got = sp.run_batch(d).cpu().numpy()
    assert got.shape == (len(members), c.frames, c.n // 2 + 1)
    for b in (0, len(members) // 2, len(members) - 1):
        _judge("i", members[b], "batch%d" % b, got[b], K.reference(oracle, members[b]))
    sp.close()


@pytest.mark.parametrize("c", K.SPECTRUM_CASES, ids=K.case_id)
def test_halfcomplex_spectra(lib, oracle, torch_cuda, monkeypatch, c):
    """run(spectrum=True): |got_X[k] - exact_X[k]| / sqrt(N) <= tau sqrt(sum_k P_k), the same units as (1), so a phase error
    counts; and the rows of that (packed) launch under (1)."""
    _select(monkeypatch, "default")
    raw, xf, exact_X, t32, tau = K.spectrum_reference(oracle, c)
    sp = _plan(lib, oracle, c)
    psd, spec = sp.run(_upload(torch_cuda, raw), spectrum=True)
    got_X = from_halfcomplex(spec.cpu().numpy())
    dev = tau_of_spectrum(got_X, exact_X, c.n)
    want_X = from_halfcomplex(np.stack([oracle.rfft_halfcomplex(row) for row in
                                        (K.X.frames64(xf, c.n, c.ovl).astype(np.float32) * K.window(oracle, c.n, c.window))]))
    print("rows-bin-by-bin %-2s %-62s %-8s device tau %.3e bound %.3e fraction %.3f tau_f32 %.3e oracle tau %.3e" % (
        "i", K.case_id(c), "spectrum", dev, tau, dev / tau, t32, tau_of_spectrum(want_X, exact_X, c.n)))
    check_spectrum(got_X, exact_X, c.n, tau, K.case_id(c))
    _judge("i", c, "spec-psd", psd.cpu().numpy(), K.reference(oracle, c))
    sp.close()


@pytest.mark.parametrize("c", K.AVG_CASES, ids=K.case_id)
def test_plain_average_inside_the_launch(lib, oracle, torch_cuda, monkeypatch, c):
    """run_avg PLAIN depth 4 against update_avg_plain's window mean of the float64 rows: a weighted sum of rows, so (1) holds
    for it with the rows' own tau (Cauchy-Schwarz over the rows of the window).  Where the call qualifies
    (K.avg_in_launch_from) the frames from b0 on are averaged in registers inside spectro16h.hip's launch and the head frames
    by the two launches: head, body and the seam at b0 are judged, the record lines say which is which.  GLFER_AVG_FUSED=0
    is a static of the library, read once per process, so it cannot be switched per test: its path (update_avg over run's
    rows) is judged beside it as 'avg-staged', and the in-launch doubles must be that path's doubles."""
    _select(monkeypatch, "default")
    r = K.reference(oracle, c)
    exact_avg = K.plain_average(r.exact, K.AVG_DEPTH)
    dx = _upload(torch_cuda, r.raw)
    sp = _plan(lib, oracle, c)
    bins = sp.bins
    avg, ret, psd = sp.run_avg(dx, lib.AVG_PLAIN, K.AVG_DEPTH, 0, bins, want_psd=True)
    quiet, _, _ = sp.run_avg(dx, lib.AVG_PLAIN, K.AVG_DEPTH, 0, bins, want_psd=False, want_ret=False)    # (no row leaves the launch)
    staged, _ = lib.update_avg(lib.AVG_PLAIN, sp.run(dx), K.AVG_DEPTH, 0, bins)
    _judge("i", c, "avg-psd", psd.cpu().numpy(), r)
    avg, quiet, staged = avg.cpu().numpy(), quiet.cpu().numpy(), staged.cpu().numpy()
    assert avg.dtype == np.float64 and avg.shape == exact_avg.shape
    b0 = K.avg_in_launch_from(c)
    parts = [("avg-2launch", slice(0, c.frames))] if b0 is None else [("avg-head", slice(0, b0)), ("avg-seam", slice(b0 - 1, b0 + 2)),
                                                                        ("avg-inlaunch", slice(b0, c.frames))]
    f32_avg, want_avg = K.plain_average(r.f32, K.AVG_DEPTH), K.plain_average(r.want, K.AVG_DEPTH)
    for name, rows in [(nm, avg[sl]) for nm, sl in parts] + [("avg-norows", quiet), ("avg-staged", staged)]:
        sl = dict(parts).get(name, slice(0, c.frames))
        dev = tau_of(rows, exact_avg[sl])
        print("rows-bin-by-bin %-2s %-62s %-12s device tau %.3e bound %.3e fraction %.3f tau_f32 %.3e oracle tau %.3e" % (
            "i", K.case_id(c), name, dev, r.tau, dev / r.tau, tau_of(f32_avg[sl], exact_avg[sl]), tau_of(want_avg[sl], exact_avg[sl])))
        check_rows(rows, exact_avg[sl], r.tau, "%s %s" % (K.case_id(c), name))
    assert np.array_equal(avg, staged) and np.array_equal(quiet, staged)
    sp.close()
