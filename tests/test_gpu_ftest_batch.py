"""The harmonic F-test of many streams per call (-m gpu): glfer_hip_mtm_ftest_batch_device / Spectrogram.ftest_batch against
a loop of the single-stream entry (Spectrogram.ftest) over the same streams, on the same plan.

The Nyquist column of an F row is x/0 by the reference's own quirk -- an infinity, or NaN with mu dead -- so every equality
here compares BIT PATTERNS (.view(torch.int32)), never floats.  The streams of a batch differ in seed, amplitude and DC level,
so that a row taken from the wrong stream, history read across a stream boundary or a mean taken from the wrong stream's hops
cannot come out equal by accident.  The batch's output sits inside a larger buffer pre-filled with a sentinel: every value of
the range must be written and no float outside it.

GLFER_FTEST_PAIRED is read on every call, so the in-launch form is chosen per test as tests/test_gpu_ftest.py does: 'single'
= 0 (one sequence per transform), 'paired' = 1 (two, separated through the mirror bins), 'default' = unset (paired from 2048).
"""
import ctypes as C

import numpy as np
import pytest

import _ftest_batch_cases as B
import _ftest_cases as K
from _ftest_check import TOL, check_ftest
from _signals import synth

pytestmark = pytest.mark.gpu
E_ARG = -1                                # GLFER_E_ARG (include/glfer_hip.h)
SENTINEL = 0x5A5A5A5A                     # (3.76e16 as a float: no F row holds it)
PAD = 96                                  # guard floats either side of the output
FORMS = ("default", "single", "paired")
BOTH = ("single", "paired")


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


_PLANS = {}


def _plan(lib, n, ovl, nw, kmax, **kw):
    """One plan per configuration for the whole module (the tapers are made once; the form is read per call)."""
    key = (n, ovl, nw, kmax, tuple(sorted(kw.items())))
    if key not in _PLANS:
        _PLANS[key] = lib.Spectrogram(lib.MtmParams(n=n, overlap=ovl, w=nw, kmax=kmax, **kw))
    return _PLANS[key]


def _streams(torch, lib, fmt, nb, nsamples, pitch=None, gap=None, dc_rms=False):
    """[nb, nsamples] view of a [nb, pitch] buffer of the plan's sample type; the pitch - nsamples samples after each stream
    hold `gap`.  dc_rms: DC levels of the size of the signal's rms (0.4 for synth at amplitude 1), of either sign."""
    pitch = pitch or nsamples
    if fmt != lib.SAMPLES_F32:
        pitch += pitch & 1                             # integer samples: an even stream pitch (glfer_hip.h)
    out = np.zeros((nb, pitch), np.float64)
    for b in range(nb):
        amp = 0.4 + 0.6 * ((b * 7919) % 11) / 10.0
        dc = 0.05 * (((b * 104729) % 9) - 4)
        if dc_rms:
            dc = (0.4, -0.4, 0.3, -0.25)[b % 4] * amp
        out[b, :nsamples] = amp * synth(nsamples, seed=1000 + b) + dc
    if fmt == lib.SAMPLES_F32:
        buf = out.astype(np.float32)
    elif fmt == lib.SAMPLES_S16:
        buf = np.clip(np.round(out * 20000.0), -32768, 32767).astype(np.int16)
    else:
        buf = np.clip(np.round(128.0 + out * 90.0), 0, 255).astype(np.uint8)
    if gap is not None and pitch > nsamples:
        buf[:, nsamples:] = gap
    return torch.from_numpy(buf).to("cuda:0")[:, :nsamples]


def _check(torch, sp, x, first=0, nframes=None, mu_live=True):
    """The batched call into a guarded buffer against the loop of single-stream calls: bit patterns, guards, and (mu live)
    finite values below Nyquist.  Returns the batch's rows [B][nframes][bins]."""
    nb, half = x.size(0), sp.n // 2
    nframes = sp.num_frames(x.size(1)) - first if nframes is None else nframes
    assert nframes > 0
    count = nb * nframes * sp.bins
    buf = torch.full((PAD + count + PAD,), SENTINEL, dtype=torch.int32, device="cuda:0")
    out = buf[PAD:PAD + count].view(torch.float32).view(nb, nframes, sp.bins)
    got = sp.ftest_batch(x, first_frame=first, nframes=nframes, mu_live=mu_live, out=out)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr() and got.shape == (nb, nframes, sp.bins)
    want = torch.stack([sp.ftest(x[b], first_frame=first, nframes=nframes, mu_live=mu_live) for b in range(nb)])
    torch.cuda.synchronize()
    gb, wb = buf[PAD:PAD + count].view(nb, nframes, sp.bins), want.view(torch.int32)
    assert not bool((gb == SENTINEL).any()), "a value of the range was not written"
    bad = [b for b in range(nb) if not torch.equal(gb[b], wb[b])]
    assert not bad, ("streams whose rows differ from the single entry's", bad[:8])
    assert bool((buf[:PAD] == SENTINEL).all()) and bool((buf[PAD + count:] == SENTINEL).all()), "the entry wrote outside its rows"
    if mu_live:
        assert bool(torch.isfinite(got[:, :, :half]).all())
        assert not bool(torch.isfinite(got[:, :, half]).any())
        for a in range(nb - 1):                        # the streams do differ: the next stream's rows would not pass for this one's
            assert not torch.equal(gb[a], gb[a + 1]), a
    return got


def _nsamples(sp, frames):
    return frames * sp.hop + sp.hop // 3


# ---- batch equals loop: every in-launch size class, both forms, the stream-by-stream route ------------------------------
# (n, overlap, nw, kmax, frames)
SHAPES = {
    "n256": (256, 0.75, 2.0, 2, 39),                  # the smallest in-launch size
    "n1024": (1024, 0.5, 4.0, 7, 13),
    "n2048_k3": (2048, 0.5, 2.5, 3, 9),               # the smallest default-paired size: five sequences with mu (odd) ...
    "n2048_k4": (2048, 0.0, 2.5, 4, 9),               # ... and six (even)
    "n4096": (4096, 0.0, 2.5, 4, 7),                  # 5 tapers
    "n16384": (16384, 0.0, 4.5, 8, 5),
}


@pytest.mark.parametrize("nb", [3, 37])
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_batch_equals_loop(torch_cuda, lib, monkeypatch, shape, form, nb):
    _select(monkeypatch, form)
    n, ovl, nw, kmax, frames = SHAPES[shape]
    sp = _plan(lib, n, ovl, nw, kmax)
    _check(torch_cuda, sp, _streams(torch_cuda, lib, lib.SAMPLES_F32, nb, _nsamples(sp, frames)))


@pytest.mark.parametrize("nb", [3, 37])
def test_stream_by_stream_below_256(torch_cuda, lib, monkeypatch, nb):
    """N = 64: the spectra go through memory and the per-bin epilogue, one stream after the other inside the call."""
    _select(monkeypatch, "default")
    sp = _plan(lib, 64, 0.5, 2.5, 3)
    _check(torch_cuda, sp, _streams(torch_cuda, lib, lib.SAMPLES_F32, nb, _nsamples(sp, 29)))


@pytest.mark.parametrize("nb", [3, 37])
@pytest.mark.parametrize("shape", ["n256", "n2048"])
def test_more_work_than_the_shared_grid(torch_cuda, lib, monkeypatch, shape, nb):
    """The persistent grid of a launch is shared among its streams (glfer_batch_cap): 4 x 768 workgroups of 16 frames at
    N = 256, 4 x 512 of 2 frames at N = 2048, divided by the stream count.  With 37 streams that is 84 and 56 workgroups per
    stream, with 3 streams 1024 and 683 (cut to a multiple of 8: the XCD order): every stream has more frames than one pass
    of its share holds, and a last workgroup partly filled."""
    _select(monkeypatch, "default")
    n, ovl, nw, kmax = {"n256": (256, 0.75, 2.5, 4), "n2048": (2048, 0.75, 2.5, 3)}[shape]
    share = -(-(4 * (768 if n == 256 else 512)) // nb) * (16 if n == 256 else 2)      # frames in one pass of a stream's share
    frames = share + share // 3 + 5
    sp = _plan(lib, n, ovl, nw, kmax)
    _check(torch_cuda, sp, _streams(torch_cuda, lib, lib.SAMPLES_F32, nb, _nsamples(sp, frames)))


# ---- mu never written ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", BOTH)
@pytest.mark.parametrize("shape", ["n256", "n2048_k3", "n2048_k4"])
def test_dead_mu(torch_cuda, lib, monkeypatch, shape, form):
    """mu_live = False (the reference build without FFTW): +0.0 below Nyquist and 0/0 at Nyquist, the loop's bits."""
    torch = torch_cuda
    _select(monkeypatch, form)
    n, ovl, nw, kmax, frames = SHAPES[shape]
    sp = _plan(lib, n, ovl, nw, kmax)
    got = _check(torch, sp, _streams(torch, lib, lib.SAMPLES_F32, 5, _nsamples(sp, frames)), mu_live=False)
    assert bool((got[:, :, :n // 2].contiguous().view(torch.int32) == 0).all())
    assert bool(torch.isnan(got[:, :, n // 2]).all())


# ---- 16-bit and 8-bit samples --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", BOTH)
@pytest.mark.parametrize("fmt", [1, 2])
@pytest.mark.parametrize("shape", ["n256", "n2048_k3", "n4096"])
def test_integer_sample_formats(torch_cuda, lib, monkeypatch, shape, fmt, form):
    _select(monkeypatch, form)
    n, ovl, nw, kmax, frames = SHAPES[shape]
    sp = _plan(lib, n, ovl, nw, kmax, sample_format=fmt)
    x = _streams(torch_cuda, lib, fmt, 5, _nsamples(sp, frames))
    assert x.stride(0) % 2 == 0
    _check(torch_cuda, sp, x)


# ---- mean removal: the batch's corrected copies ----------------------------------------------------------------------------
# hops of 4 and 16 sixteenths of the block, and overlap 0.9 (a hop that is no sixteenth multiple)
MEAN_SHAPES = {"n256": (256, 0.75, 2.0, 3, 29), "n2048": (2048, 0.0, 2.5, 4, 9), "n4096": (4096, 0.9, 2.5, 4, 15)}


@pytest.mark.parametrize("form", BOTH)
@pytest.mark.parametrize("dc_rms", [False, True], ids=["dc_small", "dc_rms"])
@pytest.mark.parametrize("sub_mean", [1, 2])
@pytest.mark.parametrize("shape", sorted(MEAN_SHAPES))
def test_mean_removal(torch_cuda, lib, monkeypatch, shape, sub_mean, dc_rms, form):
    _select(monkeypatch, form)
    n, ovl, nw, kmax, frames = MEAN_SHAPES[shape]
    sp = _plan(lib, n, ovl, nw, kmax, sub_mean=sub_mean)
    _check(torch_cuda, sp, _streams(torch_cuda, lib, lib.SAMPLES_F32, 5, _nsamples(sp, frames), dc_rms=dc_rms))


def test_mean_removal_integer_samples(torch_cuda, lib, monkeypatch):
    _select(monkeypatch, "default")
    sp = _plan(lib, 2048, 0.75, 2.5, 4, sub_mean=1, sample_format=1)
    _check(torch_cuda, sp, _streams(torch_cuda, lib, 1, 5, _nsamples(sp, 13), dc_rms=True))


# ---- history zeroed in every frame -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", BOTH)
@pytest.mark.parametrize("sub_mean", [0, 1])
@pytest.mark.parametrize("n", [1024, 4096])
def test_history_zeroed_in_every_frame(torch_cuda, lib, monkeypatch, n, sub_mean, form):
    _select(monkeypatch, form)
    sp = _plan(lib, n, 0.75, 2.5, 4, history_mode=lib.HISTORY_ZERO_ALWAYS, sub_mean=sub_mean)
    _check(torch_cuda, sp, _streams(torch_cuda, lib, lib.SAMPLES_F32, 5, _nsamples(sp, 15)))


# ---- a frame range inside the stream ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", BOTH)
@pytest.mark.parametrize("sub_mean", [0, 1])
@pytest.mark.parametrize("n,ovl", [(1024, 0.5), (4096, 0.75)])
def test_frame_range_inside_the_stream(torch_cuda, lib, monkeypatch, n, ovl, sub_mean, form):
    """first_frame = 5 and the launch ending 4 frames before the streams do."""
    _select(monkeypatch, form)
    sp = _plan(lib, n, ovl, 2.5, 4, sub_mean=sub_mean)
    frames = 24
    _check(torch_cuda, sp, _streams(torch_cuda, lib, lib.SAMPLES_F32, 7, _nsamples(sp, frames)), first=5, nframes=frames - 9)


# ---- what lies between the streams -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", [0, 1, 2])
@pytest.mark.parametrize("shape,sub_mean", [("n256", 0), ("n256", 1), ("n2048_k3", 0), ("n2048_k3", 2), ("n4096", 0), ("n4096", 1)])
def test_gap_between_streams(torch_cuda, lib, monkeypatch, shape, sub_mean, fmt):
    """The samples between streams are NaN (f32) or full scale (integers): history read from the previous stream or a read
    past a stream's end shows as a non-finite or unequal row."""
    _select(monkeypatch, "default")
    n, ovl, nw, kmax, frames = SHAPES[shape]
    sp = _plan(lib, n, ovl, nw, kmax, sub_mean=sub_mean, sample_format=fmt)
    nsamples = frames * sp.hop
    gap = {0: np.float32(np.nan), 1: np.int16(32767), 2: np.uint8(255)}[fmt]
    x = _streams(torch_cuda, lib, fmt, 5, nsamples, pitch=nsamples + 2 * n + 6, gap=gap)
    assert x.stride(0) >= nsamples + 2 * n + 6
    _check(torch_cuda, sp, x)


# ---- a pitched plan ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", BOTH)
def test_f_rows_stay_dense_on_a_pitched_plan(torch_cuda, lib, monkeypatch, form):
    """cfg.psd_pitch = 2112 at N = 4096: the PSD rows are 2112 floats apart, the F rows N/2 + 1, stream after stream."""
    _select(monkeypatch, form)
    sp = _plan(lib, 4096, 0.0, 2.5, 4, psd_pitch=2112)
    assert sp.pitch == 2112 and sp.bins == 2049
    x = _streams(torch_cuda, lib, lib.SAMPLES_F32, 5, _nsamples(sp, 7))
    got = _check(torch_cuda, sp, x)
    dense = _plan(lib, 4096, 0.0, 2.5, 4).ftest_batch(x)
    assert torch_cuda.equal(got.view(torch_cuda.int32), dense.view(torch_cuda.int32))


# ---- more streams than the grid's y dimension holds ------------------------------------------------------------------------
def test_large_batch_crosses_grid_y_limit(torch_cuda, lib, monkeypatch):
    """70 000 one-frame streams: more than one chunk of the grid's y limit (65 535)."""
    torch = torch_cuda
    _select(monkeypatch, "default")
    sp = _plan(lib, 256, 0.0, 2.0, 2)
    nb, hop, half = 70000, sp.hop, 128
    x = (torch.rand((nb, hop), generator=torch.Generator().manual_seed(5), dtype=torch.float32) - 0.5)
    x = (x * torch.linspace(0.4, 1.0, nb)[:, None] + torch.linspace(-0.3, 0.3, nb)[:, None]).to("cuda:0")
    got = sp.ftest_batch(x)
    torch.cuda.synchronize()
    assert got.shape == (nb, 1, sp.bins)
    assert bool(torch.isfinite(got[:, :, :half]).all()) and not bool(torch.isfinite(got[:, :, half]).any())
    probe = sorted(set([0, 1, 65534, 65535, 65536, 65537, nb - 2, nb - 1] + [int(v) for v in np.random.default_rng(3).integers(0, nb, 64)]))
    for b in probe:
        want = sp.ftest(x[b])
        torch.cuda.synchronize()
        assert torch.equal(got[b].view(torch.int32), want.view(torch.int32)), b


# ---- a stream beyond 4 GiB of the buffer -----------------------------------------------------------------------------------
def test_stream_past_4gib(torch_cuda, lib, monkeypatch):
    """The second stream of the batch starts beyond 4 GiB of the buffer: first, middle and last frame of both streams."""
    torch = torch_cuda
    _select(monkeypatch, "default")
    sp = _plan(lib, 2048, 0.0, 2.5, 4)
    nsamples = 64 * sp.hop
    pitch = (1 << 30) + 4096                           # floats: stream 1 at 4 GiB + 16 KiB
    buf = torch.empty(pitch + nsamples, dtype=torch.float32, device="cuda:0")
    buf[:nsamples] = torch.from_numpy(synth(nsamples, seed=21)).to("cuda:0")
    buf[pitch:] = torch.from_numpy(0.7 * synth(nsamples, seed=22) + 0.1).to("cuda:0")
    x = buf.as_strided((2, nsamples), (pitch, 1))
    got = sp.ftest_batch(x)
    want = [sp.ftest(buf[:nsamples]), sp.ftest(buf[pitch:])]
    torch.cuda.synchronize()
    nf = sp.num_frames(nsamples)
    assert nf == 64 and got.shape == (2, nf, sp.bins)
    for f in (0, nf // 2, nf - 1):
        for b in (0, 1):
            assert torch.equal(got[b, f].view(torch.int32), want[b][f].view(torch.int32)), (b, f)
            assert bool(torch.isfinite(got[b, f, :1024]).all())
    assert not torch.equal(got[0, 0].view(torch.int32), got[1, 0].view(torch.int32))
    del buf, x, got, want
    torch.cuda.empty_cache()


# ---- refusals and empty calls ------------------------------------------------------------------------------------------------
def _call_into(torch, lib, sp, x, nb, pitch, nsamples, first, nframes, rows):
    """The C entry with `rows` rows of sentinel as its output: (rc, output untouched)."""
    buf = torch.full((max(rows, 1) * sp.bins,), SENTINEL, dtype=torch.int32, device="cuda:0")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = lib.api.lib().glfer_hip_mtm_ftest_batch_device(sp._h, C.c_void_p(x.data_ptr()), nb, pitch, nsamples, first, nframes,
                                                        C.c_void_p(buf.data_ptr()), 1, st)
    torch.cuda.synchronize()
    return rc, bool((buf == SENTINEL).all())


def test_refusals_and_empty_calls(torch_cuda, lib, monkeypatch):
    torch = torch_cuda
    _select(monkeypatch, "default")
    L = lib.api.lib()
    n, frames = 1024, 8
    s16 = _plan(lib, n, 0.0, 2.5, 4, sample_format=1)
    x = torch.zeros((4, 2 * frames * n), dtype=torch.int16, device="cuda:0")
    pitch, nsamples = 2 * frames * n, frames * n
    assert _call_into(torch, lib, s16, x, 3, pitch - 1, nsamples, 0, 4, 12) == (E_ARG, True)         # odd pitch with s16 samples
    assert _call_into(torch, lib, s16, x, 3, pitch, nsamples, 0, frames + 1, 27) == (E_ARG, True)    # a frame past the stream
    assert _call_into(torch, lib, s16, x, 3, pitch, nsamples, frames, 1, 3) == (E_ARG, True)
    assert _call_into(torch, lib, s16, x, 0, pitch, nsamples, 0, 4, 12) == (0, True)                 # empty calls: nothing launched
    assert _call_into(torch, lib, s16, x, 3, pitch, nsamples, 0, 0, 12) == (0, True)
    assert _call_into(torch, lib, s16, x, 3, pitch, nsamples, frames + 5, 0, 12) == (0, True)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    out = torch.zeros(3 * 4 * s16.bins, device="cuda:0")
    assert L.glfer_hip_mtm_ftest_batch_device(s16._h, None, 3, pitch, nsamples, 0, 4, C.c_void_p(out.data_ptr()), 1, st) == E_ARG
    assert L.glfer_hip_mtm_ftest_batch_device(s16._h, C.c_void_p(x.data_ptr()), 3, pitch, nsamples, 0, 4, None, 1, st) == E_ARG
    assert L.glfer_hip_mtm_ftest_batch_device(s16._h, C.c_void_p(x.data_ptr()), 3, pitch, nsamples, 0, 1 << 31, C.c_void_p(out.data_ptr()),
                                              1, st) == E_ARG
    assert _call_into(torch, lib, s16, x, 3, pitch, nsamples, 0, 4, 12) == (0, False)                 # the same call, well formed: rows written
    # a plan that is not MTM, and an MTM plan above the entry's range
    per = lib.Spectrogram(lib.FftParams(n=1024, window_type=0, overlap=0.0))
    xf = torch.zeros((3, 4 * 1024), device="cuda:0")
    assert _call_into(torch, lib, per, xf, 3, 4 * 1024, 4 * 1024, 0, 4, 12) == (E_ARG, True)
    big = lib.Spectrogram(lib.MtmParams(n=32768, overlap=0.0, w=2.0, kmax=2))
    xb = torch.zeros((3, 2 * 32768), device="cuda:0")
    assert _call_into(torch, lib, big, xb, 3, 2 * 32768, 2 * 32768, 0, 2, 6) == (E_ARG, True)
    with pytest.raises(lib.GlferHipError, match="bad argument"):
        big.ftest_batch(xb)


# ---- what the call leaves of the plan --------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", BOTH)
@pytest.mark.parametrize("n,sub_mean", [(512, 1), (2048, 0), (4096, 0)])
def test_plan_after_the_call(torch_cuda, lib, monkeypatch, n, sub_mean, form):
    """The single entry and run() give, after a batched call on the plan, the bits they gave before it; and a plan whose first
    F call is the batched one (it makes the tables) gives the bits of a plan whose first was the single entry."""
    torch = torch_cuda
    _select(monkeypatch, form)
    mk = lambda: lib.Spectrogram(lib.MtmParams(n=n, overlap=0.5, w=2.5, kmax=4, sub_mean=sub_mean))
    sp = mk()
    x = _streams(torch, lib, lib.SAMPLES_F32, 4, _nsamples(sp, 11))
    bits = lambda t: t.contiguous().view(torch.int32)
    f_before = [sp.ftest(x[b]) for b in range(4)]
    r_before = sp.run(x[1])
    d_before = sp.ftest(x[2], mu_live=False)
    got = _check(torch, sp, x)
    _check(torch, sp, x, mu_live=False)
    for b in range(4):
        assert torch.equal(bits(sp.ftest(x[b])), bits(f_before[b])) and torch.equal(bits(got[b]), bits(f_before[b])), b
    assert torch.equal(bits(sp.run(x[1])), bits(r_before))
    assert torch.equal(bits(sp.ftest(x[2], mu_live=False)), bits(d_before))
    other = mk()                                         # no F call yet: the batched entry makes the tables
    assert torch.equal(bits(other.ftest_batch(x)), bits(got))
    assert torch.equal(bits(other.ftest(x[3])), bits(f_before[3]))
    assert torch.equal(bits(other.run(x[1])), bits(r_before))
    assert torch.equal(bits(other.run_batch(x)[1]), bits(r_before))


# ---- oracle parity through the batch -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", B.PARITY_CASES, ids=K.case_id)
def test_batch_oracle_parity(torch_cuda, lib, oracle, monkeypatch, c):
    """One case per in-launch form (N = 1024: one sequence per transform; N = 4096: two), four streams; every stream by
    check_ftest against the oracle, the bound weighed by float64 num / den, at the rule's own TOL.
    tests/test_ftest_batch_host.py holds the reference alone to the same rule on each of these streams."""
    torch = torch_cuda
    _select(monkeypatch, "default")
    refs = [B.reference(oracle, c, b) for b in range(B.NSTREAMS)]
    x = torch.from_numpy(np.stack([r[0] for r in refs])).to("cuda:0")
    sp = _plan(lib, c.n, c.ovl, c.nw, c.kmax)
    got = sp.ftest_batch(x).cpu().numpy()
    for b, (_, want, num, den) in enumerate(refs):
        frac = check_ftest(got[b], want, num, den, c.kmax, tol=TOL)
        print("ftest-batch-parity %-44s stream %d device/oracle %.4f of the bound" % (K.case_id(c), b, frac))
        assert frac <= 1.0
