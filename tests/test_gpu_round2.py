"""GPU parity tests (-m gpu) for the rows added in round 2, all through the C-ABI:
LMP estimator, MTM harmonic F-test, prepare_audio frames, the WAV trailing partial block, sharding
with per-hop mean removal, the multi-GPU host entry, the chunk ring and the waterfall entry.

Tolerances.  Bit-exact where the device executes the reference's own float/double statements on
identical inputs (the LMP and F-test epilogues on the device's own spectra; prepare_audio without
the limiter).  End to end against the oracle, the spectra differ by the two FFTs' float32 rounding
(<= 1e-5 peak-normalised, test_gpu_parity.py), and LMP / F are ill-conditioned functions of the
spectra.  LMP and HP-ARMA are held to a MEASURED bound: the largest movement of the oracle's own
output, over the frames of the test, when every input sample is perturbed by at most one float ulp
(the bar VERDICT r1 item 6 asks for; 1e-5 is the floor).  The F statistic is a quotient num/den of
two spectrum-like sums, each of which carries the PSD tolerance; its bound is that tolerance
propagated through the quotient, plus distribution checks (median, argmax)."""
import ctypes as C
import glob
import os

import numpy as np
import pytest

from _exact import ftest64
from _ftest_check import check_ftest
from _signals import rel_err, synth

pytestmark = pytest.mark.gpu
TOL = 1e-5
GOLD = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _ulp_perturbations(x, k, seed=0):
    """k copies of x with every sample moved by -1, 0 or +1 float32 ulp."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(k):
        step = (rng.integers(0, 3, x.size) - 1).astype(np.float32)
        out.append(np.nextafter(x, x + step).astype(np.float32))
    return out


def _frame_err(got, ref):
    """per frame max|d| / max|ref| over the finite entries (both must agree on where those are)."""
    fin = np.isfinite(ref)
    assert np.array_equal(fin, np.isfinite(got))
    g = np.where(fin, got, 0.0).astype(np.float64)
    r = np.where(fin, ref, 0.0).astype(np.float64)
    return np.abs(g - r).max(axis=1) / np.abs(r).max(axis=1)


# ---- LMP ------------------------------------------------------------------------------------------
def _lmp_numpy(P, nl, first=0):
    frames, nb = P.shape
    out = np.empty((frames, nb), np.float64)
    ring = np.zeros((nl, nb), np.float64)
    for f in range(frames):
        ring[(first + f) % nl] = P[f]
        my = ring.sum(axis=0) / nl
        sy = ((ring - my) ** 2).sum(axis=0) / (nl - 1)
        v = 0.5 * (my - np.sqrt(np.maximum(my * my - sy, 0.0)))
        with np.errstate(divide="ignore", invalid="ignore"):
            o = -np.sqrt(nl / 2.0) + (nl * my) / (2.0 * np.sqrt(2.0 * nl) * v)
        o = np.where(o <= 1e-3, 1e-3, o)
        o[0] = 1e-3
        out[f] = o
    return out


@pytest.mark.parametrize("n,ovl,nl,sub_mean,frames", [(1024, 0.5, 4, 0, 40), (4096, 0.75, 4, 1, 37), (512, 0.0, 7, 0, 50),
                                                     (2048, 0.9, 3, 0, 33), (256, 0.0, 2, 1, 64), (1024, 0.0, 8, 0, 45)])
def test_lmp_vs_oracle(lib, oracle, torch_cuda, n, ovl, nl, sub_mean, frames):
    h = oracle.hop(n, ovl)
    x = synth(frames * h, fs=8000.0, seed=n + nl)
    want = oracle.spectrogram_lmp(x, n, ovl, nl, sub_mean=sub_mean)
    sp = lib.Spectrogram(lib.LmpParams(n=n, overlap=ovl, avg=nl, sub_mean=sub_mean))
    dx = torch_cuda.from_numpy(x).cuda()
    got = sp.run(dx).cpu().numpy()
    assert got.shape == want.shape == (frames, n // 2 + 1)
    assert np.all(got[:, 0] == np.float32(1e-3)) and got.min() >= np.float32(1e-3)
    # (a) the epilogue on the device's own periodograms: the reference's double formula, float out
    per = lib.Spectrogram(lib.FftParams(n=n, window_type=lib.WINDOWS["rectangular"], overlap=ovl, sub_mean=sub_mean))
    P = per.run(dx).cpu().numpy().astype(np.float64)
    assert np.allclose(got, _lmp_numpy(P, nl), rtol=3e-7, atol=0)
    # (b) end to end, per frame max|d|/max(ref): no worse than 3x the largest movement the oracle
    # itself makes in some frame of this stream under 1-ulp input perturbations (6 draws)
    spread = np.zeros(frames)
    for xp in _ulp_perturbations(x, 6, seed=n):
        spread = np.maximum(spread, _frame_err(oracle.spectrogram_lmp(xp, n, ovl, nl, sub_mean=sub_mean), want))
    err = _frame_err(got, want)
    print("lmp n=%d nl=%d: gpu err max %.2e, oracle 1-ulp spread max %.2e" % (n, nl, err.max(), spread.max()))
    assert err.max() <= max(TOL, 3.0 * spread.max()), (err.max(), spread.max())
    # a launch in the middle of the stream recomputes the ring's frames: same rows
    part = sp.run(dx, first_frame=5, nframes=frames - 9).cpu().numpy()
    assert np.array_equal(part.view(np.uint32), got[5:frames - 4].view(np.uint32))


def test_lmp_degenerate_and_golden(lib, oracle, torch_cuda):
    n, nl = 512, 4
    sp = lib.Spectrogram(lib.LmpParams(n=n, overlap=0.0, avg=nl))
    z = sp.run(torch_cuda.zeros(6 * n, device="cuda")).cpu().numpy()
    assert np.all(z[:, 0] == np.float32(1e-3)) and np.isnan(z[:, 1:]).all()           # 0/0, and NaN <= 1e-3 is false
    x = np.tile(synth(n, seed=3), 8)
    r = sp.run(torch_cuda.from_numpy(x).cuda()).cpu().numpy()
    assert np.isinf(r[nl - 1:, 1:]).all() and np.isfinite(r[:nl - 1, 1:]).all()       # variance 0 from the nl-th frame on
    one = lib.Spectrogram(lib.LmpParams(n=n, overlap=0.0, avg=1)).run(torch_cuda.from_numpy(synth(4 * n, seed=5)).cuda())
    assert np.isnan(one.cpu().numpy()[:, 1:]).all()                                    # nl - 1 = 0
    for path in sorted(glob.glob(os.path.join(GOLD, "l_*.npz"))):
        g = np.load(path)
        sp = lib.Spectrogram(lib.LmpParams(n=int(g["n"]), overlap=float(g["overlap"]), avg=int(g["nl"]), sub_mean=int(g["sub_mean"])))
        got = sp.run(torch_cuda.from_numpy(g["x"]).cuda()).cpu().numpy()
        assert np.all(_frame_err(got, g["out"]) < 1e-3), path      # the statistic's conditioning (up to 4e-4): test_lmp_vs_oracle


# ---- harmonic F-test --------------------------------------------------------------------------------
@pytest.mark.parametrize("n,ovl,nw,kmax,sub_mean,frames", [(1024, 0.0, 2.5, 4, 0, 12), (4096, 0.75, 4.0, 7, 0, 9),
                                                           (512, 0.5, 2.0, 2, 1, 20), (4096, 0.0, 2.5, 4, 0, 5)])
def test_ftest_vs_oracle(lib, oracle, torch_cuda, n, ovl, nw, kmax, sub_mean, frames):
    h = oracle.hop(n, ovl)
    x = synth(frames * h, fs=8000.0, seed=n + kmax)
    psd_w, want = oracle.spectrogram_mtm_ftest(x, n, ovl, nw, kmax, sub_mean=sub_mean, mu_live=1)
    sp = lib.Spectrogram(lib.MtmParams(n=n, overlap=ovl, w=nw, kmax=kmax, sub_mean=sub_mean))
    dx = torch_cuda.from_numpy(x).cuda()
    got = sp.ftest(dx).cpu().numpy()
    assert got.shape == want.shape
    half = n // 2
    # F = num/den, num = k |mu|^2 sum(U0^2) and den = sum_j |y_j - mu U0_j|^2 both spectrum-like sums that carry the PSD
    # tolerance (max-normalised TOL each): |dF| den <= TOL (max num + F max den) per frame and bin, the per-frame median of
    # |got/want - 1| below 1e-4, the strongest F of every frame in the same bin, and Nyquist (the denominator is never
    # accumulated -> x/0, as in the reference) non-finite in both: tests/_ftest_check.py.  num and den (float64, numpy)
    # weigh the bound; they are not what is compared.
    tapers, _ = oracle.dpss(n, kmax, nw)
    num, den, _ = ftest64(x, n, ovl, tapers, kmax, sub_mean=sub_mean)
    frac = check_ftest(got, want, num, den, kmax, tol=TOL)
    print("ftest n=%d kmax=%d: %.3f of the bound" % (n, kmax, frac))
    # the reference build without FFTW: mu is never written -> F = 0 (NaN at Nyquist: 0/0)
    dead = sp.ftest(dx, mu_live=False).cpu().numpy()
    assert np.all(dead[:, :half] == 0.0) and np.isnan(dead[:, half]).all()
    # the PSD path is untouched by the side computation
    assert max(max(rel_err(a, b)) for a, b in zip(sp.run(dx).cpu().numpy(), psd_w)) < TOL


def test_ftest_golden(lib, torch_cuda):
    for path in sorted(glob.glob(os.path.join(GOLD, "f_*mu1.npz"))):
        g = np.load(path)
        n = int(g["n"])
        sp = lib.Spectrogram(lib.MtmParams(n=n, overlap=float(g["overlap"]), w=float(g["nw"]), kmax=int(g["kmax"])))
        got = sp.ftest(torch_cuda.from_numpy(g["x"]).cuda()).cpu().numpy()[:, :n // 2].astype(np.float64)
        want = g["ftest"][:, :n // 2].astype(np.float64)
        # bins where F is large are exactly the ill-conditioned ones (tiny residual): compare in log
        assert np.median(np.abs(np.log(got / want))) < 1e-4, path
        assert np.mean(np.abs(np.log(got / want)) < 1e-2) > 0.97, path


# ---- prepare_audio ------------------------------------------------------------------------------------
@pytest.mark.parametrize("window,a,limiter,sub_mean,history_mode,ovl", [
    ("hanning", 0.0, 0, 0, 0, 0.5), ("kaiser", 0.0, 0, 1, 0, 0.75), ("blackman", 0.001, 0, 0, 0, 0.25),
    ("rectangular", 0.0, 0, 0, 1, 0.5), ("hamming", 0.0, 1, 0, 0, 0.0), ("gaussian", 0.01, 1, 1, 0, 0.9)])
def test_prepare_audio_frames(lib, oracle, torch_cuda, window, a, limiter, sub_mean, history_mode, ovl):
    """What prepare_audio leaves in inbuf_fft (fft.c:98-156), frame by frame, against the oracle's
    go_prepare: bit-exact without the limiter; the limiter's double log/exp may differ in the last
    bit of the float result."""
    n, frames = 1024, 9
    h = oracle.hop(n, ovl)
    x = synth(frames * h, fs=8000.0, seed=17)
    sp = lib.Spectrogram(lib.FftParams(n=n, window_type=lib.WINDOWS[window], overlap=ovl, a=a, limiter=limiter,
                                       sub_mean=sub_mean, history_mode=history_mode))
    got = sp.prepare(torch_cuda.from_numpy(x).cuda()).cpu().numpy()
    st = oracle._GoFftState()
    oracle._lib.go_fft_state_init(C.byref(st), n, C.c_float(ovl), oracle.WINDOWS[window], C.c_float(a), limiter, sub_mean)
    oracle._lib.go_prepare.argtypes = [C.c_void_p, np.ctypeslib.ndpointer(np.float32), C.c_int]
    for f in range(frames):
        hop = x[f * h:(f + 1) * h].copy()
        oracle._lib.go_prepare(C.byref(st), hop, 1 if (f == 0 or history_mode) else 0)
        want = np.ctypeslib.as_array(C.cast(st.inbuf_fft, C.POINTER(C.c_float)), shape=(n,)).copy()
        if sub_mean:
            # the hop mean: the reference adds the samples one by one in float, the device in a tree
            assert np.abs(got[f] - want).max() <= 2e-6 * max(1.0, np.abs(want).max()), f
        elif limiter:
            # (float)log((double)|y|) then exp(ftmp * 0.1) in double, rounded to float: a last-bit
            # difference of the device's double log moves ftmp by an ulp and the result by a few
            assert np.abs(got[f].view(np.int32).astype(np.int64) - want.view(np.int32)).max() <= 4, f
        else:
            assert np.array_equal(got[f].view(np.uint32), want.view(np.uint32)), f
    oracle._lib.go_fft_state_free(C.byref(st))


# ---- the file source's trailing partial block ---------------------------------------------------------
def _write_wav(path, samples, rate):
    import wave
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(samples.dtype.itemsize)
        w.setframerate(rate)
        w.writeframes(samples.tobytes())


@pytest.mark.parametrize("bits,extra", [(16, 200), (8, 333), (16, 1023), (8, 1)])
def test_wav_trailing_partial_block(lib, oracle, torch_cuda, tmp_path, bits, extra):
    """wav_fmt.c:102-119 behind GLFER_WAV_PARTIAL_TAIL: one more frame, fresh samples over the stale
    tail of the previous block -- AFTER its mean removal when sub_mean is on -- chunked or not."""
    n = 1024
    x = synth(11 * 1024 + extra, fs=8000.0, seed=bits + extra)
    raw = np.round(x * 30000).astype(np.int16) if bits == 16 else np.clip(np.round(x * 120 + 128), 0, 255).astype(np.uint8)
    path = tmp_path / "tail.wav"
    _write_wav(path, raw, 8000)
    fmt = lib.SAMPLES_S16 if bits == 16 else lib.SAMPLES_U8
    for params, mode, kw in (
            (lib.FftParams(n=n, window_type=7, overlap=0.5, sample_format=fmt, sub_mean=1), "fft", dict(window_type=7, sub_mean=1)),
            (lib.FftParams(n=n, window_type=0, overlap=0.0, sample_format=fmt, sub_mean=1), "fft", dict(window_type=0, sub_mean=1)),
            (lib.FftParams(n=n, window_type=0, overlap=0.75, sample_format=fmt), "fft", dict(window_type=0)),
            (lib.MtmParams(n=n, overlap=0.0, w=2.5, kmax=4, sample_format=fmt), "mtm", dict(nw=2.5, kmax=4))):
        want = oracle.wav_spectrogram(raw, bits, mode, n, params.overlap, **kw)
        sp = lib.Spectrogram(params)
        whole = raw.size // sp.hop
        assert want.shape[0] == whole + 1
        for chunk in (0, 32, 64):
            got = sp.run_wav(str(path), chunk_frames=chunk, partial_tail=True)
            assert got.shape == want.shape
            worst = max(max(rel_err(got[f], want[f])) for f in range(want.shape[0]))
            assert worst < TOL, (chunk, worst)
        # without the flag: whole blocks only, and those rows are the same
        body = sp.run_wav(str(path))
        assert body.shape[0] == whole and np.array_equal(body, got[:whole])


def test_wav_partial_block_edge_files(lib, oracle, torch_cuda, tmp_path):
    n = 1024
    sp = lib.Spectrogram(lib.FftParams(n=n, window_type=0, overlap=0.5, sample_format=lib.SAMPLES_S16, sub_mean=1))
    x = synth(3 * 512, fs=8000.0, seed=2)
    raw = np.round(x * 30000).astype(np.int16)
    # shorter than one block: fresh samples over the zeroed buffer (calloc, wav_fmt.c:99)
    p1 = tmp_path / "short.wav"
    _write_wav(p1, raw[:100], 8000)
    got = sp.run_wav(str(p1), partial_tail=True)
    want = oracle.wav_spectrogram(raw[:100], 16, "fft", n, 0.5, 0, sub_mean=1)
    assert got.shape == want.shape == (1, 513) and max(rel_err(got[0], want[0])) < TOL
    # a whole number of blocks: no extra frame
    p2 = tmp_path / "whole.wav"
    _write_wav(p2, raw, 8000)
    assert sp.run_wav(str(p2), partial_tail=True).shape[0] == 3
    # an odd last byte of a 16-bit file: a block with NO fresh sample -- the previous block again,
    # mean removed a second time
    p3 = tmp_path / "odd.wav"
    _write_wav(p3, raw, 8000)
    with open(p3, "ab") as f:
        f.write(b"\x7f")
    got = sp.run_wav(str(p3), partial_tail=True)
    pcm = np.concatenate([raw.view(np.uint8), np.array([0x7f], np.uint8)])
    want = oracle.wav_spectrogram(pcm, 16, "fft", n, 0.5, 0, sub_mean=1)
    assert got.shape == want.shape == (4, 513)
    assert max(max(rel_err(got[f], want[f])) for f in range(4)) < TOL


# ---- sharding with per-hop mean removal -----------------------------------------------------
def test_shards_with_mean_removal_and_ragged_history(lib, torch_cuda):
    """overlap 0.9 at N = 1024: hop 102, history 922 = 9.04 hops.  Per-hop means need whole hops, so
    a shard's halo is 10 hops (glfer_hip.h rule 2, shard.halo_samples); every shard computed from
    its own window alone must give the rows of the full run, bit for bit on aligned cuts."""
    from glfer_amd.shard import frame_range, halo_samples, run_shard, sample_window
    torch = torch_cuda
    for params, frames in ((lib.FftParams(n=1024, window_type=7, overlap=0.9, sub_mean=1), 333),
                           (lib.MtmParams(n=1024, overlap=0.9, w=2.5, kmax=4, sub_mean=1), 260),
                           (lib.MtmParams(n=4096, overlap=0.75, w=2.5, kmax=4, sub_mean=1), 131),
                           (lib.LmpParams(n=1024, overlap=0.5, avg=4, sub_mean=1), 200)):
        sp = lib.Spectrogram(params)
        x = torch.from_numpy(synth(frames * sp.hop, seed=23)).cuda()
        full = sp.run(x)
        extra = getattr(params, "avg", 1) - 1                  # LMP: the ring's frames are recomputed
        assert halo_samples(sp.hop, sp.n) % sp.hop == 0 and halo_samples(sp.hop, sp.n) >= sp.n - sp.hop
        for world in (2, 3):
            parts = []
            for rank in range(world):
                first, count = frame_range(frames, rank, world)
                begin, end = sample_window(first, count, sp.hop, sp.n, extra_frames=extra)
                local = x[begin:end].clone()                   # a rank holds only its window
                parts.append(run_shard(sp, local, begin, first, count))
            got = torch.cat(parts)
            same = (got == full) | (torch.isnan(got) & torch.isnan(full))
            assert bool(same.all()), (type(params).__name__, world)


# ---- host entries: the chunk ring, pinned rows, several "GPUs" -------------------------------------------
def test_host_ring_many_chunks_and_pinned_rows(lib, oracle, torch_cuda):
    """glfer_hip_spectrogram_host through >= 5 chunks (two streams in flight), rows into pageable and
    into pinned memory (direct DMA): identical to the one-launch device run."""
    for params, frames in ((lib.FftParams(n=1024, window_type=0, overlap=0.75, sub_mean=1), 70000),
                           (lib.MtmParams(n=1024, overlap=0.5, w=2.5, kmax=4), 70000),
                           (lib.LmpParams(n=1024, overlap=0.0, avg=4), 40000)):
        sp = lib.Spectrogram(params)
        x = synth(frames * sp.hop, seed=29)
        want = sp.run(torch_cuda.from_numpy(x).cuda()).cpu().numpy()
        got = sp.run_host(x)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
        pin = lib.PinnedArray((frames, sp.bins), np.float32)
        nf = C.c_size_t(0)
        lib.api._check(lib.api.lib().glfer_hip_spectrogram_host(sp._h, x.ctypes.data, x.size, pin.ptr, C.byref(nf)), "host")
        assert nf.value == frames and np.array_equal(pin.array.view(np.uint32), want.view(np.uint32))
        # the stream itself in pinned memory: uploaded from where it lies (no staging copy)
        pin_in = lib.PinnedArray((x.size,), np.float32)
        pin_in.array[:] = x
        pin.array[:] = 0
        lib.api._check(lib.api.lib().glfer_hip_spectrogram_host(sp._h, pin_in.ptr, x.size, pin.ptr, C.byref(nf)), "host, pinned in")
        assert nf.value == frames and np.array_equal(pin.array.view(np.uint32), want.view(np.uint32))
        pin_in.free()
        pin.free()
        # the Python mirror's pinned rows: same values, memory released with the array
        got_p = sp.run_host(x, pinned=True)
        assert np.array_equal(got_p.view(np.uint32), want.view(np.uint32))
        del got_p


def test_multi_gpu_entry_frame_ranges_on_one_device(lib, oracle, torch_cuda):
    """glfer_hip_spectrogram_host_multi with every device of the box in the mask; and the same
    partition arithmetic run as two and three 'ranks' on device 0 (the C entry's per-GPU job is
    glfer_hip_frame_range + the chunk ring from a frame offset) -- bit-identical to the one-shot run."""
    params = lib.MtmParams(n=4096, overlap=0.75, w=2.5, kmax=4, sub_mean=1)
    sp = lib.Spectrogram(params)
    frames = 3001
    x = synth(frames * sp.hop, seed=31)
    want = sp.run(torch_cuda.from_numpy(x).cuda()).cpu().numpy()
    ndev = torch_cuda.cuda.device_count()
    got = lib.spectrogram_host_multi(params, x, list(range(ndev)))
    assert got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # the ranges the entry hands its GPU threads
    for world in (2, 3, 8):
        cover = 0
        for r in range(world):
            first, count = lib.frame_range(frames, r, world)
            from glfer_amd.shard import frame_range as py_range
            assert (first, count) == py_range(frames, r, world) and first == cover
            assert first % 32 == 0 or first == frames
            cover += count
        assert cover == frames
    with pytest.raises(lib.GlferHipError, match="bad argument"):
        lib.spectrogram_host_multi(params, x, [ndev])          # a device the box does not have
    # two and three workers on device 0: one host thread, plan, stream pair and pinned ring each; every
    # worker but the first starts in the middle of the stream (frame offset, halo from the host array)
    for workers in ([0, 0], [0, 0, 0]):
        got = lib.spectrogram_host_multi(params, x, workers)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), workers
    for p2, fr in ((lib.FftParams(n=1024, window_type=7, overlap=0.9, sub_mean=1), 70001),      # ragged history: 9.04 hops
                   (lib.LmpParams(n=1024, overlap=0.5, avg=4), 40003),
                   (lib.MtmParams(n=16384, overlap=0.5, w=4.5, kmax=8, sample_format=lib.SAMPLES_S16), 700)):
        sp2 = lib.Spectrogram(p2)
        raw = synth(fr * sp2.hop, seed=43)
        if p2.sample_format == lib.SAMPLES_S16:
            raw = np.round(raw * 30000).astype(np.int16)
        one = sp2.run(torch_cuda.from_numpy(raw).cuda()).cpu().numpy()
        two = lib.spectrogram_host_multi(p2, raw, [0, 0])
        assert two.shape == one.shape
        same = (two == one) | (np.isnan(two) & np.isnan(one))
        assert same.all(), type(p2).__name__


def test_waterfall_host_entry(lib, oracle, torch_cuda):
    """Host samples -> RGB columns + levbuf through the ring: what the separate device calls give."""
    params = lib.FftParams(n=1024, window_type=7, overlap=0.5)
    sp = lib.Spectrogram(params)
    frames = 40000
    x = synth(frames * sp.hop, fs=8000.0, seed=37)
    psd = sp.run(torch_cuda.from_numpy(x).cuda())
    stats = lib.compute_floor(psd)
    for kw in (dict(scale_type=lib.SCALE_LOG, autoscale=1, overlap=0.5, palette=0),
               dict(scale_type=lib.SCALE_LIN, autoscale=0, max_level_db=-25.0, min_level_db=-70.0, thr_level=20.0, palette=1)):
        d1, d2 = lib.Display(**kw), lib.Display(**kw)
        rgb_w, lev_w, _ = lib.display(d1, psd, stats)
        rgb, lev = sp.waterfall_host(x, d2)
        assert np.array_equal(rgb, rgb_w.cpu().numpy()) and np.array_equal(lev, lev_w.cpu().numpy())
        assert (d1.first_buffer, d1.display_max_lvl, d1.display_min_lvl) == (d2.first_buffer, d2.display_max_lvl, d2.display_min_lvl)


# ---- HP-ARMA: the tolerance as a measured bound (VERDICT r1 item 6 i) ---------------------------------
@pytest.mark.parametrize("n,overlap,t,p_e", [(4096, 0.0, 128, 32), (1024, 0.5, 96, 16)])
def test_hparma_error_within_the_references_own_spread(lib, oracle, torch_cuda, n, overlap, t, p_e):
    """Per frame: the GPU's deviation from the oracle on |A(f)|^2 (= 1/psd below Nyquist),
    peak-normalised, against the ORACLE's own movement when every input sample is perturbed by at
    most one float ulp.  The AR vector is a noise-subspace direction of a nearly
    rank-deficient matrix: where the reference itself moves by s under such noise, no implementation
    that does not replay its every rounding can be held below ~s.  Bound per frame (tests/_spread.py): 1e-5 flat at
    BASELINE config 5's shape; max(1e-5, 3 s) elsewhere, with s the largest movement over the frames of the
    stream (a dozen draws sample a frame's own worst case poorly)."""
    from _spread import hparma_bound
    frames = 8
    h = oracle.hop(n, overlap)
    x = synth(frames * h, seed=n + t)
    bound, spread, ref = hparma_bound(oracle, x, n, overlap, t, p_e, 0, draws=12, seed=t)
    sp = lib.Spectrogram(lib.HparmaParams(n=n, overlap=overlap, t=t, p_e=p_e))
    got = sp.run(torch_cuda.from_numpy(x).cuda()).cpu().numpy().astype(np.float64)
    err = np.array([max(rel_err(1.0 / got[f, :n // 2], ref[f])) for f in range(frames)])
    print("hparma n=%d t=%d p_e=%d: gpu err %s  oracle 1-ulp spread %.2e  bound %.2e" % (n, t, p_e, np.array2string(err, precision=2), spread, bound))
    assert err.max() <= bound, (err, spread, bound)


# ---- kernel forms: the wavefront-private real-input form against the others ------------------------------
@pytest.mark.parametrize("n,overlap,fmt", [(2048, 0.5, "f32"), (4096, 0.75, "f32"), (4096, 0.75, "s16"), (8192, 0.0, "u8"),
                                           (16384, 0.5, "f32"), (4096, 0.9, "f32"), (2048, 0.0, "s16")])
def test_periodogram_forms_agree(lib, oracle, torch_cuda, n, overlap, fmt):
    """GLFER_FORM selects the kernel form per launch (h: spectro16h, w: spectro16w, x: packed): every
    form against the oracle, all windows' worth of options that reach the gather (history zeroed in
    every frame, PCM pairs), odd frame counts and launches that start inside the stream."""
    h = oracle.hop(n, overlap)
    frames = 45
    x = synth(frames * h + 5, seed=n) + np.float32(0.02)
    if fmt == "s16":
        raw = np.clip(np.round(x * 20000), -32768, 32767).astype(np.int16)
        xf, sf = oracle.pcm_s16_to_float(raw), lib.SAMPLES_S16
    elif fmt == "u8":
        raw = np.clip(np.round(x * 100 + 128), 0, 255).astype(np.uint8)
        xf, sf = oracle.pcm_u8_to_float(raw), lib.SAMPLES_U8
    else:
        raw, xf, sf = x, x, lib.SAMPLES_F32
    try:
        for history_mode in (0, 1):
            want = oracle.spectrogram_fft(xf, n, overlap, 7, history_mode=history_mode)
            sp = lib.Spectrogram(lib.FftParams(n=n, window_type=7, overlap=overlap, sample_format=sf, history_mode=history_mode))
            dx = torch_cuda.from_numpy(raw).cuda()
            for form in ("w", "h", "x"):
                os.environ["GLFER_FORM"] = form
                got = sp.run(dx).cpu().numpy()
                worst = max(max(rel_err(got[f], want[f])) for f in range(frames))
                assert worst < TOL, (form, history_mode, worst)
                part = sp.run(dx, first_frame=7, nframes=frames - 10).cpu().numpy()
                assert np.array_equal(part, got[7:frames - 3]), form
    finally:
        os.environ.pop("GLFER_FORM", None)


@pytest.mark.parametrize("n,overlap,fmt,frames", [(512, 0.75, "f32", 60001), (4096, 0.75, "f32", 20011), (4096, 0.5, "s16", 20002),
                                                  (4096, 0.875, "u8", 20003), (2048, 0.5, "f32", 30000), (16384, 0.75, "f32", 4099),
                                                  (1024, 0.875, "s16", 50001)])
def test_periodogram_register_reuse_over_long_launches(lib, oracle, torch_cuda, n, overlap, fmt, frames):
    """Launches long enough that spectro16h keeps the samples two overlapped frames share in
    registers (hop = 2, 4 or 8 sixteenths of the block; every frame slot of a workgroup walks
    consecutive frames): every row against the oracle, and a launch that starts elsewhere in the
    stream (other slot boundaries, ragged last workgroup) must give the same rows bit for bit."""
    h = oracle.hop(n, overlap)
    x = synth(frames * h + 3, seed=n + frames) + np.float32(0.01)
    if fmt == "s16":
        raw = np.clip(np.round(x * 20000), -32768, 32767).astype(np.int16)
        xf, sf = oracle.pcm_s16_to_float(raw), lib.SAMPLES_S16
    elif fmt == "u8":
        raw = np.clip(np.round(x * 100 + 128), 0, 255).astype(np.uint8)
        xf, sf = oracle.pcm_u8_to_float(raw), lib.SAMPLES_U8
    else:
        raw, xf, sf = x, x, lib.SAMPLES_F32
    want = oracle.spectrogram_fft(xf, n, overlap, 7)
    sp = lib.Spectrogram(lib.FftParams(n=n, window_type=7, overlap=overlap, sample_format=sf))
    dx = torch_cuda.from_numpy(raw).cuda()
    got = sp.run(dx).cpu().numpy()
    assert got.shape == want.shape
    peak = np.abs(want).max(axis=1, keepdims=True)
    worst = (np.abs(got - want) / peak).max()
    assert worst < TOL, worst
    part = sp.run(dx, first_frame=13, nframes=frames - 20).cpu().numpy()
    assert np.array_equal(part, got[13:frames - 7])


@pytest.mark.parametrize("n,overlap,fmt,frames", [(4096, 0.75, "f32", 20011), (4096, 0.0, "f32", 3001), (1024, 0.5, "s16", 50001),
                                                  (512, 0.875, "u8", 30001), (2048, 0.75, "f32", 57), (16384, 0.5, "f32", 2049),
                                                  (8192, 0.0, "s16", 300)])
@pytest.mark.parametrize("mean_mode", [1, 2], ids=["reference-order", "in-kernel-sums"])
def test_mean_removal_inside_the_periodogram_kernel(lib, oracle, torch_cuda, n, overlap, fmt, frames, mean_mode):
    """Per-hop mean removal (the reference's default) done inside spectro16h (hops of 2/4/8/16
    sixteenths of the block) -- with the hop means given in the reference's own order (cfg.sub_mean = 1, round 4:
    the table form, the means taken piece by piece beside the estimator launches) and with the kernel's own sums
    (GLFER_SUBMEAN_FAST): against the oracle, against the pre-pass form (GLFER_MEAN_PREPASS=1:
    the hop means are summed in another order there -- rounding-level agreement), and the same rows
    bit for bit from a launch that starts elsewhere (other slots, other register rotations)."""
    h = oracle.hop(n, overlap)
    x = synth(frames * h + 3, seed=n + frames) + np.float32(0.3)       # a DC offset worth removing
    if fmt == "s16":
        raw = np.clip(np.round(x * 20000), -32768, 32767).astype(np.int16)
        xf, sf = oracle.pcm_s16_to_float(raw), lib.SAMPLES_S16
    elif fmt == "u8":
        raw = np.clip(np.round(x * 100 + 128), 0, 255).astype(np.uint8)
        xf, sf = oracle.pcm_u8_to_float(raw), lib.SAMPLES_U8
    else:
        raw, xf, sf = x, x, lib.SAMPLES_F32
    sp = lib.Spectrogram(lib.FftParams(n=n, window_type=7, overlap=overlap, sub_mean=mean_mode, sample_format=sf))
    dx = torch_cuda.from_numpy(raw).cuda()
    got = sp.run(dx).cpu().numpy()
    nchk = min(frames, 600)                                             # the oracle on the first and last frames
    want_head = oracle.spectrogram_fft(xf[:nchk * h].copy(), n, overlap, 7, 0.0, 0, 1, 0)
    peak = np.abs(want_head).max(axis=1, keepdims=True)
    assert (np.abs(got[:nchk] - want_head) / peak).max() < TOL
    before = os.environ.get("GLFER_MEAN_PREPASS")
    try:
        os.environ["GLFER_MEAN_PREPASS"] = "1"
        pre = sp.run(dx).cpu().numpy()
    finally:
        if before is None:
            os.environ.pop("GLFER_MEAN_PREPASS", None)
        else:
            os.environ["GLFER_MEAN_PREPASS"] = before
    rowpeak = np.abs(pre).max(axis=1, keepdims=True)
    assert (np.abs(got - pre) / rowpeak).max() < 2e-6
    if frames > 40:
        part = sp.run(dx, first_frame=13, nframes=frames - 20).cpu().numpy()
        assert np.array_equal(part, got[13:frames - 7])


@pytest.mark.parametrize("n,overlap,kmax,fmt,frames", [(4096, 0.0, 4, "f32", 4001), (4096, 0.5, 2, "s16", 3000), (4096, 0.75, 6, "f32", 2501),
                                                       (4096, 0.0, 4, "u8", 64), (4096, 0.75, 4, "f32", 6),
                                                       (1024, 0.0, 7, "f32", 9001), (2048, 0.5, 4, "s16", 4000), (256, 0.75, 3, "u8", 9000),
                                                       (4096, 0.5, 5, "f32", 1500), (512, 0.0, 1, "f32", 7000),
                                                       (1024, 0.0, 4, "f32", 9001), (512, 0.5, 2, "s16", 9000), (256, 0.75, 4, "u8", 9001),
                                                       (1024, 0.75, 6, "f32", 5000),
                                                       (16384, 0.0, 8, "f32", 1100), (8192, 0.0, 4, "s16", 2100), (16384, 0.0, 8, "u8", 70),
                                                       (16384, 0.5, 8, "f32", 1200), (8192, 0.75, 4, "f32", 2200), (16384, 0.75, 5, "s16", 140),
                                                       (8192, 0.5, 7, "s16", 900)])
@pytest.mark.parametrize("mean_mode", [1, 2], ids=["reference-order", "in-kernel-sums"])
def test_mean_removal_inside_the_multitaper_kernel(lib, oracle, torch_cuda, n, overlap, kmax, fmt, frames, mean_mode):
    """The same for spectro16y (N = 4096, odd taper counts: frames taken in pairs, a lone first or last
    frame and the stream's first frames through the corrected copy) and for the packed kernel (even
    taper counts -- N = 1024 with 8 tapers at overlap 0 is the reference's default multitaper
    setting -- and the block sizes whose odd counts it takes) and for spectro16x / xl (odd counts
    up to N = 1024); hop = 4/8/16 sixteenths of the block.  N = 8192 / 16384 at overlap 0, 50, 75 %: the
    wavefront-private multitaper form, the hops' means across the frame's 4 / 8 wavefronts."""
    nw = 2.5 if kmax <= 4 else (4.5 if kmax == 8 else 4.0)
    h = oracle.hop(n, overlap)
    x = synth(frames * h + 3, seed=kmax + frames) + np.float32(0.3)
    if fmt == "s16":
        raw = np.clip(np.round(x * 20000), -32768, 32767).astype(np.int16)
        xf, sf = oracle.pcm_s16_to_float(raw), lib.SAMPLES_S16
    elif fmt == "u8":
        raw = np.clip(np.round(x * 100 + 128), 0, 255).astype(np.uint8)
        xf, sf = oracle.pcm_u8_to_float(raw), lib.SAMPLES_U8
    else:
        raw, xf, sf = x, x, lib.SAMPLES_F32
    sp = lib.Spectrogram(lib.MtmParams(n=n, overlap=overlap, w=nw, kmax=kmax, sub_mean=mean_mode, sample_format=sf))
    dx = torch_cuda.from_numpy(raw).cuda()
    got = sp.run(dx).cpu().numpy()
    nchk = min(frames, 300)
    want = oracle.spectrogram_mtm(xf[:nchk * h].copy(), n, overlap, nw, kmax, sub_mean=1, history_mode=0)
    peak = np.abs(want).max(axis=1, keepdims=True)
    assert (np.abs(got[:nchk] - want) / peak).max() < TOL
    before = os.environ.get("GLFER_MEAN_PREPASS")
    try:
        os.environ["GLFER_MEAN_PREPASS"] = "1"
        pre = sp.run(dx).cpu().numpy()
    finally:
        if before is None:
            os.environ.pop("GLFER_MEAN_PREPASS", None)
        else:
            os.environ["GLFER_MEAN_PREPASS"] = before
    rowpeak = np.abs(pre).max(axis=1, keepdims=True)
    assert (np.abs(got - pre) / rowpeak).max() < 2e-6
    if frames > 100:
        cnt = (frames - 39) // 32 * 32                                           # cuts on the frame-group grid (GLFER_FRAME_ALIGN): the same groups
        part = sp.run(dx, first_frame=32, nframes=cnt).cpu().numpy()
        assert np.array_equal(part, got[32:32 + cnt])
        odd = sp.run(dx, first_frame=13, nframes=frames - 20).cpu().numpy()      # off the grid: lone frames by other routes
        assert (np.abs(odd - got[13:frames - 7]) / np.abs(got[13:frames - 7]).max(axis=1, keepdims=True)).max() < 2e-6


@pytest.mark.parametrize("n,overlap,kmax,nw,sub_mean", [(2048, 0.25, 4, 2.5, 0), (4096, 0.0, 4, 2.5, 0), (4096, 0.75, 7, 4.0, 1),
                                                       (8192, 0.5, 4, 2.5, 0), (16384, 0.0, 8, 4.5, 0), (16384, 0.75, 1, 1.5, 1)])
def test_multitaper_forms_agree(lib, oracle, torch_cuda, n, overlap, kmax, nw, sub_mean):
    h = oracle.hop(n, overlap)
    frames = 19
    x = synth(frames * h, seed=n + kmax)
    want = oracle.spectrogram_mtm(x, n, overlap, nw, kmax, sub_mean=sub_mean)
    sp = lib.Spectrogram(lib.MtmParams(n=n, overlap=overlap, w=nw, kmax=kmax, sub_mean=sub_mean))
    dx = torch_cuda.from_numpy(x).cuda()
    try:
        for form in ("w", "h", "x"):
            os.environ["GLFER_FORM"] = form
            got = sp.run(dx).cpu().numpy()
            for f in range(frames):
                assert np.abs(got[f] - want[f]).max() <= TOL * want[f].max(), (form, f)
    finally:
        os.environ.pop("GLFER_FORM", None)


# ---- block sizes outside 256 .. 16384 (the reference takes any power of two, g_options.c:386-387) ---------
@pytest.mark.parametrize("n", [8, 16, 32, 64, 128, 32768, 65536])
def test_block_sizes_outside_the_16_point_range(lib, oracle, torch_cuda, n):
    """N = 8..128 (spectro_small.hip), N = 32768 and 65536 (spectro_big.hip: zero-history frames,
    RA9MB / limiter, integer samples on odd hops; the halfcomplex spectrum at 32768 from
    spectro16w.hip's general form): periodogram with every option, multitaper with odd and even
    taper counts, LMP, against the oracle."""
    big = n > 16384
    frames = 7 if big else 40
    for window, overlap, kw in (("hanning", 0.5, {}), ("kaiser", 0.0, dict(sub_mean=1)), ("blackman", 0.75, dict(a=0.001)),
                                ("hamming", 0.25, dict(limiter=1)), ("rectangular", 0.5, dict(history_mode=1))):
        h = oracle.hop(n, overlap)
        x = synth(frames * h + min(3, h - 1), fs=8000.0, seed=n) + np.float32(0.03)
        want = oracle.spectrogram_fft(x, n, overlap, oracle.WINDOWS[window], kw.get("a", 0.0), kw.get("limiter", 0),
                                      kw.get("sub_mean", 0), kw.get("history_mode", 0))
        sp = lib.Spectrogram(lib.FftParams(n=n, window_type=lib.WINDOWS[window], overlap=overlap, **kw))
        got = sp.run(torch_cuda.from_numpy(x).cuda()).cpu().numpy()
        tol = TOL                                                  # (the limiter too: fft.c:151-156 in double on the device since round 4)
        assert got.shape == want.shape == (frames, n // 2 + 1)
        if big and not kw:
            # At N = 32768 the REFERENCE's float32 recurrence-twiddle transform is itself ~7e-5 away from
            # exact arithmetic in this norm (fft_radix2.c:127-141; measured here with numpy's float64
            # rfft), so parity is: the device within 1e-6 of the exact transform, and no further from
            # the reference than the reference is from exact (x1.1)
            w64 = oracle.window(oracle.WINDOWS[window], n).astype(np.float64)
            fr = np.zeros(n)
            for f in range(frames):
                fr = np.concatenate([fr[h:], x[f * h:(f + 1) * h].astype(np.float64)])
                exact = np.abs(np.fft.rfft(fr * w64)) ** 2 / n
                ref_err = max(rel_err(want[f], exact))
                assert max(rel_err(got[f], exact)) < 1e-6, f
                assert max(rel_err(got[f], want[f])) <= max(TOL, 1.1 * ref_err), (f, ref_err)
            continue
        if big:
            tol = 2e-4 if n == 32768 else 1e-3                     # the reference's own error at these sizes, see above
        assert max(max(rel_err(got[f], want[f])) for f in range(frames)) < tol, (window, kw)
    if n > 32768:                      # no spectrum output from the two-kernel form (glfer_hip.h)
        with pytest.raises(lib.GlferHipError):
            lib.Spectrogram(lib.FftParams(n=n, window_type=0, overlap=0.0)).run(torch_cuda.zeros(n, device="cuda"), spectrum=True)
        torch_cuda.cuda.synchronize()
    # halfcomplex spectrum (what fft_do leaves in outbuf)
    x = synth(5 * n, fs=8000.0, seed=3)
    sp = lib.Spectrogram(lib.FftParams(n=n, window_type=0, overlap=0.0))
    w = oracle.window(0, n)
    psd, spec = sp.run(torch_cuda.from_numpy(x).cuda(), spectrum=True) if n <= 32768 else (None, None)
    for f in range(5 if n <= 32768 else 0):
        want = oracle.rfft_halfcomplex(w * x[f * n:(f + 1) * n])
        if big:                                                    # the reference transform is ~4e-5 off at this size: exact arithmetic instead
            X = np.fft.rfft((w * x[f * n:(f + 1) * n]).astype(np.float64))
            want = np.concatenate([X.real, X.imag[1:n // 2][::-1]])
        assert np.abs(spec[f].cpu().numpy() - want).max() <= 2e-6 * np.abs(want).max(), f
    # integer samples on an odd hop (pairs unaligned), PCM conversion in the gather
    raw = np.clip(np.round(synth(frames * n, seed=5) * 20000), -32768, 32767).astype(np.int16)
    sp = lib.Spectrogram(lib.FftParams(n=n, window_type=7, overlap=0.33, sample_format=lib.SAMPLES_S16))
    want = oracle.spectrogram_fft(oracle.pcm_s16_to_float(raw), n, 0.33, 7)
    got = sp.run(torch_cuda.from_numpy(raw).cuda()).cpu().numpy()
    assert max(max(rel_err(got[f], want[f])) for f in range(want.shape[0])) < ((2e-4 if n == 32768 else 1e-3) if big else TOL)
    # 8-bit samples, frames inside the stream (the staged gather of the two-kernel form at N >= 32768)
    raw8 = np.clip(np.round(synth((frames + 2) * (n // 2), seed=6) * 100 + 128), 0, 255).astype(np.uint8)
    sp = lib.Spectrogram(lib.FftParams(n=n, window_type=2, overlap=0.5, sample_format=lib.SAMPLES_U8))
    want = oracle.spectrogram_fft(oracle.pcm_u8_to_float(raw8), n, 0.5, 2)
    got = sp.run(torch_cuda.from_numpy(raw8).cuda()).cpu().numpy()
    assert max(max(rel_err(got[f], want[f])) for f in range(want.shape[0])) < ((2e-4 if n == 32768 else 1e-3) if big else TOL)
    # multitaper, odd and even counts; LMP
    for kmax, nw, overlap in ((4, 2.5, 0.5), (3, 2.5, 0.0), (0, 1.0, 0.0)):
        if n < 16 and kmax > 1:
            continue
        h = oracle.hop(n, overlap)
        x = synth(frames * h, fs=8000.0, seed=n + kmax)
        want = oracle.spectrogram_mtm(x, n, overlap, nw, kmax)
        got = lib.Spectrogram(lib.MtmParams(n=n, overlap=overlap, w=nw, kmax=kmax)).run(torch_cuda.from_numpy(x).cuda()).cpu().numpy()
        for f in range(frames):
            assert np.abs(got[f] - want[f]).max() <= ((2e-4 if n == 32768 else 1e-3) if big else TOL) * want[f].max(), (kmax, f)
    x = synth(frames * n, fs=8000.0, seed=9)
    got = lib.Spectrogram(lib.LmpParams(n=n, overlap=0.0, avg=3)).run(torch_cuda.from_numpy(x).cuda()).cpu().numpy()
    want = oracle.spectrogram_lmp(x, n, 0.0, 3)
    if big:     # the reference's transform is ~7e-5 off at this size and the statistic amplifies it: check the epilogue instead
        P = lib.Spectrogram(lib.FftParams(n=n, window_type=lib.WINDOWS["rectangular"], overlap=0.0)).run(
            torch_cuda.from_numpy(x).cuda()).cpu().numpy().astype(np.float64)
        assert np.allclose(got, _lmp_numpy(P, 3), rtol=3e-7, atol=0)
        assert np.all(_frame_err(got, want) < (5e-2 if n == 32768 else 0.25))      # the reference transform error, amplified
    else:
        assert np.all(_frame_err(got, want) < (1e-2 if n < 64 else 1e-3))     # the statistic's conditioning, see test_lmp_vs_oracle


def test_waterfall_device_tiles_equal_the_separate_stages(lib, torch_cuda):
    """glfer_hip_waterfall_device (floor -> [average] -> levels -> map, in tiles) against the three
    stages run over the whole batch: identical pixels, levbuf, statistics and carried state, with
    and without averaging, across tile boundaries (70 000 rows of 513 bins in tiles of 30 000)."""
    torch = torch_cuda
    os.environ["GLFER_WATERFALL_TILE"] = "30000"
    rows, bins = 70000, 513
    g = torch.Generator(device="cuda")
    g.manual_seed(5)
    psd = (torch.rand((rows, bins), device="cuda", generator=g) ** 4 * 1e-3).contiguous()
    stats = lib.compute_floor(psd)
    for kw in (dict(scale_type=lib.SCALE_LOG, autoscale=1, overlap=0.5, palette=0),
               dict(scale_type=lib.SCALE_LIN_MAX0, autoscale=0, max_level_db=-30.0, min_level_db=-80.0, thr_level=10.0, palette=5)):
        for avg_mode, max0 in ((0, 0), (lib.AVG_PLAIN, 0), (lib.AVG_SUMEXTREME, 1)):
            d1, d2 = lib.Display(**kw), lib.Display(**kw)
            if avg_mode:
                src, _ = lib.update_avg(avg_mode, psd, 4, 25, 500, max0=max0)
            else:
                src = psd
            rgb_w, lev_w, _ = lib.display(d1, src, stats)
            rgb, lev, st = lib.waterfall(d2, psd, avg_mode=avg_mode, depth=4, minbin=25, maxbin=500, max0=max0, want_stats=True)
            assert torch.equal(st, stats)
            if avg_mode == lib.AVG_SUMEXTREME:
                # reduction order of the band statistics differs between a restart and the full run by ulps
                assert (rgb != rgb_w).float().mean().item() < 1e-4 and (lev != lev_w).float().mean().item() < 1e-4
            else:
                assert torch.equal(rgb, rgb_w) and torch.equal(lev, lev_w), (kw["scale_type"], avg_mode)
            assert (d1.first_buffer, d1.display_max_lvl, d1.display_min_lvl) == (d2.first_buffer, d2.display_max_lvl, d2.display_min_lvl)
    os.environ.pop("GLFER_WATERFALL_TILE", None)


def test_bench_two_ranks_on_one_gpu():
    """`python bench.py --gpus 2` as the driver types it -- the parent starts the two ranks itself --
    end to end on this box's one GPU (GLFER_BENCH_REHEARSE=1: both ranks on cuda:0, gloo for the
    barrier and the max over ranks; a rehearsal of the launch path and the per-rank sharding, not a
    measurement).  Two GPU processes, within the box's limit."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, GLFER_BENCH_REHEARSE="1")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1",
                        "--frames", "8192", "--full", "--no-cpu-baseline"], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["n_gpus"] == 2 and line["scaling"] == "weak" and line["value"] > 0
    assert line["config"]["frames_per_gpu_per_step"] == 8192
    assert abs(line["value"] - 2 * 8192 / (line["ms_per_step"] * 1e-3)) < 1e-6 * line["value"]


def test_per_column_stages_at_n32768(lib, oracle, torch_cuda):
    """compute_floor, update_avg and the display map on 16385-bin rows (N = 32768): the floor's
    workgroup-per-row form with > 64 KB of dynamic LDS at 32769 bins is covered by
    test_floor_statistics_row_shapes; here the whole chain on real rows."""
    n = 32768
    x = synth(12 * n, fs=8000.0, seed=41)
    sp = lib.Spectrogram(lib.FftParams(n=n, window_type=7, overlap=0.0))
    psd = sp.run(torch_cuda.from_numpy(x).cuda())
    rows = psd.cpu().numpy()
    stats = lib.compute_floor(psd).cpu().numpy().astype(np.float64)
    want = np.array([oracle.floor_stats(r) for r in rows], np.float64)
    assert np.array_equal(stats[:, [0, 2, 3]], want[:, [0, 2, 3]]) and np.allclose(stats[:, 1], want[:, 1], rtol=TOL)
    avg, ret = lib.update_avg(lib.AVG_PLAIN, psd, 4, 100, 16000, n_out=n)
    a = oracle.Averager(n, 4)
    for f in range(rows.shape[0]):
        r, av, peak, _ = a.update("plain", rows[f], 100, 16000, n=16385)
        assert np.array_equal(avg[f, :16385].cpu().numpy(), av) and abs(ret[f, 0].item() / r - 1) < 1e-11 and int(ret[f, 1].item()) == peak
    d = lib.Display(scale_type=lib.SCALE_LOG, autoscale=1, overlap=0.0, palette=3)
    rgb, lev, _ = lib.display(d, psd, lib.compute_floor(psd))
    rgb_w, lev_w, _, _ = oracle.display(rows, stats, palette_id=3, scale_log=True, autoscale=True, overlap=0.0)
    assert np.array_equal(rgb.cpu().numpy(), rgb_w) and np.array_equal(lev.cpu().numpy(), lev_w)


@pytest.mark.parametrize("bins,minbin,maxbin,depth", [(513, 25, 500, 4), (129, 0, 129, 1), (2049, 0, 2049, 4), (2049, 30, 1999, 11),
                                                      (8193, 100, 8100, 6), (1025, 0, 1024, 40)])
def test_waterfall_averages_inside_the_map_kernel(lib, torch_cuda, bins, minbin, maxbin, depth):
    """update_avg_* taken inside the mapping kernel (no averaged rows in memory) against the staged
    form of the same entry (GLFER_WATERFALL_FUSED=0: update_avg rows, then the map): identical
    pixels, levbuf and carried state in every averaging mode and both normalisations, with bands
    that do and do not reach the row's ends, windows shorter and longer than a chunk restart, LDS
    ring and memory re-read forms (depth 40 at 1025 bins exceeds the ring), and across tile seams."""
    torch = torch_cuda
    rows = 3000 if bins > 4096 else 9000
    g = torch.Generator(device="cuda")
    g.manual_seed(bins + depth)
    psd = (torch.rand((rows, bins), device="cuda", generator=g) ** 4 * 1e-3 + 1e-9).contiguous()
    psd[rows // 3, minbin + (maxbin - minbin) // 3] = 0.7
    saved = {k: os.environ.get(k) for k in ("GLFER_WATERFALL_FUSED", "GLFER_WATERFALL_TILE")}
    try:
        for kw in (dict(scale_type=lib.SCALE_LOG, autoscale=1, overlap=0.5, palette=0),
                   dict(scale_type=lib.SCALE_LIN, autoscale=1, overlap=0.0, palette=3),
                   dict(scale_type=lib.SCALE_LOG_MAX0, autoscale=0, max_level_db=0.0, min_level_db=-60.0, thr_level=10.0, palette=5)):
            for avg_mode in (lib.AVG_PLAIN, lib.AVG_SUMEXTREME, lib.AVG_SUMAVG):
                for max0 in (0, 1):
                    out = {}
                    for fused, tile in (("0", None), ("1", None), ("1", str(rows // 3 + 7))):
                        os.environ["GLFER_WATERFALL_FUSED"] = fused
                        if tile:
                            os.environ["GLFER_WATERFALL_TILE"] = tile
                        else:
                            os.environ.pop("GLFER_WATERFALL_TILE", None)
                        d = lib.Display(**kw)
                        rgb, lev, _ = lib.waterfall(d, psd, avg_mode=avg_mode, depth=depth, minbin=minbin, maxbin=maxbin, max0=max0,
                                                    want_stats=True)
                        out[(fused, tile)] = (rgb, lev, (d.first_buffer, d.display_max_lvl, d.display_min_lvl))
                    want = out[("0", None)]
                    got = out[("1", None)]
                    assert got[2] == want[2]
                    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), (kw["scale_type"], avg_mode, max0)
                    tiled = out[("1", str(rows // 3 + 7))]
                    assert tiled[2] == want[2]
                    if avg_mode == lib.AVG_PLAIN:
                        assert torch.equal(tiled[0], want[0]) and torch.equal(tiled[1], want[1])
                    else:   # the chunk restarts fall elsewhere: band statistics differ by ulps in a few columns
                        assert (tiled[0] != want[0]).float().mean().item() < 1e-4 and (tiled[1] != want[1]).float().mean().item() < 1e-4
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def test_waterfall_plain_average_against_the_oracle(lib, oracle, torch_cuda):
    """The fused average-and-map kernel against the oracle's row-by-row chain (compute_floor ->
    update_avg_plain -> the waterfall loop): plain averaging is bit-identical to avg.c, so pixels and
    levbuf must be identical too."""
    rng = np.random.default_rng(77)
    frames, bins, depth, minbin, maxbin = 400, 513, 4, 10, 500
    p = (rng.random((frames, bins)) ** 4 * 1e-2 + 1e-8).astype(np.float32)
    stats = np.array([oracle.floor_stats(r) for r in p], np.float32)
    a = oracle.Averager(bins, depth)
    avg = np.stack([a.update("plain", p[f], minbin, maxbin, n=bins)[1] for f in range(frames)])
    for scale_type, autoscale in ((lib.SCALE_LOG, 1), (lib.SCALE_LIN, 0)):
        w_rgb, w_lev, _, _ = oracle.display(avg, stats, palette_id=2, scale_log=scale_type >= 2, autoscale=bool(autoscale),
                                            overlap=0.5, max_level_db=-20.0, min_level_db=-70.0)
        d = lib.Display(palette=2, scale_type=scale_type, autoscale=autoscale, overlap=0.5, max_level_db=-20.0, min_level_db=-70.0)
        rgb, lev, _ = lib.waterfall(d, torch_cuda.from_numpy(p).cuda(), avg_mode=lib.AVG_PLAIN, depth=depth, minbin=minbin, maxbin=maxbin,
                                    want_stats=True)
        assert np.array_equal(lev.cpu().numpy(), w_lev), scale_type
        assert np.array_equal(rgb.cpu().numpy(), w_rgb), scale_type


def test_kept_scratch_blocks_across_streams(lib, torch_cuda):
    """Scratch of 16 MiB and more comes from blocks the library keeps; a block given back on one stream
    and taken again on another first waits for the event recorded at the give-back.  The staged
    waterfall (averaged rows as scratch: 20000 x 513 doubles = 82 MB) alternately on two streams with
    different inputs, no host synchronisation in between, against the same calls on one stream."""
    torch = torch_cuda
    rows, bins = 20000, 513
    g = torch.Generator(device="cuda")
    g.manual_seed(9)
    inputs = [(torch.rand((rows, bins), device="cuda", generator=g) ** 4 * 1e-3 + 1e-9).contiguous() for _ in range(4)]
    saved = os.environ.get("GLFER_WATERFALL_FUSED")
    os.environ["GLFER_WATERFALL_FUSED"] = "0"
    try:
        kw = dict(scale_type=lib.SCALE_LOG, autoscale=1, overlap=0.5, palette=1)
        want = [lib.waterfall(lib.Display(**kw), x, avg_mode=lib.AVG_SUMEXTREME, depth=5, minbin=3, maxbin=500)[0].clone() for x in inputs]
        torch.cuda.synchronize()
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        got = []
        for rep in range(3):
            for i, x in enumerate(inputs):
                with torch.cuda.stream(streams[i % 2]):
                    got.append((i, lib.waterfall(lib.Display(**kw), x, avg_mode=lib.AVG_SUMEXTREME, depth=5, minbin=3, maxbin=500)[0]))
        torch.cuda.synchronize()
        for i, rgb in got:
            assert torch.equal(rgb, want[i]), i
    finally:
        if saved is None:
            os.environ.pop("GLFER_WATERFALL_FUSED", None)
        else:
            os.environ["GLFER_WATERFALL_FUSED"] = saved
