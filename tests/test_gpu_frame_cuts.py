"""The edges of the launchers' frame cuts at the smallest shapes (-m gpu).  glfer_amd/csrc/frame_cuts.h cuts a call's frames
into head (the stream's first frames and the frames below the first whole frame group: packed kernel, corrected copy), body
(whole, globally aligned groups: the route's kernel) and tail; the single, batch, ragged and F entries all cut with it.  Here
calls start and end ON, one BELOW and one ABOVE every edge -- first in {0, 1, first_inside, G-1, G, G+1}, nframes in
{1, G-1, G, 2G+1} -- on one plan per route:

    A  N = 1024, 5 tapers, overlap 0.5    shared-odd (spectro16x / xl)   G = 8, first_inside = 1     (also with s16 samples)
    B  N = 4096, 5 tapers, overlap 0.75   shared-odd (spectro16y)        G = 2, first_inside = 3
    C  N = 1024, periodogram, 0.75        real-input (spectro16h)        G = 1, first_inside = 3     (also with ZERO_ALWAYS history)
    D  N = 256,  periodogram, 0.5         packed                         no groups (cut as G = 1), first_inside = 1

each with sub_mean 0, 1 (the reference's summation order) and GLFER_SUBMEAN_FAST.  The single-stream rows are held to the
oracle (per frame max|d|/max and ||d||2/||ref||2 <= 1e-5); the batch, ragged and batched F entries to the
single-stream entry, bit for bit.

The oracle-checked stream is zero-mean noise: GLFER_SUBMEAN_FAST sums a hop in another order than the reference, a deviation
that grows with |hop mean| / rms (include/glfer_hip.h) and is no part of what is tested here.  The other two streams of a batch
differ from it in amplitude and DC level, so that a row or a mean taken from the wrong stream cannot come out equal.
"""
import numpy as np
import pytest

from _signals import rel_err, synth

pytestmark = pytest.mark.gpu
TOL = 1e-5
FRAMES = 48

# name: (kind, n, overlap, sample format, history_mode, G, first_inside)
PLANS = {
    "A": ("mtm", 1024, 0.5, 0, 0, 8, 1), "A_s16": ("mtm", 1024, 0.5, 1, 0, 8, 1),
    "B": ("mtm", 4096, 0.75, 0, 0, 2, 3),
    "C": ("fft", 1024, 0.75, 0, 0, 1, 3), "C_zero_always": ("fft", 1024, 0.75, 0, 1, 1, 3),
    "D": ("fft", 256, 0.5, 0, 0, 1, 1),
}
SUB_MEANS = {"sub0": 0, "sub1": 1, "fast": 2}


def _uniq(values):
    return [v for i, v in enumerate(values) if v > -1 and v not in values[:i]]


def _calls(G, fi):
    firsts = _uniq([0, 1, fi, G - 1, G, G + 1])
    counts = [c for c in _uniq([1, G - 1, G, 2 * G + 1]) if c > 0]
    return [(f, c) for f in firsts for c in counts]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _raw(x, fmt):
    """(samples as the plan takes them, the floats the reference sees)"""
    if fmt == 1:
        raw = np.clip(np.round(x * 20000.0), -32768, 32767).astype(np.int16)
        return raw, raw.astype(np.float32) / np.float32(32768.0)
    return x.astype(np.float32), x.astype(np.float32)


def _stream(b, nsamples):
    if b == 0:
        return (0.3 * np.random.default_rng(5).standard_normal(nsamples)).clip(-0.99, 0.99)
    return (0.4 + 0.25 * b) * synth(max(nsamples, 1), seed=3000 + b)[:nsamples].astype(np.float64) + 0.07 * (2 * b - 3)


_made = {}


def _setup(torch, lib, oracle, plan, sub):
    """(Spectrogram, [3, T] device streams, the oracle's rows of stream 0), built once per plan and sub_mean"""
    key = (plan, sub)
    if key not in _made:
        kind, n, overlap, fmt, hm, G, fi = PLANS[plan]
        sm = SUB_MEANS[sub]
        assert sm in (0, lib.SUBMEAN_EXACT, lib.SUBMEAN_FAST)
        common = dict(n=n, overlap=overlap, sub_mean=sm, history_mode=hm, sample_format=fmt)
        params = lib.MtmParams(w=2.5, kmax=4, **common) if kind == "mtm" else lib.FftParams(window_type=lib.WINDOWS["hanning"], **common)
        sp = lib.Spectrogram(params)
        assert sp.hop == int(n * (1.0 - overlap)) and -(-(n - sp.hop) // sp.hop) == fi
        nsamples = (FRAMES * sp.hop + sp.hop // 3) & ~1                  # (integer samples: an even stream pitch)
        raws, floats = zip(*(_raw(_stream(b, nsamples), fmt) for b in range(3)))
        ref_mean = 1 if sm else 0
        want = (oracle.spectrogram_mtm(floats[0], n, overlap, 2.5, 4, sub_mean=ref_mean, history_mode=hm) if kind == "mtm" else
                oracle.spectrogram_fft(floats[0], n, overlap, oracle.WINDOWS["hanning"], 0.0, 0, ref_mean, hm))
        _made[key] = (sp, torch.from_numpy(np.stack(raws)).to("cuda:0"), want)
    return _made[key]


@pytest.mark.parametrize("sub", sorted(SUB_MEANS))
@pytest.mark.parametrize("plan", sorted(PLANS))
def test_single_rows_match_the_oracle_and_batches_match_single(torch_cuda, lib, oracle, plan, sub):
    torch = torch_cuda
    sp, x, want = _setup(torch, lib, oracle, plan, sub)
    G, fi = PLANS[plan][5:]
    worst = 0.0
    for first, count in _calls(G, fi):
        assert first + count <= FRAMES
        single = torch.stack([sp.run(x[b], first_frame=first, nframes=count) for b in range(3)])
        batch = sp.run_batch(x, first_frame=first, nframes=count)
        torch.cuda.synchronize()
        assert torch.equal(batch, single), (plan, sub, first, count)
        rows = single[0, :, :sp.bins].cpu().numpy()
        for f in range(count):
            e_max, e_l2 = rel_err(rows[f], want[first + f])
            worst = max(worst, e_max, e_l2)
            assert e_max <= TOL and e_l2 <= TOL, (plan, sub, first, count, f, e_max, e_l2)
    print("frame cuts %s %s: %d calls, worst error against the oracle %.2e" % (plan, sub, len(_calls(G, fi)), worst))


@pytest.mark.parametrize("sub", sorted(SUB_MEANS))
@pytest.mark.parametrize("plan", sorted(PLANS))
def test_ragged_streams_on_the_cut_edges_match_single(torch_cuda, lib, oracle, plan, sub):
    """whole streams of 0, first_inside, first_inside + G - 1, 2G + 3 and 4G frames in one ragged call"""
    torch = torch_cuda
    sp, x, _ = _setup(torch, lib, oracle, plan, sub)
    fmt, G, fi = PLANS[plan][3], PLANS[plan][5], PLANS[plan][6]
    frames = [0, fi, fi + G - 1, 2 * G + 3, 4 * G]
    lens = [sp.hop - 1, fi * sp.hop, (fi + G - 1) * sp.hop + sp.hop // 2, (2 * G + 3) * sp.hop + 1, 4 * G * sp.hop]
    gap = 6
    fill = float("nan") if fmt == 0 else 32767
    buf = torch.full((sum(lens) + gap * (len(lens) + 1) + len(lens),), fill, dtype=x.dtype, device="cuda:0")
    offs, at = [], 0
    for b, n in enumerate(lens):                                   # stream b: a piece of batch stream b % 3, from another start each
        at += gap
        at += at & 1
        offs.append(at)
        buf[at:at + n] = x[b % 3, b * 7:b * 7 + n]
        at += n
    got, starts = sp.run_ragged(buf, offs, lens)
    torch.cuda.synchronize()
    assert list(starts) == [0] + list(np.cumsum(frames))
    for b, (o, n) in enumerate(zip(offs, lens)):
        if frames[b]:
            single = sp.run(buf[o:o + n])
            torch.cuda.synchronize()
            assert torch.isfinite(single[:, :sp.bins]).all()
            assert torch.equal(got[int(starts[b]):int(starts[b + 1])], single), (plan, sub, b, frames[b])


def test_batched_f_rows_match_the_single_f_entry(torch_cuda, lib, oracle):
    """plan A with the reference's mean removal: the batched F entry cuts its corrected copies as the single entry does"""
    torch = torch_cuda
    sp, x, _ = _setup(torch, lib, oracle, "A", "sub1")
    G, fi = PLANS["A"][5:]
    for first, count in _calls(G, fi):
        single = torch.stack([sp.ftest(x[b], first_frame=first, nframes=count) for b in range(3)])
        batch = sp.ftest_batch(x, first_frame=first, nframes=count)
        torch.cuda.synchronize()
        assert torch.equal(batch, single), (first, count)
