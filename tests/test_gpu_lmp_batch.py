"""The LMP statistic as a stage of its own (lmp_statistic, lmp_statistic_batch, lmp_statistic_ragged) and LMP plans through the
batch and ragged entries in one launch set.  The contract is bit for bit: every output equals what the single-stream LMP
entry (Spectrogram(LmpParams).run) writes for that stream, so rows are compared as uint32 views.  A float64 restatement of
lmp.c:132-160 (written here) bounds the statistic itself at rtol = 3e-7, the rule of test_lmp_vs_oracle (a)."""
import numpy as np
import pytest

from _signals import synth

pytestmark = pytest.mark.gpu

AVGS = (1, 2, 3, 4, 8, 7, 16)


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def rect(lib, n, **k):
    return lib.Spectrogram(lib.FftParams(n=n, window_type=lib.WINDOWS["rectangular"], overlap=0.0, **k))


def lmp(lib, n, avg, **k):
    return lib.Spectrogram(lib.LmpParams(n=n, overlap=0.0, avg=avg, **k))


def run_whole(sp, v):
    """sp.run(v); a stream shorter than a hop has no rows (and an empty tensor no address to pass)"""
    import torch
    return sp.run(v) if v.numel() >= sp.hop else torch.empty((0, sp.pitch), dtype=torch.float32, device=v.device)


def lmp_float64(P, nl):
    """lmp.c:132-160 over periodogram rows P [frames][bins]: the ring of the last nl rows, written round-robin and zero before
    its first write, summed over the slots in slot order in float64; the statistic rounded to float32 as psd_buf is"""
    frames, nbins = P.shape
    ring = np.zeros((nl, nbins), np.float64)
    out = np.empty((frames, nbins), np.float32)
    with np.errstate(all="ignore"):
        for f in range(frames):
            ring[f % nl] = P[f]
            my = np.zeros(nbins)
            for j in range(nl):
                my += ring[j]
            my /= nl
            sy = np.zeros(nbins)
            for j in range(nl):
                sy += (ring[j] - my) * (ring[j] - my)
            sy /= (nl - 1)
            v_hat = my * my - sy
            v_hat[v_hat < 0.0] = 0.0
            v_hat = 0.5 * (my - np.sqrt(v_hat))
            r = (-np.sqrt(nl / 2.0) + (nl * my) / (2.0 * np.sqrt(2.0 * nl) * v_hat)).astype(np.float32)
            r[r <= 1.0e-3] = 1e-3
            r[0] = 1e-3
            out[f] = r
    return out


@pytest.fixture(scope="module")
def one_stream(lib, torch):
    """per (n, frames): the samples, the rectangular-window periodogram rows, and per avg the LMP estimator's rows (computed once)"""
    made = {}

    def get(n, frames):
        if (n, frames) not in made:
            x = torch.from_numpy(synth(frames * n, fs=8000.0, seed=n + frames)).cuda()
            P = rect(lib, n).run(x)
            made[(n, frames)] = (x, P, {avg: lmp(lib, n, avg).run(x) for avg in AVGS})
        return made[(n, frames)]
    return get


@pytest.mark.parametrize("frames", [5, 70])             # the LDS ring starts at 64 frames: frame by frame below, the ring above
@pytest.mark.parametrize("n", [256, 1024])              # 129 bins: less than one bin block; 513: a ragged last bin block
def test_stage_equals_estimator(lib, torch, one_stream, n, frames):
    x, P, want = one_stream(n, frames)
    for avg in AVGS:
        sp = lmp(lib, n, avg)
        for first in (0, 1, avg, avg + 1):
            if first >= frames:
                continue
            lead = min(avg - 1, first)
            got = lib.lmp_statistic(P[first - lead:], avg, first_frame=first, lead=lead)
            assert same(got, want[avg][first:]), (avg, first)
            if first:
                assert same(got, sp.run(x, first_frame=first)), (avg, first)        # the estimator started there itself
                more = lib.lmp_statistic(P, avg, first_frame=first, lead=first)     # rows that reach further back than needed
                assert same(more, got), (avg, first)


@pytest.mark.parametrize("frames", [5, 70])
@pytest.mark.parametrize("n", [256, 1024])
def test_stage_against_float64(lib, torch, one_stream, n, frames):
    x, P, want = one_stream(n, frames)
    Pn = P.cpu().numpy().astype(np.float64)
    for avg in AVGS:
        got = lib.lmp_statistic(P, avg).cpu().numpy()
        assert np.all(got[:, 0] == np.float32(1e-3))
        if avg == 1:                                     # nl - 1 = 0: 0/0 in every other bin (test_lmp_degenerate_and_golden)
            assert np.isnan(got[:, 1:]).all()
            continue
        ref = lmp_float64(Pn, avg)
        worst = np.nanmax(np.abs(got - ref) / np.abs(ref))
        print("lmp_statistic n=%d frames=%d avg=%d: max rel err vs float64 %.2e" % (n, frames, avg, worst))
        assert np.allclose(got, ref, rtol=3e-7, atol=0), (avg, worst)
        assert got.min() >= np.float32(1e-3)


@pytest.fixture(scope="module")
def streams33(torch):
    """33 streams of 70 frames at N = 256 (f32), and their s16 form"""
    n, frames, B = 256, 70, 33
    x = np.stack([synth(frames * n, fs=8000.0, seed=100 + b) for b in range(B)])
    return torch.from_numpy(x).cuda(), torch.from_numpy(np.round(x * 20000).astype(np.int16)).cuda()


@pytest.mark.parametrize("B", [3, 33])
def test_batch_stage_equals_single_calls(lib, torch, streams33, B):
    xs = streams33[0][:B]
    n = 256
    P = rect(lib, n).run_batch(xs)                       # [B][70][129]
    for avg in AVGS:
        for first in sorted({0, 1, avg - 2, avg + 1, 2 * avg + 1} - {-1}):   # 1, avg - 2: first < avg - 1; avg + 1: not a multiple of avg
            if first < 0 or first >= P.size(1):
                continue
            lead = min(avg - 1, first)
            view = P[:, first - lead:]                   # a slice along the frames: the streams stay 70 rows apart
            got = lib.lmp_statistic_batch(view, avg, first_frame=first, lead=lead)
            assert got.shape == (B, P.size(1) - first, P.size(2))
            for b in range(B):
                assert same(got[b], lib.lmp_statistic(view[b].contiguous(), avg, first_frame=first, lead=lead)), (avg, first, b)
    few = lib.lmp_statistic_batch(P[:, :5].contiguous(), 7)                   # under the LDS ring's 64 frames: frame by frame
    for b in range(B):
        assert same(few[b], lib.lmp_statistic(P[b, :5].contiguous(), 7)), b


def test_ring_above_64_from_a_later_frame(lib, torch, streams33):
    """avg = 65 is past the sizes of the ring in LDS: every entry goes frame by frame, and a frame's slot (frame mod avg) is taken
    in 32 bits from the launch's first frame mod avg, which the host computes.  first = 1 and 66 make that remainder 1 (66: past
    one whole turn of the ring); AVGS stops at 16, where 70 frames take the ring kernels instead."""
    n, avg, B, frames = 256, 65, 3, 70
    xs = streams33[0][:B]
    P = rect(lib, n).run_batch(xs)                       # [3][70][129]
    sp = lmp(lib, n, avg)
    ref = [lmp_float64(P[b].cpu().numpy().astype(np.float64), avg) for b in range(B)]
    packed, _ = lib.lmp_statistic_ragged(P.reshape(B * frames, 129), np.arange(B + 1) * frames, avg)
    for first in (0, 1, 66):
        lead = min(avg - 1, first)
        view = P[:, first - lead:]
        batch = lib.lmp_statistic_batch(view, avg, first_frame=first, lead=lead)
        for b in range(B):
            want = sp.run(xs[b], first_frame=first)      # the one-stream estimator, started at `first` itself
            stage = lib.lmp_statistic(view[b].contiguous(), avg, first_frame=first, lead=lead)
            assert same(stage, want), (first, b)
            assert same(batch[b], want), (first, b)
            assert same(packed[b * frames + first:(b + 1) * frames], want), (first, b)
            got = stage.cpu().numpy()
            worst = np.nanmax(np.abs(got - ref[b][first:]) / np.abs(ref[b][first:]))
            print("lmp_statistic avg=65 first=%d stream %d: max rel err vs float64 %.2e" % (first, b, worst))
            assert np.allclose(got, ref[b][first:], rtol=3e-7, atol=0), (first, b, worst)


@pytest.mark.parametrize("sub_mean", [0, 1])
@pytest.mark.parametrize("B", [3, 33])
def test_run_batch_equals_loop_of_run(lib, torch, streams33, B, sub_mean):
    xs = streams33[0][:B]
    for n, avg in ((256, 4), (1024, 4), (256, 7), (256, 3)):
        sp = lmp(lib, n, avg, sub_mean=sub_mean)
        for first in (0, 3) if avg == 4 else (0, avg + 1):
            got = sp.run_batch(xs, first_frame=first)
            for b in range(B):
                assert same(got[b], sp.run(xs[b], first_frame=first)), (n, avg, first, b)
    sp = lmp(lib, 256, 7, sub_mean=sub_mean)
    got = sp.run_batch(xs, first_frame=2, nframes=5)     # few frames in the middle: the frame-by-frame form of the batch
    for b in range(B):
        assert same(got[b], sp.run(xs[b], first_frame=2, nframes=5)), b


def test_run_batch_s16(lib, torch, streams33):
    xs = streams33[1][:5]
    for sub_mean in (0, 1):
        sp = lmp(lib, 256, 4, sub_mean=sub_mean, sample_format=lib.SAMPLES_S16)
        for first in (0, 3):
            got = sp.run_batch(xs, first_frame=first)
            for b in range(xs.size(0)):
                assert same(got[b], sp.run(xs[b], first_frame=first)), (sub_mean, first, b)


def _ragged_lengths(avg, n):
    frames = [0, 1, 2, avg - 1, 15, 16, 17, 70, 0, 0, 16]
    order = np.random.default_rng(avg).permutation(len(frames))
    return [frames[i] * n + (7 if k % 3 == 0 else 0) for k, i in enumerate(order)]      # a few samples short of another hop


@pytest.mark.parametrize("avg", [3, 4, 7])
def test_ragged_stage_and_sentinel(lib, torch, streams33, avg):
    n = 256
    lens = _ragged_lengths(avg, n)
    views = [streams33[0][b, :m] for b, m in enumerate(lens)]
    per = rect(lib, n)
    rows = [run_whole(per, v) for v in views]
    packed = torch.cat([torch.zeros((2, 129), device="cuda")] + rows + [torch.zeros((3, 129), device="cuda")])   # rows no stream owns at both ends
    starts = np.concatenate([[2], 2 + np.cumsum([r.size(0) for r in rows])])
    sentinel = torch.full_like(packed, -77.0)
    before = bits(sentinel).copy()
    out, st = lib.lmp_statistic_ragged(packed, starts, avg, out=sentinel)
    assert out is sentinel and list(st) == list(starts)
    sp = lmp(lib, n, avg)
    for b, v in enumerate(views):
        assert same(out[starts[b]:starts[b + 1]], run_whole(sp, v)), (avg, b, lens[b] // n)
    got = bits(out)
    assert np.array_equal(got[:2], before[:2]) and np.array_equal(got[-3:], before[-3:])   # nothing outside the streams' rows


@pytest.mark.parametrize("history_mode", [0, 1])
@pytest.mark.parametrize("sub_mean", [0, 1])
@pytest.mark.parametrize("avg", [3, 4, 7])
def test_run_ragged_equals_single_calls(lib, torch, streams33, avg, sub_mean, history_mode):
    n = 256
    lens = _ragged_lengths(avg, n)
    offs = [b * streams33[0].size(1) for b in range(len(lens))]
    flat = streams33[0].reshape(-1)
    sp = lmp(lib, n, avg, sub_mean=sub_mean, history_mode=history_mode)
    total, starts = sp.ragged_frames(lens)
    out = torch.full((total + 4, 129), -77.0, device="cuda")
    got, st = sp.run_ragged(flat, offs, lens, out=out)
    assert list(st) == list(starts)
    want = [run_whole(sp, flat[o:o + m]) for o, m in zip(offs, lens)]
    for b in range(len(lens)):
        assert same(out[starts[b]:starts[b + 1]], want[b]), (avg, sub_mean, history_mode, b, lens[b] // n)
    assert (bits(out[total:]) == np.float32(-77.0).view(np.uint32)).all()     # nothing past the last stream's rows
    if sub_mean == 0 and history_mode == 0:
        listed = sp.run_list([flat[o:o + m] for o, m in zip(offs, lens)])
        for b in range(len(lens)):
            assert same(listed[b], want[b]), (avg, b)


def test_run_ragged_s16(lib, torch, streams33):
    n, avg = 256, 4
    lens = _ragged_lengths(avg, n)
    offs = [b * streams33[1].size(1) for b in range(len(lens))]
    flat = streams33[1].reshape(-1)
    sp = lmp(lib, n, avg, sub_mean=1, sample_format=lib.SAMPLES_S16)
    got, starts = sp.run_ragged(flat, offs, lens)
    for b, (o, m) in enumerate(zip(offs, lens)):
        assert same(got[starts[b]:starts[b + 1]], run_whole(sp, flat[o:o + m])), b


def test_more_streams_than_a_grid_dimension(lib, torch):
    """The batch kernels carry the stream in blockIdx.z (65 535 at most): 65 537 streams of two frames at N = 256 are cut into
    launches of 65 535 and 2.  The ragged kernels cannot meet such a limit: their streams are entries of one flat block list."""
    n, B, avg = 256, 65537, 4
    g = torch.Generator(device="cuda").manual_seed(7)
    xs = torch.randn((B, 2 * n), device="cuda", generator=g) * 0.2
    sp = lmp(lib, n, avg)
    got = sp.run_batch(xs)
    assert got.shape == (B, 2, 129)
    assert same(got[:65535], sp.run_batch(xs[:65535])) and same(got[65535:], sp.run_batch(xs[65535:]))
    for b in (0, 1, 65534, 65535, 65536):
        assert same(got[b], sp.run(xs[b])), b
    P = rect(lib, n).run_batch(xs)
    stage = lib.lmp_statistic_batch(P, avg)
    assert same(stage, got)
    starts = np.arange(B + 1) * 2
    packed, _ = lib.lmp_statistic_ragged(P.view(2 * B, 129), starts, avg)
    assert same(packed.view(B, 2, 129), got)


def test_scratch_chunks_leave_the_rows_unchanged(lib, torch, streams33):
    """glfer_hip_scratch_limit low enough that the 33 streams' periodograms go through scratch in four chunks (a chunk takes the
    streams whose rows fit half the cap: ten of them), and in chunks of one stream each"""
    xs = streams33[0]
    n, avg, L = 256, 4, lib.api.lib()
    lens = [xs.size(1) - (b % 5) * n for b in range(xs.size(0))]
    offs = [b * xs.size(1) for b in range(xs.size(0))]
    sp = lmp(lib, n, avg, sub_mean=1)
    want = sp.run_batch(xs, first_frame=3)
    want_r, starts = sp.run_ragged(xs.reshape(-1), offs, lens)
    stream_bytes = (xs.size(1) // n) * 129 * 4            # a stream's periodograms (first_frame = 3 recomputes its three frames back)
    try:
        for cap in (2 * 10 * stream_bytes + 64, stream_bytes):
            L.glfer_hip_scratch_limit(cap)
            assert same(sp.run_batch(xs, first_frame=3), want), cap
            got_r, st = sp.run_ragged(xs.reshape(-1), offs, lens)
            assert list(st) == list(starts) and same(got_r, want_r), cap
    finally:
        L.glfer_hip_scratch_limit(16 << 30)


def test_averaged_lmp_rows_batch_and_ragged(lib, torch, streams33):
    xs = streams33[0][:5]
    n, avg = 256, 4
    sp = lmp(lib, n, avg)
    a, r, p = sp.run_avg_batch(xs, lib.AVG_PLAIN, 4, 0, 129, want_psd=True)
    for b in range(xs.size(0)):
        a1, r1, p1 = sp.run_avg(xs[b], lib.AVG_PLAIN, 4, 0, 129, want_psd=True)
        assert same(p[b], p1), b
        assert torch.equal(a[b].view(torch.int64), a1.view(torch.int64)) and torch.equal(r[b].view(torch.int64), r1.view(torch.int64)), b
    lens = _ragged_lengths(avg, n)[:6]
    offs = [b * streams33[0].size(1) for b in range(len(lens))]
    flat = streams33[0].reshape(-1)
    a, r, p, starts = sp.run_avg_ragged(flat, offs, lens, lib.AVG_PLAIN, 4, 0, 129, want_psd=True)
    for b, (o, m) in enumerate(zip(offs, lens)):
        if m < n:
            assert starts[b] == starts[b + 1]
            continue
        a1, r1, p1 = sp.run_avg(flat[o:o + m], lib.AVG_PLAIN, 4, 0, 129, want_psd=True)
        rows = slice(int(starts[b]), int(starts[b + 1]))
        assert same(p[rows], p1), b
        assert torch.equal(a[rows].view(torch.int64), a1.view(torch.int64)) and torch.equal(r[rows].view(torch.int64), r1.view(torch.int64)), b
