"""HP-ARMA rows for many streams in one launch: run_batch, run_ragged and run_list on HP-ARMA plans.  A row is a function of its
frame's samples alone, so the contract is bit for bit: every row equals the row a loop of Spectrogram.run over the same memory
writes (torch.equal on the bits) and is finite.  run itself is held to the oracle by the parity tests; no oracle is needed here.
The last test times the batch call against the loop: one launch over all frames, not one launch per stream."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# (n, t, p_e, overlap, frames): the kernel's instantiations and paths
C5 = (4096, 128, 32, 0.0, 5)                 # BASELINE config 5: <128, 33>
DFLT = (1024, 96, 16, 0.5, 6)                # glfer's defaults: <96, 17>
SHAPES = {
    "c5": C5,
    "default": DFLT,
    "generic": (512, 64, 20, 0.5, 4),        # the scheduled sweep with the shape from the parameters
    "unscheduled": (2048, 160, 12, 0.0, 3),  # t > 128: rotation after rotation
    "smallest": (32, 8, 3, 0.0, 6),
    "largest": (32768, 128, 32, 0.0, 2),     # one frame in flight per CU
}
ENV = ("GLFER_HPARMA_WIDTH", "GLFER_HPARMA_GENERIC", "GLFER_HPARMA_LDS_KB")


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


@pytest.fixture(autouse=True)
def _product_kernels(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)


def plan(lib, shape, **k):
    n, t, p_e, overlap, _ = shape
    return lib.Spectrogram(lib.HparmaParams(n=n, overlap=overlap, t=t, p_e=p_e, **k))


def samples(torch, lib, fmt, count, seed):
    """`count` samples of the format: noise and two tones, so that the rows have peaks and every lag matters"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    i = torch.arange(count, device="cuda", dtype=torch.float32)
    x = 0.2 * torch.randn(count, device="cuda", generator=g) + 0.4 * torch.sin(0.3 * i + seed) + 0.2 * torch.sin(1.1 * i)
    if fmt == lib.SAMPLES_F32:
        return x
    if fmt == lib.SAMPLES_S16:
        return (x * 20000).round().clamp(-32768, 32767).to(torch.int16)
    return (x * 100 + 128).round().clamp(0, 255).to(torch.uint8)


def fill_value(lib, fmt):
    """what lies between the streams: a neighbour's sample read by mistake must show up in the rows"""
    return float("nan") if fmt == lib.SAMPLES_F32 else (32767 if fmt == lib.SAMPLES_S16 else 255)


def batch_with_gaps(torch, lib, fmt, B, T, gap, seed):
    """[B, T] streams with stride(0) = T + gap, the gaps (and a margin before the first stream) filled with fill_value"""
    pitch = T + gap
    buf = samples(torch, lib, fmt, gap + B * pitch, seed)
    xs = buf[gap:].view(B, pitch)[:, :T]
    if gap:
        buf[:gap] = fill_value(lib, fmt)
        buf[gap:].view(B, pitch)[:, T:] = fill_value(lib, fmt)
    return xs


def same(torch, a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def check_batch(torch, lib, sp, xs, first=0, nframes=None):
    got = sp.run_batch(xs, first_frame=first, nframes=nframes)
    assert bool(torch.isfinite(got).all())
    for b in range(xs.size(0)):
        want = sp.run(xs[b], first_frame=first, nframes=nframes)
        assert same(torch, got[b], want), (b, first, nframes)
    return got


def run_whole(torch, sp, v):
    return sp.run(v) if v.numel() >= sp.hop else torch.empty((0, sp.pitch), dtype=torch.float32, device=v.device)


def layout(torch, lib, fmt, lens, seed, gap=6):
    """the streams in one buffer at shuffled offsets with gaps between them (even offsets: the integer formats need them);
    the gaps hold fill_value"""
    order = np.random.default_rng(seed).permutation(len(lens))
    offs, at = [0] * len(lens), gap
    for b in order:
        offs[b] = at
        at += lens[b] + gap + ((lens[b] + gap) & 1)
    buf = torch.full((at,), fill_value(lib, fmt), device="cuda",
                     dtype={lib.SAMPLES_F32: torch.float32, lib.SAMPLES_S16: torch.int16, lib.SAMPLES_U8: torch.uint8}[fmt])
    x = samples(torch, lib, fmt, sum(lens) + 1, seed)
    used = 0
    for b, m in enumerate(lens):
        buf[offs[b]:offs[b] + m] = x[used:used + m]
        used += m
    return buf, offs


def check_ragged(torch, sp, buf, offs, lens):
    total, starts = sp.ragged_frames(lens)
    assert total == sum(m // sp.hop for m in lens)
    out = torch.full((total + 3, sp.pitch), -77.0, device="cuda")
    got, st = sp.run_ragged(buf, offs, lens, out=out)
    assert list(st) == list(starts)
    for b, (o, m) in enumerate(zip(offs, lens)):
        want = run_whole(torch, sp, buf[o:o + m])
        assert same(torch, out[int(starts[b]):int(starts[b + 1])], want), (b, m // sp.hop)
    assert bool(torch.isfinite(out[:total]).all())
    assert bool((out[total:] == -77.0).all())                     # nothing past the last stream's rows
    return out[:total], starts


# ---- batch equals loop
@pytest.mark.parametrize("name", list(SHAPES))
def test_batch_equals_loop(lib, torch, name):
    shape = SHAPES[name]
    sp = plan(lib, shape)
    xs = batch_with_gaps(torch, lib, lib.SAMPLES_F32, 3, shape[4] * sp.hop + 5, 0, 1)
    got = check_batch(torch, lib, sp, xs)
    assert got.shape == (3, shape[4], sp.bins)


@pytest.mark.parametrize("opts", [dict(sub_mean=1), dict(sub_mean=2), dict(history_mode=1), dict(sub_mean=1, history_mode=1)],
                         ids=["sub_mean1", "sub_mean2", "history1", "sub_mean1_history1"])
@pytest.mark.parametrize("name", ["c5", "default"])
def test_batch_mean_removal_and_history_mode(lib, torch, name, opts):
    shape = SHAPES[name]
    sp = plan(lib, shape, **opts)
    check_batch(torch, lib, sp, batch_with_gaps(torch, lib, lib.SAMPLES_F32, 3, shape[4] * sp.hop + 5, 0, 2))


@pytest.mark.parametrize("sub_mean", [0, 1])
@pytest.mark.parametrize("fmt", ["s16", "u8"])
@pytest.mark.parametrize("name", ["c5", "default"])
def test_batch_integer_samples(lib, torch, name, fmt, sub_mean):
    shape = SHAPES[name]
    f = lib.SAMPLES_S16 if fmt == "s16" else lib.SAMPLES_U8
    sp = plan(lib, shape, sample_format=f, sub_mean=sub_mean)
    check_batch(torch, lib, sp, batch_with_gaps(torch, lib, f, 3, shape[4] * sp.hop + 6, 0, 3))


@pytest.mark.parametrize("name,B", [("c5", 1), ("c5", 2), ("default", 1), ("default", 2), ("default", 300)])
def test_batch_sizes(lib, torch, name, B):
    shape = SHAPES[name]
    sp = plan(lib, shape)
    frames = 2 if B == 300 else shape[4]
    check_batch(torch, lib, sp, batch_with_gaps(torch, lib, lib.SAMPLES_F32, B, frames * sp.hop + 1, 0, 4))


@pytest.mark.parametrize("sub_mean", [0, 1])
@pytest.mark.parametrize("name", ["c5", "default"])
def test_first_frame_inside_the_stream(lib, torch, name, sub_mean):
    shape = SHAPES[name]
    sp = plan(lib, shape, sub_mean=sub_mean)
    total = 8
    xs = batch_with_gaps(torch, lib, lib.SAMPLES_F32, 3, total * sp.hop + 3, 0, 5)
    got = check_batch(torch, lib, sp, xs, first=2, nframes=total - 3)
    whole = sp.run_batch(xs)
    assert same(torch, got, whole[:, 2:total - 1])               # the same frames of a call over the whole streams


@pytest.mark.parametrize("sub_mean", [0, 1])
@pytest.mark.parametrize("fmt", ["f32", "s16", "u8"])
@pytest.mark.parametrize("name", ["c5", "default"])
def test_gaps_between_streams(lib, torch, name, fmt, sub_mean):
    """stride(0) = T + 2 N + 6 with NaN (f32) or full scale (s16, u8) in the gaps: the rows show a read of the neighbour"""
    shape = SHAPES[name]
    f = {"f32": lib.SAMPLES_F32, "s16": lib.SAMPLES_S16, "u8": lib.SAMPLES_U8}[fmt]
    sp = plan(lib, shape, sample_format=f, sub_mean=sub_mean)
    T = shape[4] * sp.hop + 2
    xs = batch_with_gaps(torch, lib, f, 3, T, 2 * sp.n + 6, 6)
    assert xs.stride(0) == T + 2 * sp.n + 6
    got = check_batch(torch, lib, sp, xs)
    dense = sp.run_batch(xs.contiguous())                        # the same samples without the gaps
    assert same(torch, got, dense)


@pytest.mark.parametrize("name", ["c5", "default"])
def test_row_pitch_and_sentinel(lib, torch, name):
    shape = SHAPES[name]
    dense = plan(lib, shape)
    pitch = dense.bins + 7
    sp = plan(lib, shape, psd_pitch=pitch)
    assert sp.pitch == pitch and sp.bins == dense.bins
    xs = batch_with_gaps(torch, lib, lib.SAMPLES_F32, 3, shape[4] * sp.hop, 0, 7)
    out = torch.full((3, shape[4], pitch), -77.0, device="cuda")
    got = sp.run_batch(xs, out=out)
    assert got is out
    for b in range(3):
        assert same(torch, out[b, :, :sp.bins], dense.run(xs[b])), b
        assert same(torch, out[b, :, :sp.bins], sp.run(xs[b])[:, :sp.bins]), b
    assert bool((out[:, :, sp.bins:] == -77.0).all())
    lens = [2 * sp.hop, sp.hop - 1, 3 * sp.hop + 5]
    buf, offs = layout(torch, lib, lib.SAMPLES_F32, lens, 8)
    rows = torch.full((5, pitch), -77.0, device="cuda")
    sp.run_ragged(buf, offs, lens, out=rows)
    assert same(torch, rows[:2, :sp.bins], dense.run(buf[offs[0]:offs[0] + lens[0]]))
    assert same(torch, rows[2:, :sp.bins], dense.run(buf[offs[2]:offs[2] + lens[2]]))
    assert bool((rows[:, sp.bins:] == -77.0).all())


# ---- the queue
@pytest.fixture(scope="module")
def queue_streams(lib, torch):
    """48 streams of 48 frames at C5: 2 304 frames, more than the 1 792 a launch keeps in flight; and the loop's rows"""
    sp = plan(lib, C5)
    xs = batch_with_gaps(torch, lib, lib.SAMPLES_F32, 48, 96 * sp.hop, 0, 9)    # 96 frames of samples a stream: the ragged run's longest
    want = torch.stack([sp.run(xs[b]) for b in range(48)])
    torch.cuda.synchronize()
    return sp, xs, want


def test_queue_across_stream_boundaries_batch(lib, torch, queue_streams):
    sp, xs, want = queue_streams
    got = sp.run_batch(xs[:, :48 * sp.hop])
    assert got.shape == (48, 48, sp.bins) and 48 * 48 > 1792
    assert same(torch, got, want[:, :48]) and bool(torch.isfinite(got).all())


def test_queue_across_stream_boundaries_ragged(lib, torch, queue_streams):
    sp, xs, want = queue_streams
    frames = list(range(1, 97, 2))
    frames[-1] = 96
    frames = [frames[i] for i in np.random.default_rng(3).permutation(48)]
    assert len(frames) == 48 and min(frames) == 1 and max(frames) == 96 and sum(frames) > 1792
    lens = [f * sp.hop + (b % 5) for b, f in enumerate(frames)]
    lens = [min(m, xs.size(1)) for m in lens]
    offs = [b * xs.stride(0) for b in range(48)]
    got, starts = sp.run_ragged(xs.reshape(-1), offs, lens)
    assert bool(torch.isfinite(got).all())
    for b, f in enumerate(frames):
        assert same(torch, got[int(starts[b]):int(starts[b + 1])], want[b, :f]), (b, f)


# ---- ragged equals loop
def _lens(H):
    base = [2 * H, H - 1, 3 * H + 5, 0, H, 7 * H + 3]
    # empty and sub-hop streams first, last and next to each other
    edges = [0, H - 1, 2 * H, 3 * H + 5, 0, 0, H - 1, H, 7 * H + 3, H - 1, 0]
    return base, edges


@pytest.mark.parametrize("opts", [dict(), dict(sub_mean=1), dict(sub_mean=2), dict(history_mode=1), dict(sub_mean=1, history_mode=1)],
                         ids=["plain", "sub_mean1", "sub_mean2", "history1", "sub_mean1_history1"])
@pytest.mark.parametrize("name", ["c5", "default"])
def test_ragged_equals_loop(lib, torch, name, opts):
    sp = plan(lib, SHAPES[name], **opts)
    for k, lens in enumerate(_lens(sp.hop)):
        buf, offs = layout(torch, lib, lib.SAMPLES_F32, lens, 10 + k)
        check_ragged(torch, sp, buf, offs, lens)


@pytest.mark.parametrize("sub_mean", [0, 1])
@pytest.mark.parametrize("name", ["c5", "default"])
def test_ragged_s16_at_even_offsets(lib, torch, name, sub_mean):
    sp = plan(lib, SHAPES[name], sample_format=lib.SAMPLES_S16, sub_mean=sub_mean)
    for k, lens in enumerate(_lens(sp.hop)):
        buf, offs = layout(torch, lib, lib.SAMPLES_S16, lens, 20 + k)
        assert all(o % 2 == 0 for o in offs)
        check_ragged(torch, sp, buf, offs, lens)


@pytest.mark.parametrize("sub_mean", [0, 1])
@pytest.mark.parametrize("name", ["c5", "default"])
def test_ragged_many_short_streams(lib, torch, name, sub_mean):
    """300 streams of 1 .. 3 frames: the bisection over a table of 300 entries"""
    sp = plan(lib, SHAPES[name], sub_mean=sub_mean)
    lens = [(1 + (b * 5) % 3) * sp.hop + (b % 7) for b in range(300)]
    buf, offs = layout(torch, lib, lib.SAMPLES_F32, lens, 30, gap=2)
    check_ragged(torch, sp, buf, offs, lens)


@pytest.mark.parametrize("name", ["c5", "default"])
def test_ragged_one_long_stream_among_short(lib, torch, name):
    """one stream of 2 000 frames -- alone more than a grid -- among 36 streams of at most 4"""
    sp = plan(lib, SHAPES[name])
    lens = [(b % 5) * sp.hop + (b % 3) for b in range(36)]
    lens.insert(17, 2000 * sp.hop + 9)
    buf, offs = layout(torch, lib, lib.SAMPLES_F32, lens, 31)
    check_ragged(torch, sp, buf, offs, lens)


@pytest.mark.parametrize("sub_mean", [0, 1])
@pytest.mark.parametrize("name", ["c5", "default"])
def test_ragged_streams_that_overlap_in_memory(lib, torch, name, sub_mean):
    sp = plan(lib, SHAPES[name], sub_mean=sub_mean)
    H = sp.hop
    buf = samples(torch, lib, lib.SAMPLES_F32, 9 * H, 32)
    offs, lens = [0, 2 * H + 3, 2 * H + 3], [5 * H, 6 * H, 3 * H]   # the second starts inside the first; the third is its head
    check_ragged(torch, sp, buf, offs, lens)


@pytest.mark.parametrize("name", ["c5", "default"])
def test_run_list_and_one_stream_alone(lib, torch, name):
    sp = plan(lib, SHAPES[name], sub_mean=1)
    H = sp.hop
    streams = [samples(torch, lib, lib.SAMPLES_F32, m, 40 + k) for k, m in enumerate([3 * H + 1, H - 1, 5 * H, 2 * H + 7])]
    listed = sp.run_list(streams)
    for b, v in enumerate(streams):
        assert same(torch, listed[b], run_whole(torch, sp, v)), b
    one = streams[2]
    got, starts = sp.run_ragged(one, [0], [one.numel()])
    assert list(starts) == [0, 5] and same(torch, got, sp.run(one))
    assert same(torch, sp.run_batch(one.view(1, -1))[0], sp.run(one))


# ---- GLFER_HPARMA_WIDTH=16: a single-stream kernel, its batches stay the loop
def _child():
    import torch
    import glfer_amd as lib
    for shape in (C5, DFLT):
        sp = plan(lib, shape)
        xs = batch_with_gaps(torch, lib, lib.SAMPLES_F32, 3, shape[4] * sp.hop + 5, 2 * sp.n + 6, 50)
        check_batch(torch, lib, sp, xs)
        lens = _lens(sp.hop)[0]
        buf, offs = layout(torch, lib, lib.SAMPLES_F32, lens, 51)
        check_ragged(torch, sp, buf, offs, lens)
    torch.cuda.synchronize()
    print("width16 ok")


def test_width16_batches_keep_the_loop():
    """the variable is read once per process: a fresh child"""
    env = {k: v for k, v in os.environ.items() if k not in ENV}
    env["GLFER_HPARMA_WIDTH"] = "16"
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "width16 ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


# ---- one launch, not B launches
def test_one_launch_not_one_per_stream(lib, torch):
    """256 streams of 2 frames at C5, f32.  The loop is 256 launches one after another, each no shorter than a frame's latency;
    the batch is 512 frames -- fewer than the 1 792 in flight -- so one frame's latency plus a launch: the ideal ratio is about
    256, and 8 leaves a thirty-fold margin for launch overhead and a busy machine.  (Where the batch call is the loop itself the
    ratio is about 1.)"""
    sp = plan(lib, C5)
    B = 256
    xs = batch_with_gaps(torch, lib, lib.SAMPLES_F32, B, 2 * sp.hop, 0, 60)
    out = torch.empty((B, 2, sp.bins), device="cuda")
    views = [xs[b] for b in range(B)]

    def batch():
        sp.run_batch(xs, out=out)

    def loop():
        for b in range(B):
            sp.run(views[b], out=out[b])

    def once(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    times = {}
    for name, fn in (("batch", batch), ("loop", loop)):
        fn()                                                     # one warm-up each
        torch.cuda.synchronize()
        times[name] = sorted(once(fn) for _ in range(5))[2]      # the median of five
    ratio = times["loop"] / times["batch"]
    print("C5, 256 streams x 2 frames: run_batch %.3f ms, loop of run %.3f ms, loop / batch x%.1f" % (times["batch"], times["loop"], ratio))
    assert times["loop"] >= 8 * times["batch"], (times, ratio)


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    _child()
