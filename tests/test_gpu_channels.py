"""Multi-channel recordings (-m gpu): every interleaved channel as a stream of its own.

The de-interleave kernel against torch indexing; Spectrogram.run_channels against Spectrogram.run on a contiguous copy of each
channel; the host and file entries against Spectrogram.run_host on the numpy-extracted channel.  Every comparison is exact
(torch.equal / np.array_equal on the bits): the kernel moves bytes, and the rows are the single-stream entry's by contract.

The channels of a recording differ -- a signal on a DC level, a silent channel, another signal -- so that a channel mix-up, a
history read from the neighbour or a mean taken over the wrong samples cannot come out equal.
"""
import ctypes as C
import wave

import numpy as np
import pytest

from _signals import synth
from test_channels_host import plan_argument_checks

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def same(torch, a, b):
    """bit for bit (NaN rows of a silent channel included)"""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ---- the kernel alone ---------------------------------------------------------------------------------------------------------

def _selections(c):
    return [None, [c - 1], list(range(c))[::-1], [0, c - 1, 0]]


@pytest.mark.parametrize("fmt", ["f32", "s16", "u8"])
def test_deinterleave_against_torch_indexing(lib, torch, fmt):
    """C in {1, 2, 3, 4, 5, 8, 64}; select = all / one channel / reversed / with a duplicate; S in {0, 1, 7, 64, 1000, 4099}; the
    source and the destination at an aligned base and one element off it (the stereo form runs only where both allow it, the
    general form everywhere else); planes S apart and padded; the padding, the element in front and a guard region after the
    last plane keep their bytes.  The samples are random BITS of the sample's width (every float pattern included) and are compared as
    integers: the kernel must move them, not convert them."""
    idt = {"f32": torch.int32, "s16": torch.int16, "u8": torch.uint8}[fmt]
    sdt = {"f32": torch.float32, "s16": torch.int16, "u8": torch.uint8}[fmt]
    g = torch.Generator(device="cuda").manual_seed(7)
    lo, hi = {"f32": (-2 ** 31, 2 ** 31 - 1), "s16": (-2 ** 15, 2 ** 15 - 1), "u8": (0, 255)}[fmt]
    GUARD = 64
    ran = 0
    for c in (1, 2, 3, 4, 5, 8, 64):
        for s in (0, 1, 7, 64, 1000, 4099):
            src = torch.randint(lo, hi + 1, (s * c + 1,), device="cuda", generator=g, dtype=torch.int64).to(idt)
            for sel in _selections(c):
                idx = list(range(c)) if sel is None else sel
                for src_off, dst_off, pad in ((0, 0, 0), (0, 0, 8), (1, 0, 0), (0, 1, 8), (1, 1, 5)):
                    x = src[src_off:src_off + s * c]
                    pitch = s + pad
                    buf = torch.randint(lo, hi + 1, (1 + len(idx) * pitch + GUARD,), device="cuda", generator=g, dtype=torch.int64).to(idt)
                    want = buf.clone()
                    planes = want[dst_off:dst_off + len(idx) * pitch].view(len(idx), pitch)
                    planes[:, :s] = x.view(s, c)[:, idx].t()
                    out = buf[dst_off:dst_off + len(idx) * pitch].view(len(idx), pitch)[:, :s]
                    got = lib.deinterleave(x.view(sdt), c, sel, out=out.view(sdt))
                    assert got.data_ptr() == out.data_ptr()
                    assert torch.equal(buf, want), (c, s, sel, src_off, dst_off, pad)
                    ran += 1
    assert ran == 7 * 6 * 4 * 5
    # the allocating form, and a [S][C] tensor
    x = torch.randint(lo, hi + 1, (1000, 2), device="cuda", generator=g, dtype=torch.int64).to(idt)
    got = lib.deinterleave(x.view(sdt), 2)
    assert got.shape == (2, 1000) and torch.equal(got.view(idt), x.t().contiguous())


def test_deinterleave_replays_from_a_captured_graph(lib, torch):
    """the selection rides in the kernel's arguments -- no table is uploaded -- so the launch is legal under capture, and a
    replay moves the bytes the source holds THEN"""
    L = lib.api.lib()
    S, Cn = 4099, 2
    x = torch.zeros(S * Cn, dtype=torch.int16, device="cuda")
    out = torch.zeros((2, S + 5), dtype=torch.int16, device="cuda")
    sel = (C.c_int * 2)(1, 0)

    def call(stream):
        return L.glfer_hip_deinterleave_device(x.data_ptr(), S, Cn, lib.SAMPLES_S16, sel, 2, out.data_ptr(), S + 5, C.c_void_p(stream.cuda_stream))

    assert call(torch.cuda.current_stream()) == 0                      # (the module is loaded outside the capture)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        rc = call(torch.cuda.current_stream())
    assert rc == 0
    g = torch.Generator(device="cuda").manual_seed(11)
    for _ in range(2):
        x.copy_(torch.randint(-2 ** 15, 2 ** 15, (S * Cn,), device="cuda", generator=g, dtype=torch.int64).to(torch.int16))
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out[:, :S], x.view(S, Cn)[:, [1, 0]].t())
        assert not bool(out[:, S:].any())


# ---- rows ------------------------------------------------------------------------------------------------------------------------

def recording(torch, lib, fmt, s, c, seed=0):
    """[s][c] numpy recording of the plan's sample type: channel 0 a signal on a DC level, channel 1 silent, the others signals
    of their own (for c == 2: the DC channel and a signal -- the silent channel is in every three-channel case)"""
    chans = []
    for k in range(c):
        if k == 0:
            chans.append(0.5 * synth(s, seed=seed + 1).astype(np.float64) + 0.3)
        elif k == 1 and c > 2:
            chans.append(np.zeros(s))
        else:
            chans.append(0.8 * synth(s, seed=seed + 10 + k, f0=400.0 * (k + 1), f1=5100.5).astype(np.float64) - 0.02 * k)
    x = np.stack(chans, axis=1)
    if fmt == lib.SAMPLES_F32:
        return np.ascontiguousarray(x.astype(np.float32))
    if fmt == lib.SAMPLES_S16:
        return np.ascontiguousarray(np.clip(np.round(x * 30000.0), -32768, 32767).astype(np.int16))
    return np.ascontiguousarray(np.clip(np.round(x * 120.0 + 128.0), 0, 255).astype(np.uint8))


def _plans(lib):
    F, M, H, Lp = lib.FftParams, lib.MtmParams, lib.HparmaParams, lib.LmpParams
    f32, s16, u8 = lib.SAMPLES_F32, lib.SAMPLES_S16, lib.SAMPLES_U8
    ZA = lib.HISTORY_ZERO_ALWAYS
    return {
        # the smallest one-launch batch size, and the stream-by-stream route below it
        "fft256-f32": (F(n=256, window_type=0, overlap=0.5, sample_format=f32), 3),
        "fft256-s16-mean1": (F(n=256, window_type=0, overlap=0.5, sub_mean=1, sample_format=s16), 2),
        "fft256-u8-mean2": (F(n=256, window_type=0, overlap=0.5, sub_mean=2, sample_format=u8), 3),
        "fft64-u8-mean2-za": (F(n=64, window_type=0, overlap=0.5, sub_mean=2, history_mode=ZA, sample_format=u8), 3),
        "fft64-f32-mean1": (F(n=64, window_type=0, overlap=0.5, sub_mean=1, sample_format=f32), 2),
        # multitaper: five tapers at N = 4096 (the 32-frame groups), eight at N = 1024 and 75 % overlap
        "mtm4096k5-s16": (M(n=4096, overlap=0.0, w=2.5, kmax=4, sample_format=s16), 2),
        "mtm4096k5-f32-mean1-pitch": (M(n=4096, overlap=0.0, w=2.5, kmax=4, sub_mean=1, sample_format=f32, psd_pitch=2112), 3),
        "mtm4096k5-u8-mean2-za": (M(n=4096, overlap=0.0, w=2.5, kmax=4, sub_mean=2, history_mode=ZA, sample_format=u8), 2),
        "mtm1024k8-s16-mean1": (M(n=1024, overlap=0.75, w=4.0, kmax=7, sub_mean=1, sample_format=s16), 3),
        "mtm1024k8-f32-za": (M(n=1024, overlap=0.75, w=4.0, kmax=7, history_mode=ZA, sample_format=f32), 2),
        "mtm1024k8-u8-mean2": (M(n=1024, overlap=0.75, w=4.0, kmax=7, sub_mean=2, sample_format=u8), 2),
        # LMP: the ring reaches lmp_av - 1 frames further back
        "lmp256-s16-mean1": (Lp(n=256, overlap=0.5, avg=4, sub_mean=1, sample_format=s16), 3),
        "lmp256-f32": (Lp(n=256, overlap=0.5, avg=4, sample_format=f32), 2),
        "lmp256-u8-mean2-za": (Lp(n=256, overlap=0.5, avg=4, sub_mean=2, history_mode=ZA, sample_format=u8), 2),
        # HP-ARMA: one launch over the flat list of all channels' frames (stereo: its rows of a silent channel are no test)
        "hparma256-f32-mean1": (H(n=256, overlap=0.5, t=64, p_e=12, sub_mean=1, sample_format=f32), 2),
        "hparma256-s16": (H(n=256, overlap=0.0, t=64, p_e=12, sample_format=s16), 2),
        "hparma256-u8-mean2-za": (H(n=256, overlap=0.5, t=64, p_e=12, sub_mean=2, history_mode=ZA, sample_format=u8), 2),
    }


PLAN_NAMES = ["fft256-f32", "fft256-s16-mean1", "fft256-u8-mean2", "fft64-u8-mean2-za", "fft64-f32-mean1", "mtm4096k5-s16",
              "mtm4096k5-f32-mean1-pitch", "mtm4096k5-u8-mean2-za", "mtm1024k8-s16-mean1", "mtm1024k8-f32-za", "mtm1024k8-u8-mean2",
              "lmp256-s16-mean1", "lmp256-f32", "lmp256-u8-mean2-za", "hparma256-f32-mean1", "hparma256-s16", "hparma256-u8-mean2-za"]


@pytest.mark.parametrize("name", PLAN_NAMES)
def test_run_channels_equals_run_on_each_channel(lib, torch, name):
    params, c = _plans(lib)[name]
    sp = lib.Spectrogram(params)
    try:
        hop = sp.hop
        s = 40 * hop + hop // 3 + 1                                   # 40 hops and a ragged remainder
        x = torch.from_numpy(recording(torch, lib, params.sample_format, s, c)).cuda()
        halo = -(-(sp.n - hop) // hop) + (params.avg - 1 if params.mode == lib.MODE_LMP else 0)
        refs = [sp.run(x[:, k].contiguous()) for k in range(c)]       # computed once per plan
        assert refs[0].shape == (40, sp.pitch)
        assert not same(torch, refs[0][:, :sp.bins], refs[c - 1][:, :sp.bins])
        # whole recording, every channel, from the [S][C] tensor
        got = sp.run_channels(x)
        assert got.shape == (c, 40, sp.pitch)
        for k in range(c):
            assert same(torch, got[k][:, :sp.bins], refs[k][:, :sp.bins]), (name, k)
        # a selection (reversed, with a duplicate) of a frame range that starts past the halo and stops short of the end, from
        # the flat tensor, against run() over the SAME frames (the contract; a range cut off the multiples of GLFER_FRAME_ALIGN
        # equals the one-shot rows only to rounding, "Cutting a stream"); the floats between the bins and the pitch are not written
        sel = list(range(c))[::-1] + [0]
        first, nframes = halo + 2, 40 - (halo + 2) - 3
        part = [sp.run(x[:, k].contiguous(), first_frame=first, nframes=nframes) for k in range(c)]
        out = torch.full((len(sel), nframes, sp.pitch), -7.0, dtype=torch.float32, device="cuda")
        got = sp.run_channels(x.reshape(-1), channels=c, select=sel, first_frame=first, nframes=nframes, out=out)
        for j, k in enumerate(sel):
            assert same(torch, got[j][:, :sp.bins], part[k][:, :sp.bins]), (name, j, k)
        assert bool((out[:, :, sp.bins:] == -7.0).all())
        # one channel of several: the batch of one stream
        got = sp.run_channels(x, select=[c - 1], first_frame=1, nframes=5)
        assert same(torch, got[0][:, :sp.bins], sp.run(x[:, c - 1].contiguous(), first_frame=1, nframes=5)[:, :sp.bins]), name
    finally:
        sp.close()


def test_one_channel_is_the_single_stream_entry(lib, torch):
    sp = lib.Spectrogram(lib.FftParams(n=256, window_type=0, overlap=0.5, sub_mean=1, sample_format=lib.SAMPLES_S16))
    x = torch.from_numpy(recording(torch, lib, lib.SAMPLES_S16, 40 * sp.hop + 9, 1)).cuda()
    want = sp.run(x.reshape(-1))
    assert same(torch, sp.run_channels(x)[0], want)
    assert same(torch, sp.run_channels(x.reshape(-1), channels=1)[0], want)
    got = sp.run_channels(x, select=[0, 0])                            # a selection of the one channel goes through the planes
    assert same(torch, got[0], want) and same(torch, got[1], want)
    sp.close()


def test_pieces_leave_the_rows_unchanged(lib, torch):
    """glfer_hip_scratch_limit so low that the planes of a 200-frame stereo call take several times half the cap: the call runs
    in pieces of 64 and of 32 frames (the minimum), each with its own halo.  Five tapers at N = 4096: the 32-frame groups of
    that kernel are what a cut off the grid would break.  Also from a first frame off the grid."""
    L = lib.api.lib()
    sp = lib.Spectrogram(lib.MtmParams(n=4096, overlap=0.0, w=2.5, kmax=4, sub_mean=1, sample_format=lib.SAMPLES_S16))
    x = torch.from_numpy(recording(torch, lib, lib.SAMPLES_S16, 200 * sp.hop + 77, 2)).cuda()
    want = sp.run_channels(x)
    for k in range(2):
        assert same(torch, want[k], sp.run(x[:, k].contiguous())), k
    want5 = sp.run_channels(x, first_frame=5, nframes=190)
    for k in range(2):
        assert same(torch, want5[k], sp.run(x[:, k].contiguous(), first_frame=5, nframes=190)), k
    plane_bytes_70 = 2 * 70 * sp.hop * 2                               # two planes of 70 hops of s16: pieces of 64 frames
    try:
        for cap, least in ((2 * plane_bytes_70, 4), (4096, 7)):
            L.glfer_hip_scratch_limit(cap)
            # (the piece count the cap implies: the arithmetic itself is walked in tests/test_channels_host.py)
            per = max(32, (cap // 2 // (2 * sp.hop * 2)) // 32 * 32)
            assert -(-200 // per) >= least >= 3
            assert same(torch, sp.run_channels(x), want), cap
            assert same(torch, sp.run_channels(x, first_frame=5, nframes=190), want5), cap
    finally:
        L.glfer_hip_scratch_limit(16 << 30)
    sp.close()


def test_plan_argument_errors_where_a_plan_exists(lib, torch, tmp_path):
    L = lib.api.lib()
    cfg = lib.api.make_config(lib.FftParams(n=1024, window_type=0, overlap=0.5, sample_format=lib.SAMPLES_S16))
    h = C.c_void_p()
    assert L.glfer_hip_plan_create(C.byref(cfg), C.byref(h)) == 0
    try:
        plan_argument_checks(lib, h, tmp_path)
    finally:
        L.glfer_hip_plan_destroy(h)


# ---- host memory and files -------------------------------------------------------------------------------------------------------

def _write_wav(path, x, extra=b""):
    """x: [S][C] int16 or uint8"""
    with wave.open(str(path), "wb") as w:
        w.setnchannels(x.shape[1])
        w.setsampwidth(x.dtype.itemsize)
        w.setframerate(48000)
        w.writeframes(x.tobytes() + extra)


def test_stereo_16_bit_file_and_host_entries(lib, torch, tmp_path):
    sp = lib.Spectrogram(lib.FftParams(n=256, window_type=0, overlap=0.5, sub_mean=1, sample_format=lib.SAMPLES_S16))
    hop = sp.hop
    x = recording(torch, lib, lib.SAMPLES_S16, 100 * hop + 37, 2)
    path = tmp_path / "stereo.wav"
    _write_wav(path, x, extra=b"\x01\x02\x03")                        # ends in an incomplete sample frame
    refs = [sp.run_host(np.ascontiguousarray(x[:, k])) for k in range(2)]
    assert refs[0].shape == (100, sp.bins) and not np.array_equal(refs[0], refs[1])
    # several chunks (the halo comes from the previous chunk's pinned buffer), and the default chunk
    for chunk in (32, 0):
        got = sp.run_wav_channels(path, chunk_frames=chunk)
        assert got.shape == (2, 100, sp.bins)
        for k in range(2):
            assert np.array_equal(got[k].view(np.int32), refs[k].view(np.int32)), (chunk, k)
    # one channel; max_frames clips, and the planes lie max_frames apart
    got = sp.run_wav_channels(path, select=[1], chunk_frames=32)
    assert got.shape == (1, 100, sp.bins) and np.array_equal(got[0].view(np.int32), refs[1].view(np.int32))
    got = sp.run_wav_channels(path, select=[1, 0, 1], chunk_frames=32, max_frames=70)
    assert got.shape == (3, 70, sp.bins)
    for j, k in enumerate((1, 0, 1)):
        assert np.array_equal(got[j].view(np.int32), refs[k][:70].view(np.int32)), j
    # host memory: pageable, rows into pinned memory, samples from pinned memory
    for pinned in (False, True):
        got = sp.run_host_channels(x, 2, pinned=pinned)
        assert got.shape == (2, 100, sp.bins)
        for k in range(2):
            assert np.array_equal(np.asarray(got[k]).view(np.int32), refs[k].view(np.int32)), (pinned, k)
    xp = lib.pinned_empty(x.shape, x.dtype)
    xp[...] = x
    got = sp.run_host_channels(xp, 2, select=[1, 0])
    assert np.array_equal(got[0].view(np.int32), refs[1].view(np.int32)) and np.array_equal(got[1].view(np.int32), refs[0].view(np.int32))
    # the single-stream file entry keeps its meaning: the interleaved samples as ONE stream
    flat = x.reshape(-1)
    one = sp.run_wav(path)
    assert one.shape == ((flat.size + 1) // hop, sp.bins)              # (the stray bytes hold one more sample)
    assert np.array_equal(one[:flat.size // hop].view(np.int32), sp.run_host(flat).view(np.int32))
    sp.close()


def test_three_channel_8_bit_file_through_an_lmp_plan(lib, torch, tmp_path):
    """LMP: the chunk's halo is the longer one (the ring's lmp_av - 1 frames on top of the history)"""
    sp = lib.Spectrogram(lib.LmpParams(n=256, overlap=0.5, avg=4, sub_mean=1, sample_format=lib.SAMPLES_U8))
    hop = sp.hop
    x = recording(torch, lib, lib.SAMPLES_U8, 100 * hop + 50, 3)
    path = tmp_path / "three.wav"
    _write_wav(path, x, extra=b"\x80\x81")                            # two of the three samples of one more sample frame
    refs = [sp.run_host(np.ascontiguousarray(x[:, k])) for k in range(3)]
    for chunk in (32, 0):
        got = sp.run_wav_channels(path, chunk_frames=chunk)
        assert got.shape == (3, 100, sp.bins)
        for k in range(3):
            assert np.array_equal(got[k].view(np.int32), refs[k].view(np.int32)), (chunk, k)
    got = sp.run_host_channels(x.reshape(-1), 3, select=[2, 2, 1])
    for j, k in enumerate((2, 2, 1)):
        assert np.array_equal(got[j].view(np.int32), refs[k].view(np.int32)), j
    sp.close()
