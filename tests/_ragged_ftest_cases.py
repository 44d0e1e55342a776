"""Shared by tests/test_ragged_ftest_host.py and tests/test_gpu_ragged_ftest.py: the stream layout and the length list of the
ragged rows tests (copied from test_gpu_ragged.py, which is a test module and is not imported), and the argument rules of
glfer_hip_mtm_ftest_ragged_device / glfer_hip_mtm_rows_ftest_ragged_device, one assertion per rule, for whoever can make a plan."""
import numpy as np

from _signals import synth

E_ARG = -1
ENTRIES = ("glfer_hip_mtm_ftest_ragged_device", "glfer_hip_mtm_rows_ftest_ragged_device")
METHODS = ("ftest_ragged", "rows_ftest_ragged", "ftest_list", "rows_ftest_list")


def layout(torch, lib, fmt, lengths, gap=5, seed=7):
    """One device buffer that holds streams of these lengths (samples) in a shuffled order, `gap` or gap + 1 fill samples
    in front of each (f32: odd and even offsets alike; s16 / u8: even offsets only); the fill is NaN (f32) or full scale.
    The streams differ in seed, amplitude and DC level.  Returns (tensor, offsets)."""
    order = np.random.RandomState(seed).permutation(len(lengths))
    offs, at = [0] * len(lengths), 0
    for b in order:
        at += gap + (b & 1)
        if fmt != lib.SAMPLES_F32:
            at += at & 1
        offs[b] = at
        at += lengths[b]
    at += gap
    if fmt == lib.SAMPLES_F32:
        buf = np.full(at, np.nan, np.float32)
    elif fmt == lib.SAMPLES_S16:
        buf = np.full(at, 32767, np.int16)
    else:
        buf = np.full(at, 255, np.uint8)
    for b, n in enumerate(lengths):
        amp = 0.4 + 0.6 * ((b * 7919) % 11) / 10.0
        dc = 0.05 * (((b * 104729) % 9) - 4)
        x = amp * synth(max(n, 1), seed=2000 + b)[:n] + dc
        if fmt == lib.SAMPLES_S16:
            x = np.clip(np.round(x * 20000.0), -32768, 32767)
        elif fmt == lib.SAMPLES_U8:
            x = np.clip(np.round(128.0 + x * 90.0), 0, 255)
        buf[offs[b]:offs[b] + n] = x.astype(buf.dtype)
    return torch.from_numpy(buf).to("cuda:0"), offs


def lengths(n, hop, cap=None):
    """In samples: 0 frames (hop - 1 samples), 1, 2, 3, first_inside - 1, first_inside, first_inside + 1, 7 (+ hop / 2 spare
    samples), 40, 41 frames -- shuffled by a fixed seed, the longest neither first nor last."""
    fi = -(-(n - hop) // hop)
    frames = [1, 2, 3, max(fi - 1, 0), fi, fi + 1, 40, 41]
    if cap is not None:
        frames = [min(f, cap) for f in frames]
    lens = [hop - 1] + [f * hop for f in frames] + [min(7, cap or 7) * hop + hop // 2]
    rs = np.random.RandomState(11)
    while True:
        lens = [lens[i] for i in rs.permutation(len(lens))]
        top = int(np.argmax(lens))
        if 0 < top < len(lens) - 1:
            return lens


def call(L, rows, h, samples, nstreams, offs, lens, psd, ft, starts, mu_live=1, stream=None):
    """either entry with numpy arrays (or None) for the host arguments and raw pointers (or None) for the device ones"""
    ptr = lambda a: None if a is None else a.ctypes.data
    if rows:
        return L.glfer_hip_mtm_rows_ftest_ragged_device(h, samples, nstreams, ptr(offs), ptr(lens), psd, ft, mu_live, ptr(starts), stream)
    return L.glfer_hip_mtm_ftest_ragged_device(h, samples, nstreams, ptr(offs), ptr(lens), ft, mu_live, ptr(starts), stream)


def argument_rules(lib, plan):
    """Rules 1-8 of include/glfer_hip.h, in their order, for both entries.  plan(params) -> a plan handle (the caller owns it).
    No device memory is involved: every call here must return before it touches a device."""
    L = lib.api.lib()
    u64 = lambda *v: np.array(v, np.uint64)
    mtm = plan(lib.MtmParams(n=4096, overlap=0.0, w=2.5, kmax=4))
    mtm_s16 = plan(lib.MtmParams(n=4096, overlap=0.0, w=2.5, kmax=4, sample_format=lib.SAMPLES_S16))
    mtm_pitch = plan(lib.MtmParams(n=4096, overlap=0.0, w=2.5, kmax=4, psd_pitch=2112))
    fft = plan(lib.FftParams(n=4096, window_type=0, overlap=0.0))
    mtm_32768 = plan(lib.MtmParams(n=32768, overlap=0.0, w=2.5, kmax=4))
    hop = L.glfer_hip_hop(mtm)
    assert hop == 4096
    some = u64(2 * hop, hop - 1, 3 * hop)                          # 2, 0 and 3 frames
    none = u64(hop - 1, 0, 3)                                      # no frame at all
    zero = u64(0, 0, 0)
    for rows in (False, True):
        fresh = lambda: np.full(4, 9, np.uint64)
        # 1. a NULL plan, whatever else
        assert call(L, rows, None, None, 0, None, None, None, None, None) == E_ARG
        assert call(L, rows, None, None, 3, zero, some, None, None, None) == E_ARG
        # 2. not MTM, or N > 16384 -- before rule 3's GLFER_OK
        st = fresh()
        assert call(L, rows, fft, None, 0, None, None, None, None, st) == E_ARG
        assert call(L, rows, mtm_32768, None, 0, None, None, None, None, st) == E_ARG
        assert list(st) == [9, 9, 9, 9]
        # 3. no streams: GLFER_OK, row_starts[0] = 0, NULL arrays are fine
        assert call(L, rows, mtm, None, 0, None, None, None, None, st) == 0
        assert list(st) == [0, 9, 9, 9]
        assert call(L, rows, mtm, None, 0, None, None, None, None, None) == 0      # (row_starts is optional)
        # 4. NULL offsets / lengths
        st = fresh()
        assert call(L, rows, mtm, None, 3, None, none, None, None, st) == E_ARG
        assert call(L, rows, mtm, None, 3, zero, None, None, None, st) == E_ARG
        # 5. the per-stream checks, before row_starts is filled and before rule 7's GLFER_OK
        assert call(L, rows, mtm, None, 3, zero, u64(hop - 1, hop * 2 ** 31, 0), None, None, st) == E_ARG     # 2^31 frames
        assert call(L, rows, mtm_s16, None, 3, u64(0, 3, 0), none, None, None, st) == E_ARG                   # odd offset, s16
        assert call(L, rows, mtm, None, 3, u64(0, 2 ** 63, 0), u64(0, hop, 0), None, None, st) == E_ARG       # offset + length
        assert list(st) == [9, 9, 9, 9]
        # (an odd offset is free for f32: the same call passes rule 5 and ends at rule 7)
        assert call(L, rows, mtm, None, 3, u64(0, 3, 0), none, None, None, st) == 0
        # 6, 7. row_starts filled; no frame at all: GLFER_OK with NULL samples and outputs
        assert list(st) == [0, 0, 0, 0]
        # 8. frames but no samples / outputs: refused -- after row_starts was filled (6 before 8)
        st = fresh()
        assert call(L, rows, mtm, None, 3, zero, some, None, None, st) == E_ARG
        assert list(st) == [0, 2, 2, 5]
        st = fresh()
        assert call(L, rows, mtm_s16, None, 3, u64(0, 2, 4), some, None, None, st) == E_ARG                   # (even offsets pass rule 5)
        assert list(st) == [0, 2, 2, 5]
    # 5, the row sizes: the rows-and-F entry sizes its rows with the pitch (2112 floats), F with N/2+1 (2049).  A row count
    # between 2^64 / (4 * 2112) and 2^64 / (4 * 2049) overflows the first only: F goes on to rule 6 (row_starts filled) and
    # fails at rule 8, rows-and-F fails at rule 5 (row_starts untouched)
    per = 2 ** 31 - 1
    nb = (2 ** 64 // (4 * 2112)) // per + 2
    assert nb * per * 4 * 2112 >= 2 ** 64 > nb * per * 4 * 2049
    lens = np.full(nb, per * hop, np.uint64)
    offs = np.zeros(nb, np.uint64)
    for rows in (False, True):
        st = np.full(nb + 1, 9, np.uint64)
        assert call(L, rows, mtm_pitch, None, nb, offs, lens, None, None, st) == E_ARG
        assert int(st[-1]) == (9 if rows else nb * per), rows
