"""The multi-channel entries without a GPU: exported, every argument error, a clean failure where no device exists, and
glfer_amd/csrc/channel_cuts.h -- which hops a frame range reads, the plane pitch, the piece list under a byte budget -- walked by
tests/c_channel_cuts.c as a C99 caller and checked here against the definitions."""
import ctypes as C
import os
import struct
import subprocess
import sys
import wave

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG = -1
ENTRIES = ("glfer_hip_deinterleave_device", "glfer_hip_spectrogram_channels_device", "glfer_hip_spectrogram_host_channels",
           "glfer_hip_spectrogram_wav_channels")


def test_channel_entries_exported(lib):
    L = lib.api.lib()
    for name in ENTRIES:
        assert hasattr(L, name), name
        assert name in lib.api.EXPORTS, name
    for name in ("run_channels", "run_host_channels", "run_wav_channels"):
        assert callable(getattr(lib.Spectrogram, name, None)), name
    assert callable(lib.api.deinterleave) and callable(lib.deinterleave)      # the fifth: the kernel alone, from Python
    assert L.glfer_hip_abi_version() == 5
    header = open(os.path.join(ROOT, "include", "glfer_hip.h")).read()
    assert "#define GLFER_HIP_ABI 5" in header
    for name in ENTRIES:
        assert name + "(" in header, name


def _ints(*v):
    return (C.c_int * len(v))(*v)


def test_deinterleave_argument_errors(lib):
    """The kernel's entry takes no plan: every refusal is reached here, none touches a device (the pointers are never read)."""
    L = lib.api.lib()
    f = L.glfer_hip_deinterleave_device
    fake_in, fake_out = C.c_void_p(0x1000), C.c_void_p(0x100000)
    for channels in (0, -1, 65):
        assert f(fake_in, 8, channels, 0, None, 0, fake_out, 8, None) == E_ARG
    for nselect in (0, -1, 65):
        assert f(fake_in, 8, 2, 0, _ints(0, 1), nselect, fake_out, 8, None) == E_ARG
    assert f(fake_in, 8, 2, 0, _ints(0, 2), 2, fake_out, 8, None) == E_ARG           # an index that is no channel
    assert f(fake_in, 8, 2, 0, _ints(-1), 1, fake_out, 8, None) == E_ARG
    for fmt in (-1, 3):
        assert f(fake_in, 8, 2, fmt, None, 0, fake_out, 8, None) == E_ARG
    assert f(fake_in, 8, 2, 0, None, 0, fake_out, 7, None) == E_ARG                  # out_pitch < nframes
    assert f(None, 0, 2, 0, None, 0, None, 0, None) == 0                             # no frames: nothing to do
    assert f(None, 8, 2, 0, None, 0, fake_out, 8, None) == E_ARG                     # NULL buffers while there is work
    assert f(fake_in, 8, 2, 0, None, 0, None, 8, None) == E_ARG
    big = 2 ** 63
    assert f(fake_in, big, 4, 0, None, 0, fake_out, big, None) == E_ARG              # channels * nframes * 4 overflows
    assert f(fake_in, 8, 2, 0, None, 0, fake_out, big, None) == E_ARG                # nselect * out_pitch * 4 overflows


def _plan(lib, params=None):
    """A plan where one can be made (a plan needs a device for its tables), else None."""
    L = lib.api.lib()
    cfg = lib.api.make_config(params or lib.FftParams(n=1024, window_type=0, overlap=0.5, sample_format=lib.SAMPLES_S16))
    h = C.c_void_p()
    return h if L.glfer_hip_plan_create(C.byref(cfg), C.byref(h)) == 0 else None


def _wav(path, channels, width, nframes, extra=b""):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(channels)
        w.setsampwidth(width)
        w.setframerate(48000)
        w.writeframes(bytes(nframes * channels * width) + extra)


def plan_argument_checks(lib, h, tmp_path):
    """Every refusal of the three plan entries that needs a plan; shared with tests/test_gpu_channels.py, where a plan always
    exists.  The buffers are fake addresses: a refusal must come before anything reads them."""
    L = lib.api.lib()
    dev, host, ch_host = L.glfer_hip_spectrogram_channels_device, L.glfer_hip_spectrogram_host_channels, L.glfer_hip_spectrogram_wav_channels
    hop = L.glfer_hip_hop(h)
    fake, out = C.c_void_p(0x1000), C.c_void_p(0x100000)
    nf = C.c_size_t(77)
    per = 10 * hop
    for channels in (0, 65):
        assert dev(h, fake, per, channels, None, 0, 0, 4, out, None) == E_ARG
        assert host(h, fake, per, channels, None, 0, out, C.byref(nf)) == E_ARG
    for nselect in (0, 65):
        assert dev(h, fake, per, 2, _ints(0, 1), nselect, 0, 4, out, None) == E_ARG
        assert host(h, fake, per, 2, _ints(0, 1), nselect, out, C.byref(nf)) == E_ARG
    assert dev(h, fake, per, 2, _ints(2), 1, 0, 4, out, None) == E_ARG
    assert host(h, fake, per, 2, _ints(2), 1, out, C.byref(nf)) == E_ARG
    assert dev(h, None, per, 2, None, 0, 0, 0, None, None) == 0                      # no frames
    assert dev(h, None, per, 2, None, 0, 0, 4, out, None) == E_ARG                   # NULL buffers while there is work
    assert dev(h, fake, per, 2, None, 0, 0, 4, None, None) == E_ARG
    assert dev(h, fake, per, 2, None, 0, 7, 4, out, None) == E_ARG                   # a frame past the recording
    assert dev(h, fake, per, 2, None, 0, 2 ** 64 - 2, 4, out, None) == E_ARG         # first + nframes wraps
    assert dev(h, fake, 2 ** 33 * hop, 2, None, 0, 0, 2 ** 31, out, None) == E_ARG   # nframes > 0x7fffffff
    assert dev(h, fake, 2 ** 62, 8, None, 0, 0, 4, out, None) == E_ARG               # channels * samples * size overflows
    assert host(h, None, per, 2, None, 0, out, C.byref(nf)) == E_ARG
    assert host(h, fake, per, 2, None, 0, None, C.byref(nf)) == E_ARG
    assert host(h, fake, per, 2, None, 0, out, None) == E_ARG
    assert host(h, fake, 2 ** 62, 8, None, 0, out, C.byref(nf)) == E_ARG
    assert host(h, None, hop - 1, 2, None, 0, None, C.byref(nf)) == 0 and nf.value == 0   # shorter than a hop: no frame, no work
    # files: the plan takes 16-bit samples
    stereo16, stereo8 = tmp_path / "s16.wav", tmp_path / "u8.wav"
    _wav(stereo16, 2, 2, 4 * hop)
    _wav(stereo8, 2, 1, 4 * hop)
    enc = lambda p: os.fsencode(str(p))
    assert ch_host(h, enc(stereo8), None, 0, out, 4, C.byref(nf), 0) == E_ARG        # bit depth does not match the plan
    assert ch_host(h, enc(stereo16), _ints(2), 1, out, 4, C.byref(nf), 0) == E_ARG
    assert ch_host(h, enc(stereo16), _ints(0, 1), 65, out, 4, C.byref(nf), 0) == E_ARG
    assert ch_host(h, enc(stereo16), None, 0, None, 4, C.byref(nf), 0) == E_ARG      # NULL rows while there is work
    assert ch_host(h, enc(stereo16), None, 0, out, 2 ** 64 - 1, C.byref(nf), 0) == E_ARG   # two planes an unbounded max_frames apart
    assert ch_host(h, enc(stereo16), None, 0, out, 4, None, 0) == E_ARG
    assert ch_host(h, None, None, 0, out, 4, C.byref(nf), 0) == E_ARG
    assert ch_host(h, enc(tmp_path / "missing.wav"), None, 0, out, 4, C.byref(nf), 0) < 0
    assert ch_host(h, enc(stereo16), None, 0, None, 0, C.byref(nf), 0) == 0 and nf.value == 0   # max_frames 0: nothing to do


def test_null_plan_and_plan_argument_errors(lib, tmp_path):
    L = lib.api.lib()
    nf = C.c_size_t(0)
    fake = C.c_void_p(0x1000)
    assert L.glfer_hip_spectrogram_channels_device(None, fake, 4096, 2, None, 0, 0, 1, fake, None) == E_ARG
    assert L.glfer_hip_spectrogram_channels_device(None, None, 0, 0, None, 0, 0, 0, None, None) == E_ARG
    assert L.glfer_hip_spectrogram_host_channels(None, fake, 4096, 2, None, 0, fake, C.byref(nf)) == E_ARG
    assert L.glfer_hip_spectrogram_wav_channels(None, b"x.wav", None, 0, fake, 1, C.byref(nf), 0) == E_ARG
    h = _plan(lib)
    if h is not None:                      # (a plan needs a device; tests/test_gpu_channels.py runs the same checks where one exists)
        try:
            plan_argument_checks(lib, h, tmp_path)
            cfg = lib.api.make_config(lib.FftParams(n=1024, window_type=0, overlap=0.5, psd_pitch=528))
            hp = C.c_void_p()
            assert L.glfer_hip_plan_create(C.byref(cfg), C.byref(hp)) == 0
            try:                           # the host entries keep dense rows
                assert L.glfer_hip_spectrogram_host_channels(hp, fake, 8192, 2, None, 0, fake, C.byref(nf)) == E_ARG
            finally:
                L.glfer_hip_plan_destroy(hp)
        finally:
            L.glfer_hip_plan_destroy(h)


_NO_DEVICE = r"""
import ctypes as C, sys
sys.path.insert(0, sys.argv[1])
import glfer_amd as G
L = G.api.lib()
cfg = G.api.make_config(G.FftParams(n=1024, window_type=0, overlap=0.5))
h = C.c_void_p()
rc = L.glfer_hip_plan_create(C.byref(cfg), C.byref(h))
print("plan", rc)
fake = C.c_void_p(0x1000)
print("null", L.glfer_hip_spectrogram_channels_device(None, fake, 4096, 2, None, 0, 0, 4, fake, None))
# the kernel's entry needs no plan: with buffers it has to open a device, and there is none
print("kernel", L.glfer_hip_deinterleave_device(fake, 64, 2, 0, None, 0, C.c_void_p(0x100000), 64, None))
if rc == 0:
    print("channels", L.glfer_hip_spectrogram_channels_device(h, None, 4096, 2, None, 0, 0, 4, None, None))
    L.glfer_hip_plan_destroy(h)
"""


def test_channels_without_device_fail_cleanly():
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, "-c", _NO_DEVICE, ROOT], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    out = dict(line.split() for line in r.stdout.splitlines() if line.split() and line.split()[0] in ("plan", "null", "kernel", "channels"))
    assert int(out["null"]) == E_ARG, r.stdout                   # GLFER_E_ARG, no crash
    assert int(out["kernel"]) < 0, r.stdout                      # an error code, not a crash and not a quiet success
    if int(out["plan"]) == 0:
        assert int(out["channels"]) == E_ARG, r.stdout
    else:
        assert int(out["plan"]) < 0, r.stdout


# ---- channel_cuts.h ----------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    exe = tmp_path_factory.mktemp("channel_cuts") / "c_channel_cuts"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "glfer_amd", "csrc"),
                    os.path.join(ROOT, "tests", "c_channel_cuts.c"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-2000:])
    rows = {}
    for line in r.stdout.splitlines():
        kind, *nums = line.split()
        rows.setdefault(kind, []).append(tuple(int(v) for v in nums))
    return rows


def test_hops_of_a_frame_range(lines):
    """Overlaps 0, 0.3, 0.5, 0.75, 0.875 at N = 1024, with and without the LMP term, first_frame 0, 1, at and beyond the halo:
    the hops are those the frames read one by one -- frame f reads hop f and the `halo` hops below it, none below hop 0."""
    halos = {(keep, hop, lmp): halo for keep, hop, lmp, halo in lines["halo"]}
    assert len(halos) == 10
    for (keep, hop, lmp), halo in halos.items():
        back = min(k for k in range(keep + 1) if k * hop >= keep)           # whole hops that cover the N - H samples kept
        assert halo == back + (lmp - 1 if lmp else 0)
    assert {halos[(1024 - h, h, 0)] for h in (1024, 716, 512, 256, 128)} == {0, 1, 3, 7}
    assert halos[(308, 716, 0)] == 1 and halos[(896, 128, 4)] == 10
    assert len(lines["hops"]) == 10 * 4 * 4
    for first, nframes, halo, lo, n in lines["hops"]:
        read = sorted({h for f in range(first, first + nframes) for h in range(max(0, f - halo), f + 1)})
        if not read:
            assert n == 0
        else:
            assert (lo, n) == (read[0], len(read)) and read == list(range(lo, lo + n))


def test_plane_pitch_rounding(lines):
    assert len(lines["pitch"]) == 3 * 71
    for n, esz, pitch in lines["pitch"]:
        assert pitch >= n and (pitch * esz) % 16 == 0 and (pitch - n) * esz < 16    # the next multiple of 16 bytes, no more
        if esz < 4:
            assert pitch % 2 == 0                                                    # the batch entry's even-pitch rule


def test_piece_lists_under_shrinking_budgets(lines):
    runs = {}
    for hop, halo, esz, planes, first, end, budget, at, to, nbytes in lines["piece"]:
        runs.setdefault((hop, halo, esz, planes, first, end, budget), []).append((at, to, nbytes))
    assert len(runs) > 500
    cut = 0
    for (hop, halo, esz, planes, first, end, budget), pieces in runs.items():
        # every frame once, in order
        assert pieces[0][0] == first and pieces[-1][1] == end
        assert all(a[1] == b[0] for a, b in zip(pieces, pieces[1:])) and all(at < to for at, to, _ in pieces)
        for i, (at, to, nbytes) in enumerate(pieces):
            lo = max(0, at - halo)
            assert nbytes == planes * (((to - lo) * hop * esz + 15) // 16 * 16)       # the planes of its hops, halo included
            if i:
                assert at % 32 == 0                                                     # cuts on global multiples of GLFER_FRAME_ALIGN
            if i + 1 < len(pieces):
                assert to - at >= 32                                                    # a piece is a frame group at least
            if nbytes > budget:
                assert to - at < 64                                                     # over the budget: only the minimum-size piece
            elif i + 1 < len(pieces):
                # as large as the budget allows: one more group would not have fitted
                assert planes * (((min(to + 32, end) - lo) * hop * esz + 15) // 16 * 16) > budget
        cut += len(pieces) > 2
    assert cut > 100                                                                    # (the budgets did cut)
    whole = [k for k, p in runs.items() if len(p) == 1 and p[0][2] <= k[6]]
    assert len(whole) >= 3 * 3 * 2 * 6                                                  # the first budget of every case fits it in one piece


def test_selection(lines):
    assert lines["select"] == [(3,), (4, 2, 1, 1), (0, 0, 0, 0, 0, 0, 64)]
