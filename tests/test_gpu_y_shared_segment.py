"""spectro16y.hip's half-table forms fold the mirror bins inside the separation's LDS pass (entries {Re Z, Im Z, accA, accB})
and run the shared round through both exchange buffers without the buffer-release barriers; the full-table forms keep the
fold in front of the shared round and the one-buffer passes.  Every floating-point operation meets the same operands in the
same order in both, so the rows must be equal BIT FOR BIT: the full-table route of the same library (GLFER_Y_TAPERS=full,
the switch tests/test_gpu_y_half_tapers.py uses) is the reference here, and the oracle once at the project's 1e-5.

All cases: N = 4096, NW = 2.5, kmax = 4 (five tapers).  The kernel takes the whole frame pairs that lie inside the stream
(frame_cuts.h; the frames around them go to the packed kernel in both routes): at overlap 0 from frame 0, at 75 % overlap
from frame 4, so a stream is LEAD + frames long with LEAD = 0 / 4.  Frame counts 1, 2, 3, 7, 8, 9, 17: no frame B to pair
with (1, and the odd last frame of 3, 7, 9, 17), one pair, three pairs, exactly one queue chunk of four pairs = 8 frames, one
chunk with a frame over, and two chunks (17), each drawn by a workgroup of its own that then draws the ticket that ends it."""
import os

import numpy as np
import pytest

from _signals import rel_err, synth

pytestmark = pytest.mark.gpu
N = 4096
FRAMES = [1, 2, 3, 7, 8, 9, 17]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


_plans = {}


def _plan(lib, overlap, fmt, history_mode):
    key = (overlap, fmt, history_mode)
    if key not in _plans:
        sf = {"f32": lib.SAMPLES_F32, "s16": lib.SAMPLES_S16, "u8": lib.SAMPLES_U8}[fmt]
        _plans[key] = lib.Spectrogram(lib.MtmParams(n=N, overlap=overlap, w=2.5, kmax=4, sample_format=sf, history_mode=history_mode))
    return _plans[key]


def _lead(overlap):
    return 0 if overlap == 0.0 else 4


def _as_format(x, fmt):
    if fmt == "s16":
        return np.clip(np.round(x * 20000), -32768, 32767).astype(np.int16)
    if fmt == "u8":
        return np.clip(np.round(x * 100 + 128), 0, 255).astype(np.uint8)
    return x.astype(np.float32)


def _with_env(env, fn):
    keys = ("GLFER_FORM", "GLFER_Y_TAPERS", "GLFER_Y_QUEUE", "GLFER_Y_CHUNK")
    old = {k: os.environ.get(k) for k in keys}
    try:
        for k in keys:
            os.environ.pop(k, None)
        os.environ.update(env)
        return fn()
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def _both(torch, run):
    new = _with_env({}, run)
    full = _with_env({"GLFER_Y_TAPERS": "full"}, run)
    torch.cuda.synchronize()
    return new, full


@pytest.mark.parametrize("history_mode", [0, 1])
@pytest.mark.parametrize("frames", FRAMES)
@pytest.mark.parametrize("fmt", ["f32", "s16", "u8"])
@pytest.mark.parametrize("overlap", [0.0, 0.75])
def test_half_table_rows_equal_full_table_rows(lib, torch_cuda, overlap, fmt, frames, history_mode):
    hop = int(N * (1.0 - overlap))
    total = _lead(overlap) + frames
    x = synth(total * hop, seed=100 + frames) + np.float32(0.02)   # (frame f ends with sample (f + 1) * hop - 1)
    d = torch_cuda.from_numpy(_as_format(x, fmt)).cuda()
    sp = _plan(lib, overlap, fmt, history_mode)
    new, full = _both(torch_cuda, lambda: sp.run(d))
    assert new.shape[0] == total
    assert torch_cuda.equal(new, full)
    assert float(new.max()) > 0.0 and bool(torch_cuda.isfinite(new).all())


@pytest.mark.parametrize("fmt", ["f32", "s16", "u8"])
@pytest.mark.parametrize("overlap", [0.0, 0.75])
def test_chunks_drawn_from_the_queue(lib, torch_cuda, overlap, fmt):
    """561 frames = 70 chunks and a frame over: the grid is 64 workgroups (whole XCD slices), so six chunks are taken with
    tickets that succeed -- a workgroup's second chunk starts with the samples its shared round's hook asked for."""
    hop = int(N * (1.0 - overlap))
    total = _lead(overlap) + 561
    x = synth(total * hop, seed=21) + np.float32(0.02)
    d = torch_cuda.from_numpy(_as_format(x, fmt)).cuda()
    sp = _plan(lib, overlap, fmt, 0)
    new, full = _both(torch_cuda, lambda: sp.run(d))
    assert new.shape[0] == total
    assert torch_cuda.equal(new, full)
    assert float(new.min()) >= 0.0 and float(new[-2].max()) > 0.0 and bool(torch_cuda.isfinite(new).all())


@pytest.mark.parametrize("history_mode", [0, 1])
@pytest.mark.parametrize("overlap", [0.0, 0.75])
def test_a_digitally_silent_frame_beside_a_loud_one(lib, torch_cuda, overlap, history_mode):
    """A frame whose power over the first four tapers is exactly 0 enters the shared transform with scale 0 (kSilent) and
    must come out exactly 0 whatever its loud partner leaves in the transform; as frame A of a pair and as frame B."""
    hop = int(N * (1.0 - overlap))
    total = _lead(overlap) + 8
    x = synth(total * hop, seed=7)
    # frame f is samples [(f + 1) * hop - N, (f + 1) * hop).  Overlap 0: frames 2 (an A) and 5 (a B) zeroed.  75 %: hops
    # 3..10 zeroed, so frames 6..10 (with history_mode 1, which keeps a frame's own hop only, 3..10) are silent and frame
    # 10 shares its pair with the loud frame 11.
    if overlap == 0.0:
        x[2 * N:3 * N] = 0.0
        x[5 * N:6 * N] = 0.0
    else:
        x[3 * hop:11 * hop] = 0.0
    d = torch_cuda.from_numpy(x).cuda()
    sp = _plan(lib, overlap, "f32", history_mode)
    new, full = _both(torch_cuda, lambda: sp.run(d))
    assert torch_cuda.equal(new, full)
    rows = new.cpu().numpy()
    silent = [f for f in range(_lead(overlap), total) if not rows[f].any()]
    loud = [f for f in range(_lead(overlap), total) if rows[f].max() > 0.01 * rows.max()]
    assert silent and loud, (silent, loud)
    assert any(f % 2 == 0 for f in silent) and any(f % 2 == 1 for f in silent), silent
    assert any(abs(f - g) == 1 and f // 2 == g // 2 for f in silent for g in loud), (silent, loud)
    assert bool(torch_cuda.isfinite(new).all())


@pytest.mark.parametrize("fmt", ["f32", "s16"])
@pytest.mark.parametrize("overlap", [0.0, 0.75])
def test_neighbouring_frames_sixty_db_apart(lib, torch_cuda, oracle, overlap, fmt):
    """The two frames of a pair enter the shared transform with scales of their own: a frame 60 dB below its partner keeps
    the accuracy of a transform of its own (the oracle at 1e-5 per row, overlap 0) and the full-table form's bits."""
    hop = int(N * (1.0 - overlap))
    total = _lead(overlap) + 10
    x = synth(total * hop, seed=11)
    gain = np.ones(x.shape[0], np.float32)
    for f in range(0, total + 4, 2):                  # every other frame-length span 60 dB down
        gain[f * N:(f + 1) * N] = np.float32(1e-3)
    x = x * gain
    raw = _as_format(x, fmt)
    d = torch_cuda.from_numpy(raw).cuda()
    sp = _plan(lib, overlap, fmt, 0)
    new, full = _both(torch_cuda, lambda: sp.run(d))
    assert torch_cuda.equal(new, full)
    assert bool(torch_cuda.isfinite(new).all())
    if overlap == 0.0 and fmt == "f32":
        rows = new.cpu().numpy()
        want = oracle.spectrogram_mtm(x, N, overlap, 2.5, 4)
        peaks = [want[f].max() for f in range(total)]
        assert max(peaks) / min(peaks) > 1e5            # 60 dB in amplitude = 120 dB in power, less the noise's share
        for f in range(total):
            assert max(rel_err(rows[f], want[f])) < 1e-5, f


@pytest.mark.parametrize("overlap", [0.0, 0.75])
def test_rows_against_the_oracle(lib, oracle, torch_cuda, overlap):
    hop = int(N * (1.0 - overlap))
    total = _lead(overlap) + 17
    x = synth(total * hop, seed=3)
    d = torch_cuda.from_numpy(x).cuda()
    sp = _plan(lib, overlap, "f32", 0)
    got = _with_env({}, lambda: sp.run(d)).cpu().numpy()
    want = oracle.spectrogram_mtm(x, N, overlap, 2.5, 4)
    for f in range(total):
        assert max(rel_err(got[f], want[f])) < 1e-5, f
