"""spectro16y.hip's half-table form (five tapers at N = 4096: the tapers in registers as mirror-symmetric half tables,
the upper half taken from the DPP row_mirror partner) gives the rows of the full-table form BIT FOR BIT.

Two references, both on the GPU: the rows under GLFER_FORM=x (the shared-odd-taper route forced), and the rows of the
same plan with GLFER_Y_TAPERS=full, which makes the launcher keep the full-table kernel -- the form every plan ran
before, and the one that differs from the form under test."""
import os

import numpy as np
import pytest

from _signals import rel_err, synth

pytestmark = pytest.mark.gpu
N = 4096


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _raw(lib, fmt, nsamples, seed):
    x = synth(nsamples, seed=seed) + np.float32(0.02)
    x[3 * N:4 * N] *= np.float32(1e-4)                      # a quiet frame next to loud ones
    x[6 * N:7 * N] = 0.0                                    # and digital silence
    if fmt == "s16":
        return np.clip(np.round(x * 20000), -32768, 32767).astype(np.int16), lib.SAMPLES_S16
    if fmt == "u8":
        return np.clip(np.round(x * 100 + 128), 0, 255).astype(np.uint8), lib.SAMPLES_U8
    return x, lib.SAMPLES_F32


def _with_env(env, fn):
    old = {k: os.environ.get(k) for k in ("GLFER_FORM", "GLFER_Y_TAPERS")}
    try:
        for k in old:
            os.environ.pop(k, None)
        os.environ.update(env)
        return fn()
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def _three_ways(torch, run):
    new = _with_env({}, run)
    form_x = _with_env({"GLFER_FORM": "x"}, run)
    full = _with_env({"GLFER_Y_TAPERS": "full"}, run)
    torch.cuda.synchronize()
    return new, form_x, full


@pytest.mark.parametrize("history_mode", [0, 1])
@pytest.mark.parametrize("frames", [44, 45])
@pytest.mark.parametrize("fmt", ["f32", "s16", "u8"])
@pytest.mark.parametrize("overlap", [0.0, 0.75])
def test_half_table_rows_equal_full_table_rows(lib, torch_cuda, overlap, fmt, frames, history_mode):
    """C3 and C3 at 75 % overlap, every sample format, odd and even frame counts, both history modes; whole launches and
    a launch that starts inside the stream."""
    hop = int(N * (1.0 - overlap))
    raw, sf = _raw(lib, fmt, frames * hop + 5, seed=frames)
    sp = lib.Spectrogram(lib.MtmParams(n=N, overlap=overlap, w=2.5, kmax=4, sample_format=sf, history_mode=history_mode))
    d = torch_cuda.from_numpy(raw).cuda()
    new, form_x, full = _three_ways(torch_cuda, lambda: sp.run(d))
    assert new.shape[0] == frames
    assert torch_cuda.equal(new, form_x)
    assert torch_cuda.equal(new, full)
    assert float(new.max()) > 0.0 and bool(torch_cuda.isfinite(new).all())
    # (cut on frame pairs: a frame keeps its bits only while it stays in the same kernel, include/glfer_hip.h, "Cutting a stream")
    part, part_x, part_full = _three_ways(torch_cuda, lambda: sp.run(d, first_frame=10, nframes=30))
    assert torch_cuda.equal(part, part_x)
    assert torch_cuda.equal(part, part_full)
    assert torch_cuda.equal(part, new[10:40])


@pytest.mark.parametrize("overlap,fmt,frames", [(0.0, "f32", 16384 + 4097), (0.75, "s16", 2 * 16384 + 1234)])
def test_half_table_rows_over_launches_longer_than_one_pass_of_the_grid(lib, oracle, torch_cuda, overlap, fmt, frames):
    """The persistent grid takes 16384 frames per pass: every workgroup goes round its loop again, the last pass ragged."""
    hop = int(N * (1.0 - overlap))
    raw, sf = _raw(lib, fmt, frames * hop, seed=3)
    sp = lib.Spectrogram(lib.MtmParams(n=N, overlap=overlap, w=2.5, kmax=4, sample_format=sf))
    d = torch_cuda.from_numpy(raw).cuda()
    new, form_x, full = _three_ways(torch_cuda, lambda: sp.run(d))
    assert torch_cuda.equal(new, form_x)
    assert torch_cuda.equal(new, full)
    # and a few rows against the oracle (the stream's head; frames past the zero history run in the kernel under test)
    xf = raw if fmt == "f32" else oracle.pcm_s16_to_float(raw)
    head = 12
    want = oracle.spectrogram_mtm(xf[:head * hop], N, overlap, 2.5, 4)
    got = new[:head].cpu().numpy()
    for f in range(head):
        if want[f].max() > 0.0:
            assert max(rel_err(got[f], want[f])) < 1e-5, f


@pytest.mark.parametrize("overlap", [0.0, 0.75])
def test_half_table_rows_of_a_three_stream_batch(lib, torch_cuda, overlap):
    hop = int(N * (1.0 - overlap))
    frames = 61
    rows = [_raw(lib, "f32", frames * hop, seed=10 + b)[0] * np.float32(1.0 / (1 + b)) for b in range(3)]
    sp = lib.Spectrogram(lib.MtmParams(n=N, overlap=overlap, w=2.5, kmax=4))
    d = torch_cuda.from_numpy(np.stack(rows)).cuda()
    new, form_x, full = _three_ways(torch_cuda, lambda: sp.run_batch(d))
    assert torch_cuda.equal(new, form_x)
    assert torch_cuda.equal(new, full)
    for b in range(3):
        assert torch_cuda.equal(new[b], sp.run(d[b]))


@pytest.mark.parametrize("nw", [3.5, 4.0])
@pytest.mark.parametrize("overlap", [0.0, 0.75])
def test_tapers_that_are_not_exactly_symmetric_keep_the_full_tables(lib, oracle, torch_cuda, overlap, nw):
    """NW = 3.5 and 4 with five tapers: the scaled float tables are not exactly (anti)symmetric (the host test
    checks that), so the plan has no half table and runs the full-table kernel as before -- GLFER_Y_TAPERS=full changes
    nothing, and the rows are the oracle's."""
    L = lib.api.lib()
    half = np.zeros((256, 40), np.float32)
    assert L.glfer_hip_y_half_tables(N, 4, nw, half.ctypes.data, None, None) == 0
    hop = int(N * (1.0 - overlap))
    frames = 37
    x, sf = _raw(lib, "f32", frames * hop + 3, seed=5)
    sp = lib.Spectrogram(lib.MtmParams(n=N, overlap=overlap, w=nw, kmax=4))
    d = torch_cuda.from_numpy(x).cuda()
    new, form_x, full = _three_ways(torch_cuda, lambda: sp.run(d))
    assert torch_cuda.equal(new, form_x)
    assert torch_cuda.equal(new, full)
    want = oracle.spectrogram_mtm(x, N, overlap, nw, 4)
    got = new.cpu().numpy()
    for f in range(frames):
        if want[f].max() > 0.0:
            assert max(rel_err(got[f], want[f])) < 1e-5, f
        else:
            assert not got[f].any(), f                      # digital silence stays silence
