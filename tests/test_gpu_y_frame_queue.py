"""spectro16y.hip's queue form (one workgroup per resident slot, frame pairs drawn in chunks from a counter the plan owns)
gives the rows of the static-stride launch BIT FOR BIT: which workgroup takes a frame pair changes nothing that is computed
for it.

The reference rows come from ONE fresh child process that runs this file's own cases with GLFER_Y_QUEUE=0 (the static
stride); the process under test runs them with the queue on.  Every case is one plan called several times in a row on
one stream with different frame counts, the rows of every call compared: the counter is never reset, so a wrong ticket
base shows in the second call at the latest.

Frame counts, with G workgroups in a full grid and C frame pairs per ticket (glfer_hip_y_queue_shape): 1, 2 (a single
workgroup, no ticket succeeds), 3 (odd), 2GC - 1, 2GC, 2GC + 1 (the static chunks exactly), 2GC + 2, 2GC + 3 (one drawn
pair), 2(GC + C) + 1 (one full drawn chunk and an odd end), and a few thousand pairs (many tickets per workgroup).
(An estimator launch is cut on frame pairs -- include/glfer_hip.h, "Cutting a stream" -- so an odd count's last frame goes
to the packed kernel; the counts with + 2 and + 3 are there so that the drawn pair exists on either side of that cut.)"""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from _signals import synth  # noqa: E402

pytestmark = pytest.mark.gpu
N = 4096
ENV = ("GLFER_FORM", "GLFER_Y_TAPERS", "GLFER_Y_QUEUE", "GLFER_Y_CHUNK", "GLFER_MEAN_PREPASS")


def _shape(lib):
    import ctypes
    L = lib.api.lib()
    g, c = ctypes.c_int(0), ctypes.c_int(0)
    L.glfer_hip_y_queue_shape(ctypes.byref(g), ctypes.byref(c))
    assert g.value >= 8 and c.value >= 1
    return g.value, c.value


def _cases(lib):
    """name -> (params, kind, environment, frame counts of the calls in order)"""
    G, C = _shape(lib)
    edge = 2 * G * C
    every = [1, 2, 3, edge - 1, edge, edge + 1, edge + 2, edge + 3, 2 * (G * C + C) + 1, 2 * 3001 + 1, 6]
    three = [2 * (G * C + C) + 1, edge + 2, 5]                       # three calls in a row, one drawn chunk / one drawn pair / none
    cases = {"f32": (dict(fmt="f32"), "run", {}, every)}
    for fmt in ("f32", "s16", "u8"):
        for hist in (0, 1):
            if (fmt, hist) != ("f32", 0):
                cases["%s_hist%d" % (fmt, hist)] = (dict(fmt=fmt, history_mode=hist), "run", {}, three)
    cases["full_tables"] = (dict(fmt="f32"), "run", {"GLFER_Y_TAPERS": "full"}, three)
    cases["seven_tapers_hist1"] = (dict(fmt="s16", w=4.0, kmax=6, history_mode=1), "run", {}, three)
    cases["overlap75"] = (dict(fmt="f32", overlap=0.75), "run", {}, three)
    # the launches that keep the static stride: a batch, and the in-kernel mean forms (both orders of summation)
    cases["batch"] = (dict(fmt="f32"), "batch", {}, [edge // 2 + 6, 61])
    cases["sub_mean_fast"] = (dict(fmt="f32", sub_mean=2), "run", {}, [edge + 6, 44])
    cases["sub_mean_exact"] = (dict(fmt="s16", sub_mean=1), "run", {}, [edge + 6, 44])
    return cases


_STREAMS = {}


def _raw(lib, fmt, nsamples):
    if fmt not in _STREAMS:
        x = synth(2 * 3001 * N + 2 * N, seed=21) + np.float32(0.02)
        x[3 * N:4 * N] *= np.float32(1e-4)                      # a quiet frame next to loud ones
        x[6 * N:7 * N] = 0.0                                    # and digital silence
        if fmt == "s16":
            x = np.clip(np.round(x * 20000), -32768, 32767).astype(np.int16)
        elif fmt == "u8":
            x = np.clip(np.round(x * 100 + 128), 0, 255).astype(np.uint8)
        _STREAMS[fmt] = x
    return _STREAMS[fmt][:nsamples]


def _rows(lib, torch, case):
    """The rows of every call of one case, on one plan and one stream, in order."""
    params, kind, env, counts = case
    kw = dict(params)
    fmt = kw.pop("fmt")
    overlap = kw.get("overlap", 0.0)
    kw.setdefault("w", 2.5)
    kw.setdefault("kmax", 4)
    sf = {"f32": lib.SAMPLES_F32, "s16": lib.SAMPLES_S16, "u8": lib.SAMPLES_U8}[fmt]
    hop = int(N * (1.0 - overlap))
    old = {k: os.environ.get(k) for k in ("GLFER_Y_TAPERS",)}
    os.environ.update(env)
    try:
        sp = lib.Spectrogram(lib.MtmParams(n=N, sample_format=sf, **kw))
        out = []
        for frames in counts:
            raw = _raw(lib, fmt, frames * hop + 5)
            if kind == "batch":
                d = torch.from_numpy(np.stack([raw, raw[::-1].copy(), raw * np.float32(0.5)])).cuda()
                out.append(sp.run_batch(d))
            else:
                out.append(sp.run(torch.from_numpy(raw).cuda()))
        torch.cuda.synchronize()
        return out
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


@pytest.fixture(scope="module")
def static_rows(tmp_path_factory):
    """Every case's rows from the static-stride launch: one fresh child process with GLFER_Y_QUEUE=0."""
    out = tmp_path_factory.mktemp("y_static")
    env = {k: v for k, v in os.environ.items() if k not in ENV}
    env["GLFER_Y_QUEUE"] = "0"
    r = subprocess.run([sys.executable, os.path.abspath(__file__), str(out)], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return out


@pytest.fixture(autouse=True)
def _queue_on(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)


def _compare(lib, torch, static_rows, name):
    case = _cases(lib)[name]
    got = _rows(lib, torch, case)
    for i, (frames, rows) in enumerate(zip(case[3], got)):
        want = torch.from_numpy(np.load(static_rows / ("%s_%d.npy" % (name, i)))).cuda()
        assert rows.shape == want.shape and rows.shape[-2] == frames, (name, i, frames)
        assert torch.equal(rows, want), (name, i, frames)
        assert bool(torch.isfinite(rows).all()) and float(rows.max()) > 0.0, (name, i, frames)


def test_every_edge_of_the_queue_on_one_plan(lib, torch_cuda, static_rows):
    """f32, history from the stream, half tables: every frame count of the list above, one call after the other on one plan."""
    _compare(lib, torch_cuda, static_rows, "f32")


@pytest.mark.parametrize("name", ["f32_hist1", "s16_hist0", "s16_hist1", "u8_hist0", "u8_hist1"])
def test_sample_formats_and_history_modes(lib, torch_cuda, static_rows, name):
    _compare(lib, torch_cuda, static_rows, name)


@pytest.mark.parametrize("name", ["full_tables", "seven_tapers_hist1", "overlap75"])
def test_full_table_forms_and_overlapped_frames(lib, torch_cuda, static_rows, name):
    """GLFER_Y_TAPERS=full and seven tapers run the full-table kernel; at 75 % overlap frames share samples."""
    _compare(lib, torch_cuda, static_rows, name)


@pytest.mark.parametrize("name", ["batch", "sub_mean_fast", "sub_mean_exact"])
def test_batched_and_mean_removing_launches_have_not_moved(lib, torch_cuda, static_rows, name):
    """These keep the static stride whatever GLFER_Y_QUEUE says: their rows are the static-stride process's rows."""
    _compare(lib, torch_cuda, static_rows, name)


def test_queue_rows_against_the_oracle(lib, oracle, torch_cuda):
    """... and the rows are right, not only equal: the head of a launch with drawn chunks against the CPU oracle."""
    from _signals import rel_err
    G, C = _shape(lib)
    frames = 2 * (G * C + C) + 1
    x = _raw(lib, "f32", frames * N)
    sp = lib.Spectrogram(lib.MtmParams(n=N, w=2.5, kmax=4))
    got = sp.run(torch_cuda.from_numpy(x).cuda())
    torch_cuda.cuda.synchronize()
    head, tail = got[:9].cpu().numpy(), got[frames - 4:].cpu().numpy()
    want_head = oracle.spectrogram_mtm(x[:9 * N], N, 0.0, 2.5, 4)
    want_tail = oracle.spectrogram_mtm(x[(frames - 4) * N:frames * N], N, 0.0, 2.5, 4)     # (overlap 0: a frame is its own hop)
    for f in range(9):
        if want_head[f].max() > 0.0:
            assert max(rel_err(head[f], want_head[f])) < 1e-5, f
    for f in range(4):
        assert max(rel_err(tail[f], want_tail[f])) < 1e-5, f


if __name__ == "__main__":                                       # the child process of static_rows
    import torch
    import glfer_amd
    glfer_amd.api.lib()
    assert os.environ.get("GLFER_Y_QUEUE") == "0"
    for name_, case_ in _cases(glfer_amd).items():
        for i_, rows_ in enumerate(_rows(glfer_amd, torch, case_)):
            np.save(os.path.join(sys.argv[1], "%s_%d.npy" % (name_, i_)), rows_.cpu().numpy())
