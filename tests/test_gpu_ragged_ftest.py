"""The harmonic F-test and the rows-and-F pair over streams of unequal length in one call (-m gpu):
glfer_hip_mtm_ftest_ragged_device / glfer_hip_mtm_rows_ftest_ragged_device against a loop of the single entries over views of
the same buffer.  Every comparison is of bit patterns (.view(torch.int32): the Nyquist column is x/0), stream by stream.

The streams differ in seed, amplitude and DC level, they lie shuffled in one buffer whose gaps hold NaN (f32) or full-scale
values (s16 / u8), and the outputs are pre-filled with a sentinel and carry guard rows: a row from the wrong stream, an F row
at a PSD row's offset (or the reverse), a read across a stream's start or end, a copy from the wrong table entry or a row
written past a stream's own frames cannot come out equal by accident.
"""
import ctypes as C

import numpy as np
import pytest

from _ragged_ftest_cases import argument_rules, call, layout, lengths

pytestmark = pytest.mark.gpu
SENTINEL = -7.25
GUARD = 3


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _bits(t):
    import torch
    return t.contiguous().view(torch.int32)


def _select(monkeypatch, paired):
    """the F kernel's form: None = the default (paired from N = 2048), 0 / 1 = GLFER_FTEST_PAIRED (read per call)"""
    if paired is None:
        monkeypatch.delenv("GLFER_FTEST_PAIRED", raising=False)
    else:
        monkeypatch.setenv("GLFER_FTEST_PAIRED", str(paired))


def _check(torch, sp, x, offs, lens, rows, mu_live=True):
    """ftest_ragged (rows: rows_ftest_ragged) against ftest / rows_ftest on the same views: bits, guard rows, pitch padding,
    row_starts.  Returns (psd or None, ftest, row_starts)."""
    frames = [n // sp.hop for n in lens]
    total = sum(frames)
    ft = torch.full((total + GUARD, sp.bins), SENTINEL, dtype=torch.float32, device="cuda:0")
    psd = torch.full((total + GUARD, sp.pitch), SENTINEL, dtype=torch.float32, device="cuda:0") if rows else None
    if rows:
        _, _, starts = sp.rows_ftest_ragged(x, offs, lens, mu_live=mu_live, out=(psd, ft))
    else:
        _, starts = sp.ftest_ragged(x, offs, lens, mu_live=mu_live, out=ft)
    torch.cuda.synchronize()
    assert starts.dtype == np.int64 and list(starts) == [0] + list(np.cumsum(frames))
    assert sp.ragged_frames(lens)[0] == total
    want_ft = torch.full_like(ft, SENTINEL)
    want_psd = torch.full_like(psd, SENTINEL) if rows else None
    for b, (o, n) in enumerate(zip(offs, lens)):
        if not frames[b]:
            continue
        r0, r1 = int(starts[b]), int(starts[b + 1])
        if rows:
            sp.rows_ftest(x[o:o + n], mu_live=mu_live, out=(want_psd[r0:r1], want_ft[r0:r1]))
        else:
            want_ft[r0:r1] = sp.ftest(x[o:o + n], mu_live=mu_live)
    torch.cuda.synchronize()
    span = lambda b: slice(int(starts[b]), int(starts[b + 1]))
    bad = [b for b in range(len(lens)) if not torch.equal(_bits(ft[span(b)]), _bits(want_ft[span(b)]))]
    assert not bad, ("F", bad, [frames[b] for b in bad])
    half = sp.bins - 1
    if total:
        assert bool(torch.isfinite(ft[:total, 1:half]).all())
        assert not bool((ft[:total] == SENTINEL).any())
    assert bool((ft[total:] == SENTINEL).all())                  # the guard rows
    if rows:
        bad = [b for b in range(len(lens)) if not torch.equal(_bits(psd[span(b)]), _bits(want_psd[span(b)]))]
        assert not bad, ("PSD", bad, [frames[b] for b in bad])
        if total:
            assert bool(torch.isfinite(psd[:total, :sp.bins]).all()) and not bool((psd[:total, :sp.bins] == SENTINEL).any())
        assert bool((psd[total:] == SENTINEL).all())
        if sp.pitch > sp.bins:
            assert bool((psd[:, sp.bins:] == SENTINEL).all())    # the pitch padding is untouched
    # two different streams' rows differ: the equalities above are not vacuous
    live = [b for b in range(len(lens)) if frames[b]]
    if len(live) >= 2:
        a, b = live[0], live[1]
        if mu_live:                                               # (mu_live = 0: mu is all zeros and so is every F row)
            assert not torch.equal(_bits(ft[int(starts[a])]), _bits(ft[int(starts[b])]))
        if rows:
            assert not torch.equal(_bits(psd[int(starts[a])]), _bits(psd[int(starts[b])]))
    return psd, ft, starts


C3 = lambda **k: dict(dict(n=4096, overlap=0.0, w=2.5, kmax=4), **k)

# name: (MtmParams arguments, frames cap per stream, GLFER_FTEST_PAIRED or None, mu_live)
CASES = {
    "n256_t4": (dict(n=256, overlap=0.0, w=2.5, kmax=3), None, None, True),       # the smallest in-launch size; one sequence per transform
    "n1024_t8": (dict(n=1024, overlap=0.0, w=4.0, kmax=7), None, None, True),     # one sequence per transform
    "n2048_t4": (dict(n=2048, overlap=0.0, w=2.5, kmax=3), None, None, True),     # paired by default
    "C3_paired0": (C3(), None, 0, True),
    "C3_paired1": (C3(), None, 1, True),
    "n16384_t9": (dict(n=16384, overlap=0.0, w=4.5, kmax=8), 6, None, True),
    "n128": (dict(n=128, overlap=0.0, w=2.5, kmax=3), None, None, True),          # stream by stream inside the call
    "C3_mu0": (C3(), None, None, False),
    "C3_mu1": (C3(), None, None, True),
    "C3_sub0": (C3(sub_mean=0), None, None, True),
    "C3_sub1": (C3(sub_mean=1), None, None, True),
    "C3_sub2": (C3(sub_mean=2), None, None, True),
    "C3_overlap_sub1": (C3(overlap=0.5, sub_mean=1), None, None, True),
    "C3_zero_always": (C3(history_mode=1, overlap=0.5, sub_mean=1), None, None, True),
    "C3_s16": (C3(sample_format=1), None, None, True),
    "C3_u8": (C3(sample_format=2), None, None, True),
    "C3_s16_sub1": (C3(sample_format=1, sub_mean=1), None, None, True),
    "C3_pitch": (C3(psd_pitch=2112), None, None, True),
}


@pytest.mark.parametrize("rows", [False, True], ids=["f", "rows_f"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_ragged_ftest_equals_loop(torch_cuda, lib, monkeypatch, name, rows):
    spec, cap, paired, mu_live = CASES[name]
    _select(monkeypatch, paired)
    params = lib.MtmParams(**spec)
    sp = lib.Spectrogram(params)
    lens = lengths(params.n, sp.hop, cap)
    x, offs = layout(torch_cuda, lib, params.sample_format, lens)
    _check(torch_cuda, sp, x, offs, lens, rows, mu_live=mu_live)


@pytest.mark.parametrize("rows", [False, True], ids=["f", "rows_f"])
def test_one_stream_and_one_live_stream(torch_cuda, lib, monkeypatch, rows):
    """nstreams = 1 (the single entry inside the call), and a list in which only one stream has frames (a launch whose other
    workgroups leave at once)"""
    _select(monkeypatch, None)
    for sub in (0, 1):
        sp = lib.Spectrogram(lib.MtmParams(**C3(sub_mean=sub)))
        lens = [9 * sp.hop + 3]
        x, offs = layout(torch_cuda, lib, lib.SAMPLES_F32, lens)
        _check(torch_cuda, sp, x, offs, lens, rows)
        lens = [sp.hop - 1, 0, 5 * sp.hop + 1, 17]
        x, offs = layout(torch_cuda, lib, lib.SAMPLES_F32, lens)
        _check(torch_cuda, sp, x, offs, lens, rows)


@pytest.mark.parametrize("rows", [False, True], ids=["f", "rows_f"])
def test_all_empty(torch_cuda, lib, rows):
    torch = torch_cuda
    sp = lib.Spectrogram(lib.MtmParams(**C3(sub_mean=1)))
    lens = [sp.hop - 1, 0, 17]
    x, offs = layout(torch, lib, lib.SAMPLES_F32, lens)
    _, _, starts = _check(torch, sp, x, offs, lens, rows)
    assert list(starts) == [0, 0, 0, 0]


@pytest.mark.parametrize("name", ["n1024_t8", "C3_sub1", "C3_s16"])
def test_equal_lengths_equal_the_batch_entries(torch_cuda, lib, monkeypatch, name):
    torch = torch_cuda
    _select(monkeypatch, None)
    params = lib.MtmParams(**CASES[name][0])
    sp = lib.Spectrogram(params)
    nb, n = 5, 13 * sp.hop + 2 * (sp.hop // 6)
    pitch = n + 6
    x, _ = layout(torch, lib, params.sample_format, [nb * pitch], gap=0)
    streams = x[:nb * pitch].view(nb, pitch)[:, :n]
    offs, lens = [b * pitch for b in range(nb)], [n] * nb
    want = sp.ftest_batch(streams)
    got, starts = sp.ftest_ragged(x, offs, lens)
    torch.cuda.synchronize()
    assert list(starts) == [13 * b for b in range(nb + 1)]
    assert torch.equal(_bits(got).view(nb, 13, sp.bins), _bits(want))
    want_psd, want_ft = sp.rows_ftest_batch(streams)
    psd, ft, starts = sp.rows_ftest_ragged(x, offs, lens)
    torch.cuda.synchronize()
    assert torch.equal(_bits(ft).view(nb, 13, sp.bins), _bits(want_ft))
    assert torch.equal(_bits(psd).view(nb, 13, sp.pitch), _bits(want_psd))
    assert not torch.equal(_bits(ft[0]), _bits(ft[13]))


@pytest.mark.parametrize("rows", [False, True], ids=["f", "rows_f"])
def test_above_the_grid_y_limit(torch_cuda, lib, monkeypatch, rows):
    """65 537 streams of 1 .. 3 frames at N = 256: two chunks of the grid's y limit (65 535), the second of two streams.  The
    streams around the cut, the last two and a seeded sample against the single entry."""
    torch = torch_cuda
    _select(monkeypatch, None)
    sp = lib.Spectrogram(lib.MtmParams(n=256, overlap=0.0, w=2.0, kmax=2, sub_mean=1))
    nb, hop = 65537, sp.hop
    frames = 1 + (np.arange(nb) * 5) % 3
    lens = frames * hop + (np.arange(nb) % 7)
    offs = np.concatenate(([0], np.cumsum(lens + 1)))[:nb]        # one fill sample between streams
    size = int(offs[-1] + lens[-1])
    g = torch.Generator(device="cuda:0").manual_seed(5)
    x = (torch.rand(size, device="cuda:0", generator=g) - 0.5) * torch.linspace(0.4, 1.0, size, device="cuda:0") \
        + torch.linspace(-0.3, 0.3, size, device="cuda:0")
    total = int(frames.sum())
    ft = torch.full((total + GUARD, sp.bins), SENTINEL, dtype=torch.float32, device="cuda:0")
    if rows:
        psd = torch.full((total + GUARD, sp.pitch), SENTINEL, dtype=torch.float32, device="cuda:0")
        _, _, starts = sp.rows_ftest_ragged(x, offs, lens, out=(psd, ft))
    else:
        _, starts = sp.ftest_ragged(x, offs, lens, out=ft)
    torch.cuda.synchronize()
    assert int(starts[-1]) == total and list(starts[:4]) == [0, 1, 4, 6]
    half = sp.bins - 1
    assert bool(torch.isfinite(ft[:total, 1:half]).all()) and not bool(torch.isfinite(ft[:total, half]).any())
    assert bool((ft[total:] == SENTINEL).all())
    if rows:
        assert bool(torch.isfinite(psd[:total]).all()) and not bool((psd[:total] == SENTINEL).any())
        assert bool((psd[total:] == SENTINEL).all())
    probe = sorted(set([0, 1, 65533, 65534, 65535, 65536, nb - 2, nb - 1]
                       + [int(v) for v in np.random.default_rng(3).integers(0, nb, 64)]))
    for b in probe:
        view = x[int(offs[b]):int(offs[b] + lens[b])]
        r0, r1 = int(starts[b]), int(starts[b + 1])
        if rows:
            want_psd, want_ft = sp.rows_ftest(view)
            torch.cuda.synchronize()
            assert torch.equal(_bits(psd[r0:r1]), _bits(want_psd)), b
        else:
            want_ft = sp.ftest(view)
            torch.cuda.synchronize()
        assert torch.equal(_bits(ft[r0:r1]), _bits(want_ft)), b


@pytest.mark.parametrize("rows", [False, True], ids=["f", "rows_f"])
def test_refuses_a_capturing_stream(torch_cuda, lib, monkeypatch, rows):
    """the tables are uploaded from host memory that is gone after the call: a captured copy would read it at every replay"""
    torch = torch_cuda
    _select(monkeypatch, None)
    sp = lib.Spectrogram(lib.MtmParams(n=1024, overlap=0.0, w=2.5, kmax=3))
    x = torch.from_numpy(np.linspace(-0.5, 0.5, 16 * sp.hop, dtype=np.float32)).to("cuda:0")
    ft = torch.full((8 + GUARD, sp.bins), SENTINEL, dtype=torch.float32, device="cuda:0")
    psd = torch.full((8 + GUARD, sp.pitch), SENTINEL, dtype=torch.float32, device="cuda:0")
    sp.ftest(x[:sp.hop])                                          # (the plan's F tables exist before the capture)
    torch.cuda.synchronize()
    offs, lens = [0, 8 * sp.hop], [4 * sp.hop, 4 * sp.hop]
    run = (lambda: sp.rows_ftest_ragged(x, offs, lens, out=(psd, ft))) if rows else (lambda: sp.ftest_ragged(x, offs, lens, out=ft))
    graph, refused = torch.cuda.CUDAGraph(), False
    with torch.cuda.graph(graph):
        try:
            run()
        except lib.GlferHipError:
            refused = True
    torch.cuda.synchronize()
    assert refused
    assert bool((ft == SENTINEL).all()) and bool((psd == SENTINEL).all())
    run()                                                          # outside a capture: as ever
    torch.cuda.synchronize()
    assert not bool((ft[:8] == SENTINEL).any()) and bool((ft[8:] == SENTINEL).all())
    assert torch.equal(_bits(ft[:4]), _bits(sp.ftest(x[:4 * sp.hop])))


def test_ftest_list_and_rows_ftest_list(torch_cuda, lib, monkeypatch):
    torch = torch_cuda
    _select(monkeypatch, None)
    for fmt in (lib.SAMPLES_F32, lib.SAMPLES_S16):
        sp = lib.Spectrogram(lib.MtmParams(**C3(sample_format=fmt, sub_mean=1)))
        lens = [5 * sp.hop + 1, sp.hop - 1, 9 * sp.hop + 3, 2 * sp.hop + 1]      # odd lengths: the lists keep the offsets even
        x, offs = layout(torch, lib, fmt, lens)
        parts = [x[o:o + n].clone() for o, n in zip(offs, lens)]
        fts = sp.ftest_list(parts)
        pairs = sp.rows_ftest_list(parts)
        torch.cuda.synchronize()
        assert [r.size(0) for r in fts] == [n // sp.hop for n in lens]
        assert [(p.size(0), f.size(0)) for p, f in pairs] == [(n // sp.hop,) * 2 for n in lens]
        for part, f, (p2, f2) in zip(parts, fts, pairs):
            if f.size(0):
                assert torch.equal(_bits(f), _bits(sp.ftest(part)))
                wp, wf = sp.rows_ftest(part)
                assert torch.equal(_bits(f2), _bits(wf)) and torch.equal(_bits(p2), _bits(wp))


def test_argument_order(torch_cuda, lib):
    """the rules of tests/test_ragged_ftest_host.py where a plan always exists, then those that need device memory"""
    torch = torch_cuda
    L = lib.api.lib()
    keep = []

    def plan(params):
        keep.append(lib.Spectrogram(params))
        return keep[-1]._h

    argument_rules(lib, plan)
    # rule 8 with real memory: each missing pointer alone is refused, nothing is written
    sp = lib.Spectrogram(lib.MtmParams(**C3(psd_pitch=2112)))
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    x = torch.zeros(8 * sp.hop, device="cuda:0")
    ft = torch.full((8 + GUARD, sp.bins), SENTINEL, dtype=torch.float32, device="cuda:0")
    psd = torch.full((8 + GUARD, sp.pitch), SENTINEL, dtype=torch.float32, device="cuda:0")
    offs, lens = np.array([0, 4 * sp.hop], np.uint64), np.array([4 * sp.hop, 4 * sp.hop], np.uint64)
    X, F, P = C.c_void_p(x.data_ptr()), C.c_void_p(ft.data_ptr()), C.c_void_p(psd.data_ptr())
    assert call(L, False, sp._h, None, 2, offs, lens, None, F, None, stream=st) == -1
    assert call(L, False, sp._h, X, 2, offs, lens, None, None, None, stream=st) == -1
    assert call(L, True, sp._h, None, 2, offs, lens, P, F, None, stream=st) == -1
    assert call(L, True, sp._h, X, 2, offs, lens, None, F, None, stream=st) == -1
    assert call(L, True, sp._h, X, 2, offs, lens, P, None, None, stream=st) == -1
    # rule 5 before rule 8 with real memory too: 2^31 frames through `lengths` alone
    big = np.array([4 * sp.hop, sp.hop * 2 ** 31], np.uint64)
    assert call(L, True, sp._h, X, 2, offs, big, P, F, None, stream=st) == -1
    torch.cuda.synchronize()
    assert bool((ft == SENTINEL).all()) and bool((psd == SENTINEL).all())
    # (F alone takes no d_psd: the same call with everything it needs goes through)
    assert call(L, False, sp._h, X, 2, offs, lens, None, F, None, stream=st) == 0
    torch.cuda.synchronize()
    assert not bool((ft[:8] == SENTINEL).any()) and bool((ft[8:] == SENTINEL).all())
