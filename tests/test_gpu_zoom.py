"""GPU tests (-m gpu): Spectrogram.run_zoom, the two-sided rows of the down-converter's output (glfer_hip_spectrogram_zoom_device).

Bit for bit (int32 views): run_zoom against run_iq(ddc.run(x)), frame ranges and centered included, for a periodogram plan and a
multitaper plan at N = 256.  Orientation: two real tones 3 / (D N) cycles apart around the zoom frequency land in columns N/2 and
N/2 + 3 of the centred rows.  Accuracy: every bin of those rows under the I/Q rule of tests/_rows_check.py against
_iq_exact.periodogram64 of the float64 down-converter output, tau_f32 from the float32 stand-ins of both stages in a row.

The matrix of tests/_zoom_cases.py (every N = 256 .. 16384 and so every compile and prefetch scheme of spectro16c.hip, eight (D, T)
shapes, the six input kinds, both history modes, hops of N, N/2, N/4 and 0.7 N, two pieces 2^36 samples into a stream): every bin
of every frame is held to

    | sqrt(got[k]) - sqrt(exact[k]) |  <=  tau * sqrt( sum_k exact[k] ),    tau = 4 * max(tau_f32, 2**-24)

with `exact` float64 through both stages and tau_f32 the larger of the two float32 stand-ins (the converter summed in tap order and
in ddc.hip's row order), computed on the CPU and never from device output; tests/test_zoom_criterion.py shows without a GPU what the
rule accepts and rejects.  `line` scenes: the largest bin of every settled frame is the weak line's.  The same call is bit equal to
the two separate calls (the far pieces: both C entries on virtual bases); once per N, centered, a pitched `out` between sentinels and
frame ranges from 0, from the first frame whose `lo` is positive and from the last.  The three routes of the stream-ordered scratch
(small pool, hipMallocAsync, a kept block) back to back and on a side stream; the entry's refusals with real handles.

Lines starting with 'zoom-rows' (run with -s) are the record kept in profiles/zoom_rows.txt.
"""
import ctypes as C

import numpy as np
import pytest

import _ddc_exact as X
import _iq_exact as XC
import _zoom_cases as Z
from _rows_check import bound, check_rows, tau_of

pytestmark = pytest.mark.gpu
D, N = 16, 256


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _same(a, b):
    import torch
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("est", ["fft", "mtm"])
def test_zoom_equals_iq_rows_of_the_ddc_output(lib, torch_cuda, est):
    torch = torch_cuda
    if est == "fft":
        sp = lib.Spectrogram(lib.FftParams(n=N, window_type=lib.WINDOWS["hanning"], overlap=0.5))
    else:
        sp = lib.Spectrogram(lib.MtmParams(n=N, overlap=0.75, w=2.5, kmax=4))
    frames = 21
    rng = np.random.default_rng(5)
    x = torch.from_numpy((0.25 * rng.standard_normal(frames * sp.hop * D + D // 2 + 1)).astype(np.float32)).cuda()
    ddc = lib.Ddc(D, 0.1234567)
    base = ddc.run(x)
    assert base.shape == (frames * sp.hop,)
    want = sp.run_iq(base)
    assert want.shape == (frames, N)
    assert _same(sp.run_zoom(ddc, x), want)
    assert _same(sp.run_zoom(ddc, x, centered=True), sp.run_iq(base, centered=True))
    cuts = [0, 1, 3, 11, frames - 1, frames]
    for a, b in zip(cuts, cuts[1:]):
        assert _same(sp.run_zoom(ddc, x, first_frame=a, nframes=b - a), want[a:b]), (a, b)
        assert _same(sp.run_zoom(ddc, x, first_frame=a, nframes=b - a, centered=True), torch.roll(want[a:b], N // 2, dims=-1)), (a, b)
    pitched = torch.full((frames, N + 24), -7.25, dtype=torch.float32, device="cuda")
    sp.run_zoom(ddc, x, out=pitched[:, :N])
    assert _same(pitched[:, :N], want) and bool((pitched[:, N:] == -7.25).all())
    assert sp.run_zoom(ddc, x, first_frame=frames, nframes=0).shape == (0, N)
    with pytest.raises(lib.GlferHipError):
        sp.run_zoom(ddc, x, first_frame=frames, nframes=1)           # a frame past the baseband
    s16 = lib.Spectrogram(lib.FftParams(n=N, window_type=0, overlap=0.5, sample_format=lib.SAMPLES_S16))
    with pytest.raises(lib.GlferHipError):
        s16.run_zoom(ddc, x)                                         # the baseband is f32: the plan must be
    s16.close()
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    out = torch.empty((frames, N), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.graph(graph, stream=side):
        with pytest.raises(lib.GlferHipError):
            sp.run_zoom(ddc, x, out=out)                             # documented: a captured stream is refused
        base.add_(0)                                                 # (a capture must record something)
    torch.cuda.synchronize()
    ddc.close()
    sp.close()


def test_two_tones_land_in_their_own_columns(lib, torch_cuda):
    torch = torch_cuda
    frames, fc = 3, 0.1234567
    ns = frames * N * D
    t = np.arange(ns, dtype=np.float64)
    f1, f2 = fc, fc + 3.0 / (D * N)
    x = (0.4 * np.cos(2 * np.pi * f1 * t + 0.3) + 0.3 * np.cos(2 * np.pi * f2 * t + 1.1)).astype(np.float32)
    sp = lib.Spectrogram(lib.FftParams(n=N, window_type=lib.WINDOWS["rectangular"], overlap=0.0))
    ddc = lib.Ddc(D, fc)
    got = sp.run_zoom(ddc, torch.from_numpy(x).cuda(), centered=True).cpu().numpy()
    assert got.shape == (frames, N)
    top2 = np.sort(np.argsort(got, axis=1)[:, -2:], axis=1)
    assert (top2 == np.array([N // 2, N // 2 + 3])).all(), top2
    # every bin, against float64 all the way: the exact DDC output, its exact periodogram
    W = X.phase_word(fc)
    g = X.tables(W, ddc.taps)
    assert np.array_equal(g.view(np.int32), ddc.tables().view(np.int32))
    nout = ns // D
    y64, _ = X.exact(x.astype(np.complex64), g, W, D, 0, nout)
    y32 = X.standin32(x.astype(np.complex64), g, W, D, 0, nout)
    ones = np.ones(N, np.float32)
    exact = np.roll(XC.periodogram64(y64, N, 0.0, ones), N // 2, axis=1)
    f32 = np.roll(XC.periodogram32(y32, N, 0.0, ones), N // 2, axis=1)
    tau_f32 = tau_of(f32, exact)
    tau = bound(tau_f32)
    frac = check_rows(got, exact, tau, "zoom two tones")
    print("ddc-rows zoom D%d N%d two tones: fraction %.3f of the bound, tau_f32 %.3e" % (D, N, frac, tau_f32))
    ddc.close()
    sp.close()


# ---- the matrix: every bin under the rule, bit equality with the two separate calls ---------------------------------------------------
SENTINEL = -7.25
ESZ = {"f32": 4, "s16": 2, "u8": 1}
EXTRAS = {min((i for i, c in enumerate(Z.CASES) if c.n == n and c.first == 0)) for n in {c.n for c in Z.CASES}}   # once per N


def _handles(lib, c, taps):
    fmt = {"f32": lib.SAMPLES_F32, "s16": lib.SAMPLES_S16, "u8": lib.SAMPLES_U8}[c.fmt]
    ddc = lib.Ddc(c.D, c.freq, taps=taps, complex_in=bool(c.cplx), sample_format=fmt)
    if c.est == "fft":
        sp = lib.Spectrogram(lib.FftParams(n=c.n, window_type=lib.WINDOWS[c.window], overlap=c.ovl, history_mode=c.history_mode))
    else:
        sp = lib.Spectrogram(lib.MtmParams(n=c.n, overlap=c.ovl, w=c.nw, kmax=c.kmax, history_mode=c.history_mode))
    return ddc, sp


def _far(lib, torch, c, ddc, sp, d, centered=False):
    """A piece far into a stream through the C entries: (zoom rows, rows of the two separate calls, the baseband of the first)."""
    L = lib.api.lib()
    lo, hi = Z.lo_hi(c)
    ns, pitch, guard = Z.nsamples_of(c), c.n + 24, 64
    vin = (d.data_ptr() - Z.base_of(c) * ESZ[c.fmt] * (2 if c.cplx else 1)) % (1 << 64)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    flags = lib.api.IQ_CENTERED if centered else 0
    bufs = [torch.full((guard + c.frames * pitch + guard,), SENTINEL, dtype=torch.float32, device="cuda") for _ in range(2)]
    rows = [b[guard:guard + c.frames * pitch].view(c.frames, pitch) for b in bufs]
    rc = L.glfer_hip_spectrogram_zoom_device(sp._h, ddc._h, C.c_void_p(vin), ns, c.first, c.frames, C.c_void_p(rows[0].data_ptr()), pitch,
                                             flags, st)
    assert rc == 0, rc
    base = torch.full((hi - lo + 16,), complex(SENTINEL, 3.5), dtype=torch.complex64, device="cuda")
    rc = L.glfer_hip_ddc_device(ddc._h, C.c_void_p(vin), ns, lo, hi - lo, C.c_void_p(base[8:].data_ptr()), st)
    assert rc == 0, rc
    vbase = (base[8:].data_ptr() - lo * 8) % (1 << 64)
    rc = L.glfer_hip_spectrogram_iq_device(sp._h, C.c_void_p(vbase), ns // c.D, c.first, c.frames, C.c_void_p(rows[1].data_ptr()), pitch, flags, st)
    assert rc == 0, rc
    torch.cuda.synchronize()
    for b, r in zip(bufs, rows):
        assert bool((r[:, c.n:] == SENTINEL).all()) and bool((b[:guard] == SENTINEL).all()) and bool((b[-guard:] == SENTINEL).all())
    assert bool((base[:8] == complex(SENTINEL, 3.5)).all()) and bool((base[8 + hi - lo:] == complex(SENTINEL, 3.5)).all())
    return rows[0][:, :c.n], rows[1][:, :c.n], base[8:8 + hi - lo]


def _extras(torch, c, ddc, sp, d, want):
    """Once per N: centered against torch.roll, a pitched `out` between sentinels, frame ranges from 0, from the first frame whose
    baseband range starts above sample 0, and from the last frame."""
    n, h = c.n, Z.hop(c)
    assert _same(sp.run_zoom(ddc, d, centered=True), torch.roll(want, n // 2, dims=-1))
    pitch, guard = n + 24, 4096
    buf = torch.full((guard + c.frames * pitch + guard,), SENTINEL, dtype=torch.float32, device="cuda")
    rows = buf[guard:guard + c.frames * pitch].view(c.frames, pitch)
    out = sp.run_zoom(ddc, d, out=rows[:, :n])
    assert out.data_ptr() == rows.data_ptr() and _same(rows[:, :n], want)
    assert bool((rows[:, n:] == SENTINEL).all()) and bool((buf[:guard] == SENTINEL).all()) and bool((buf[-guard:] == SENTINEL).all())
    positive = next(f for f in range(c.frames + 1) if f * h > n - h)
    assert 0 < positive < c.frames, "the case must hold a frame whose lo is positive"
    for a in (0, positive, c.frames - 1):
        k = min(2, c.frames - a)
        assert _same(sp.run_zoom(ddc, d, first_frame=a, nframes=k), want[a:a + k]), (a, k)
        assert _same(sp.run_zoom(ddc, d, first_frame=a, nframes=k, centered=True), torch.roll(want[a:a + k], n // 2, dims=-1)), (a, k)


@pytest.mark.parametrize("i", range(len(Z.CASES)), ids=[Z.case_id(c) for c in Z.CASES])
def test_rows_under_the_rule(lib, oracle, torch_cuda, i):
    torch = torch_cuda
    c = Z.CASES[i]
    r = Z.reference(oracle, c)
    ddc, sp = _handles(lib, c, r.taps)
    assert ddc.phase_word == r.W
    assert np.array_equal(ddc.tables().view(np.int32), r.g.view(np.int32))
    if c.est == "fft":
        assert np.array_equal(sp.window(), oracle.window(oracle.WINDOWS[c.window], c.n))    # (rectangular: a table no frame is multiplied with)
    d = torch.from_numpy(np.array(r.raw)).cuda()
    if c.first == 0:
        rows = sp.run_zoom(ddc, d)
        base = ddc.run(d)
        assert base.shape == (len(r.raw) // c.D,) and len(r.raw) // c.D // sp.hop == c.frames
        apart = sp.run_iq(base)
        base = base[:Z.lo_hi(c)[1]]
    else:
        rows, apart, base = _far(lib, torch, c, ddc, sp, d)
        cen, cen_apart, _ = _far(lib, torch, c, ddc, sp, d, centered=True)
        assert _same(cen, cen_apart) and _same(cen, torch.roll(rows, c.n // 2, dims=-1))
    got = rows.cpu().numpy()
    assert got.shape == (c.frames, c.n) and got.dtype == np.float32
    dev = tau_of(got, r.exact)
    first_stage = tau_of(Z.rows64(oracle, c, base.cpu().numpy()), r.exact)      # float64 rows of the device's own baseband
    print("zoom-rows %-64s device tau %.3e bound %.3e fraction %.3f tau_f32(taps) %.3e tau_f32(rows) %.3e | converter alone (float64 rows of "
          "its output) %.3e" % (Z.case_id(c), dev, r.tau, dev / r.tau, r.tau_taps, r.tau_rows, first_stage))
    check_rows(got, r.exact, r.tau, Z.case_id(c))
    if c.scene == "zero":
        assert not r.exact.any() and not got.any()
    if c.scene == "line":
        k = np.arange(c.n)
        dist = np.abs((k - Z.line_bin(c) + c.n // 2) % c.n - c.n // 2)
        for f in Z.settled_frames(c):
            assert dist[int(np.argmax(got[f]))] <= (np.ceil(c.nw) if c.est == "mtm" else 0), (f, int(np.argmax(got[f])), Z.line_bin(c))
    assert _same(rows, apart)                                                    # the two separate calls on the same input
    if i in EXTRAS:
        _extras(torch, c, ddc, sp, d, apart)
    ddc.close()
    sp.close()


# ---- the scratch routes -------------------------------------------------------------------------------------------------------------------
ROUTES = {"small-pool": (256, 37), "malloc-async": (16384, 16), "kept-block": (16384, (1 << 21) // 16384 + 1)}


@pytest.mark.parametrize("route", list(ROUTES))
def test_scratch_routes(lib, torch_cuda, route):
    """The mixer (D = 1, one tap) on real f32 input and a rectangular periodogram plan without overlap: the baseband is as long as the
    input, under 1 MiB, between 1 and 16 MiB, and above 16 MiB (2^21 + a hop complex outputs)."""
    torch = torch_cuda
    L = lib.api.lib()
    n, frames = ROUTES[route]
    nbytes = frames * n * 8
    assert {"small-pool": nbytes < 1 << 20, "malloc-async": 1 << 20 <= nbytes < 16 << 20, "kept-block": nbytes >= 16 << 20}[route]
    sp = lib.Spectrogram(lib.FftParams(n=n, window_type=lib.WINDOWS["rectangular"], overlap=0.0))
    ddc = lib.Ddc(1, 0.1234567, taps=np.ones(1, np.float32))
    rng = np.random.default_rng(n + frames)
    xs = [torch.from_numpy((0.25 * rng.standard_normal(frames * n + 1)).astype(np.float32)).cuda() for _ in range(2)]
    assert not torch.equal(xs[0], xs[1])
    dev = torch.cuda.current_device()
    torch.cuda.synchronize()
    before = L.glfer_hip_scratch_held(dev)
    got = [sp.run_zoom(ddc, xs[0])]                                              # two calls back to back, nothing synchronised between
    held_first = L.glfer_hip_scratch_held(dev)
    got.append(sp.run_zoom(ddc, xs[1]))
    held_second = L.glfer_hip_scratch_held(dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got += [sp.run_zoom(ddc, xs[0]), sp.run_zoom(ddc, xs[1])]
    held_side = L.glfer_hip_scratch_held(dev)
    torch.cuda.synchronize()
    if route == "kept-block":                                                    # the second call took the block the first gave back
        assert held_first >= nbytes and held_second == held_first and held_side == held_first
    else:
        assert held_first == held_second == held_side == before
    want = [sp.run_iq(ddc.run(x)) for x in xs]
    assert want[0].shape == (frames, n) and not _same(want[0], want[1])
    for j, g in enumerate(got):
        assert _same(g, want[j % 2]), (route, j)
    torch.cuda.synchronize()
    L.glfer_hip_scratch_trim(dev, 0)                                             # the module leaves nothing kept
    assert L.glfer_hip_scratch_held(dev) == 0
    ddc.close()
    sp.close()


# ---- the entry's refusals -------------------------------------------------------------------------------------------------------------------
def test_entry_refusals(lib, torch_cuda):
    """Real handles, and only arguments the entry turns down before it takes scratch or launches anything: the buffers are fake
    addresses."""
    L = lib.api.lib()
    zoom = L.glfer_hip_spectrogram_zoom_device
    OK, E_ARG = 0, -1
    n, D = 256, 16
    sp = lib.Spectrogram(lib.FftParams(n=n, window_type=lib.WINDOWS["rectangular"], overlap=0.5))
    ddc = lib.Ddc(D, 0.1234567)
    h = sp.hop
    ns = 10 * h * D + 3                                                          # a baseband of ten hops
    fake, out = C.c_void_p(0x10000), C.c_void_p(0x4000000)
    p, q = sp._h, ddc._h
    assert zoom(p, q, None, ns, 0, 0, None, 0, 0, None) == OK                    # no frames: nothing to do, every pointer null
    assert zoom(p, q, None, ns, 99, 0, None, n + 8, lib.api.IQ_CENTERED, None) == OK
    assert zoom(None, q, fake, ns, 0, 4, out, 0, 0, None) == E_ARG
    assert zoom(p, None, fake, ns, 0, 4, out, 0, 0, None) == E_ARG
    others = [lib.FftParams(n=n, window_type=0, overlap=0.5, sample_format=lib.SAMPLES_S16),      # the baseband is f32: the plan must be
              lib.FftParams(n=n, window_type=0, overlap=0.5, sample_format=lib.SAMPLES_U8),
              lib.FftParams(n=128, window_type=0, overlap=0.5),                                    # no I/Q rows at this N
              lib.FftParams(n=n, window_type=0, overlap=0.5, sub_mean=1)]                          # nor with mean removal
    for params in others:
        bad = lib.Spectrogram(params)
        assert zoom(bad._h, q, fake, 10 * bad.hop * D, 0, 4, out, 0, 0, None) == E_ARG, params.__dict__
        assert zoom(bad._h, q, None, 10 * bad.hop * D, 0, 0, None, 0, 0, None) == E_ARG           # (refused even with no work)
        bad.close()
    for flags in (lib.api.IQ_SWAP, lib.api.IQ_SWAP | lib.api.IQ_CENTERED, 4, 0x80000000):        # the converter has no swapped output
        assert zoom(p, q, fake, ns, 0, 4, out, 0, flags, None) == E_ARG, flags
    for pitch in (1, n - 1, n // 2 + 1):                                         # a pitch below N
        assert zoom(p, q, fake, ns, 0, 4, out, pitch, 0, None) == E_ARG, pitch
    assert zoom(p, q, fake, ns, 7, 4, out, 0, 0, None) == E_ARG                  # first + nframes past nbase / H
    assert zoom(p, q, fake, ns, 10, 1, out, 0, 0, None) == E_ARG
    assert zoom(p, q, fake, ns + (h - 1) * D - 3, 10, 1, out, 0, 0, None) == E_ARG       # (a sample short of an eleventh hop)
    assert zoom(p, q, fake, ns, 2 ** 64 - 2, 4, out, 0, 0, None) == E_ARG        # ... and the same wrapping size_t
    assert zoom(p, q, fake, 2 ** 33 * h * D, 0, 2 ** 31, out, 0, 0, None) == E_ARG       # nframes above 2^31 - 1
    many = (1 << 31) // h + 1                                                    # a frame range whose baseband passes 2^31 - 1 outputs
    assert many <= 0x7fffffff and many * h - 0 > 0x7fffffff
    assert zoom(p, q, fake, 2 ** 33 * h * D, 0, many, out, 0, 0, None) == E_ARG
    assert zoom(p, q, fake, 2 ** 33 * h * D, 5, many, out, 0, 0, None) == E_ARG
    assert zoom(p, q, None, ns, 0, 4, out, 0, 0, None) == E_ARG                  # null buffers while there is work
    assert zoom(p, q, fake, ns, 0, 4, None, 0, 0, None) == E_ARG
    ddc.close()
    sp.close()
