"""GPU tests (-m gpu): the two-sided rows of complex I/Q input, Spectrogram.run_iq / run_iq_batch (spectro16c.hip).

Accuracy: every one of the N bins of every frame is held to

    | sqrt(got[k]) - sqrt(exact[k]) |  <=  tau * sqrt( sum_k exact[k] ),    tau = 4 * max(tau_f32, 2**-24)

(tests/_rows_check.py, rule and margin as in tests/test_gpu_rows.py) with `exact` the float64 rows of tests/_iq_exact.py and tau_f32
what its float32 stand-in reaches, computed on the CPU per case and never from device output.  The cases are tests/_iq_cases.py's;
tests/test_iq_criterion.py shows without a GPU that the rule rejects mirrored, shifted, swapped, I-only and taper-short rows.
Orientation: exp(+2 pi i k0 n / N) lands in column k0 (or (k0 + N/2) mod N with centered=True) with P = N.
Bit for bit (torch.equal on the int32 view): batches against the loop of single calls, frame ranges against the whole run,
centered against torch.roll, swap against the exchanged copy, a pitched `out` against the dense one; padding and guard regions
keep their bytes.  The refusals of tests/test_iq_host.py's helper with real plans; one graph capture and replay.

Lines starting with 'iq-rows' (run with -s) are the record kept in profiles/iq_rows.txt.
"""
import numpy as np
import pytest

import _iq_cases as Q
import _iq_exact as XC
from _rows_check import bound, check_rows, tau_of
from test_iq_host import device_entry_refusals

pytestmark = pytest.mark.gpu
SENTINEL = -7.25


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _plan(lib, c):
    fmt = {"f32": lib.SAMPLES_F32, "s16": lib.SAMPLES_S16, "u8": lib.SAMPLES_U8}[c.fmt]
    if c.est == "fft":
        return lib.Spectrogram(lib.FftParams(n=c.n, window_type=lib.WINDOWS[c.window], overlap=c.ovl, history_mode=c.history_mode,
                                             sample_format=fmt))
    return lib.Spectrogram(lib.MtmParams(n=c.n, overlap=c.ovl, w=c.nw, kmax=c.kmax, history_mode=c.history_mode, sample_format=fmt))


def _bits(x):
    import torch
    return x.contiguous().view(torch.int32)


def _same(a, b):
    import torch
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


# ---- accuracy, bin by bin -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", Q.CASES, ids=Q.case_id)
def test_rows_bin_by_bin(lib, oracle, torch_cuda, c):
    torch = torch_cuda
    r = Q.reference(oracle, c)
    sp = _plan(lib, c)
    assert np.array_equal(sp.window(), oracle.window(oracle.WINDOWS[c.window], c.n)) if c.est == "fft" else True
    if c.fmt == "f32":                                           # complex64 [S]: the same bytes as the [S, 2] float32 pairs
        d = torch.from_numpy(r.z).cuda()
        assert np.array_equal(r.z.view(np.float32).reshape(-1, 2), r.raw)
    else:
        d = torch.from_numpy(r.raw).cuda()
    got = sp.run_iq(d).cpu().numpy()
    sp.close()
    assert got.shape == (c.frames, c.n) and got.dtype == np.float32
    dev = tau_of(got, r.exact)
    print("iq-rows %-52s device tau %.3e bound %.3e fraction %.3f tau_f32 %.3e" % (Q.case_id(c), dev, r.tau, dev / r.tau, r.tau_f32))
    check_rows(got, r.exact, r.tau, Q.case_id(c))
    if c.signal == "zero":
        assert not r.exact.any() and not got.any()               # silence: exactly zero rows


# ---- orientation --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,k0", [(256, 3), (256, 256 - 5), (1024, 1024 - 200), (4096, 77), (4096, 4096 - 1), (16384, 5000), (16384, 16384 - 3000)])
def test_tone_lands_in_its_own_bin(lib, torch_cuda, n, k0):
    torch = torch_cuda
    frames = 3
    t = np.arange(frames * n, dtype=np.float64)
    z = np.exp(2j * np.pi * ((k0 * t) % n) / n).astype(np.complex64)
    ones = np.ones(n, np.float32)
    exact = XC.periodogram64(z, n, 0.0, ones)
    tau = bound(tau_of(XC.periodogram32(z, n, 0.0, ones), exact))
    sp = lib.Spectrogram(lib.FftParams(n=n, window_type=lib.WINDOWS["rectangular"], overlap=0.0))
    d = torch.from_numpy(z).cuda()
    nat = sp.run_iq(d)
    cen = sp.run_iq(d, centered=True)
    sp.close()
    got = nat.cpu().numpy()
    check_rows(got, exact, tau, "tone n=%d k0=%d" % (n, k0))      # every other bin is under the rule's bound
    assert (np.argmax(got, axis=1) == k0).all()
    assert np.abs(got[:, k0] / n - 1.0).max() <= 3 * tau           # P[k0] = N to rounding
    assert (np.argmax(cen.cpu().numpy(), axis=1) == (k0 + n // 2) % n).all()
    assert _same(cen, torch.roll(nat, n // 2, dims=-1))


# ---- bit for bit --------------------------------------------------------------------------------------------------------
BIT_CASES = [Q.fft(4096, 0.75, "hanning", 23, "noise"), Q.mtm(1024, 0.5, 2.5, 4, 37, "noise", "s16"),
             Q.fft(256, 0.3, "hanning", 37, "noise", "u8", 1), Q.mtm(16384, 0.5, 2.0, 1, 6, "noise")]
bit_cases = pytest.mark.parametrize("c", BIT_CASES, ids=Q.case_id)


def _device_input(torch, c):
    raw, _ = Q.make_input(c)
    return torch.from_numpy(raw).cuda()


@bit_cases
def test_batch_equals_loop_of_single_calls(lib, torch_cuda, c):
    """B = 1, 2 and 5; streams a pitch larger than S apart; overlapping streams cut from one buffer."""
    torch = torch_cuda
    sp = _plan(lib, c)
    hop = sp.hop
    S = c.frames * hop
    big = _device_input(torch, c._replace(frames=c.frames + 12))          # [S + 12 hops (+3)][2]
    for B in (1, 2, 5):
        pitched = torch.zeros((B, S + 5 * hop + 3, 2), dtype=big.dtype, device="cuda")
        for b in range(B):
            pitched[b, :S] = big[b * hop:b * hop + S]
        views = [pitched[:, :S], big.as_strided((B, S, 2), (3 * hop * 2, 2, 1))]
        for v in views:
            got = sp.run_iq_batch(v)
            assert got.shape == (B, c.frames, c.n)
            for b in range(B):
                assert _same(got[b], sp.run_iq(v[b])), (B, b)
            flagged = sp.run_iq_batch(v, first_frame=2, nframes=c.frames - 3, centered=True, swap=True)
            for b in range(B):
                assert _same(flagged[b], sp.run_iq(v[b], first_frame=2, nframes=c.frames - 3, centered=True, swap=True)), (B, b)
    sp.close()


def test_batch_sharing_the_grid_equals_single_calls(lib, torch_cuda):
    """N = 16384: a launch keeps 1024 workgroups for all its streams, so five streams of 300 frames walk their frames in the
    persistent loop (200 workgroups each) while a single call has a workgroup per frame."""
    torch = torch_cuda
    c = Q.fft(16384, 0.75, "hanning", 300 + 4 * 3, "noise")
    sp = _plan(lib, c)
    big = _device_input(torch, c)
    S = 300 * sp.hop
    v = big.as_strided((5, S, 2), (3 * sp.hop * 2, 2, 1))
    got = sp.run_iq_batch(v)
    for b in range(5):
        assert _same(got[b], sp.run_iq(v[b])), b
    sp.close()


@bit_cases
def test_frame_ranges_equal_the_whole_run(lib, torch_cuda, c):
    torch = torch_cuda
    sp = _plan(lib, c)
    d = _device_input(torch, c)
    whole = sp.run_iq(d)
    cuts = [0, 1, 3, c.frames // 2 + 1, c.frames - 1, c.frames]
    for a, b in zip(cuts, cuts[1:]):
        assert _same(sp.run_iq(d, first_frame=a, nframes=b - a), whole[a:b]), (a, b)
    assert sp.run_iq(d, first_frame=c.frames, nframes=0).shape == (0, c.n)
    sp.close()


@bit_cases
def test_centered_and_swap(lib, torch_cuda, c):
    torch = torch_cuda
    sp = _plan(lib, c)
    d = _device_input(torch, c)
    nat = sp.run_iq(d)
    assert _same(sp.run_iq(d, centered=True), torch.roll(nat, c.n // 2, dims=-1))
    exchanged = d.flip(-1).contiguous()                                   # Q, I, Q, I ... in memory
    assert not torch.equal(exchanged, d)
    sw = sp.run_iq(d, swap=True)
    assert _same(sw, sp.run_iq(exchanged)) and not _same(sw, nat)
    assert _same(sp.run_iq(exchanged, swap=True), nat)
    assert _same(sp.run_iq(d, centered=True, swap=True), torch.roll(sw, c.n // 2, dims=-1))
    sp.close()


@bit_cases
def test_pitched_out_and_guards(lib, torch_cuda, c):
    """A pitched `out`: the same bins, the padding keeps its bytes; guard regions before and after d_psd keep theirs."""
    torch = torch_cuda
    sp = _plan(lib, c)
    d = _device_input(torch, c)
    dense = sp.run_iq(d)
    pitch, guard = c.n + 24, 4096
    buf = torch.full((guard + c.frames * pitch + guard,), SENTINEL, dtype=torch.float32, device="cuda")
    rows = buf[guard:guard + c.frames * pitch].view(c.frames, pitch)
    for kw in ({}, {"centered": True}):
        buf.fill_(SENTINEL)
        out = sp.run_iq(d, out=rows[:, :c.n], **kw)
        assert out.data_ptr() == rows.data_ptr()
        want = torch.roll(dense, c.n // 2, dims=-1) if kw else dense
        assert _same(rows[:, :c.n], want)
        assert bool((rows[:, c.n:] == SENTINEL).all())
        assert bool((buf[:guard] == SENTINEL).all()) and bool((buf[guard + c.frames * pitch:] == SENTINEL).all())
    # dense rows between guards, single and batch
    buf.fill_(SENTINEL)
    tight = buf[guard:guard + c.frames * c.n].view(c.frames, c.n)
    sp.run_iq(d, out=tight)
    assert _same(tight, dense)
    assert bool((buf[:guard] == SENTINEL).all()) and bool((buf[guard + c.frames * c.n:] == SENTINEL).all())
    two = torch.full((guard + 2 * c.frames * pitch + guard,), SENTINEL, dtype=torch.float32, device="cuda")
    brows = two[guard:guard + 2 * c.frames * pitch].view(2, c.frames, pitch)
    sp.run_iq_batch(torch.stack([d, d]), out=brows[:, :, :c.n])
    assert _same(brows[0, :, :c.n], dense) and _same(brows[1, :, :c.n], dense)
    assert bool((brows[:, :, c.n:] == SENTINEL).all())
    assert bool((two[:guard] == SENTINEL).all()) and bool((two[guard + 2 * c.frames * pitch:] == SENTINEL).all())
    sp.close()


# ---- refusals, graph capture -----------------------------------------------------------------------------------------------
def test_device_entry_refusals_with_real_plans(lib, torch_cuda):
    assert device_entry_refusals(lib) == 11


def test_wrapper_refuses_wrong_inputs(lib, torch_cuda):
    torch = torch_cuda
    sp = lib.Spectrogram(lib.FftParams(n=1024, window_type=0, overlap=0.5, sample_format=lib.SAMPLES_S16))
    good = torch.zeros((4096, 2), dtype=torch.int16, device="cuda")
    assert sp.run_iq(good).shape == (8, 1024)
    for bad in (torch.zeros((4096, 2), dtype=torch.float32, device="cuda"), torch.zeros(4096, dtype=torch.complex64, device="cuda"),
                torch.zeros((4096, 3), dtype=torch.int16, device="cuda"), torch.zeros(8192, dtype=torch.int16, device="cuda"),
                torch.zeros((4096, 4), dtype=torch.int16, device="cuda")[:, ::2]):
        with pytest.raises(AssertionError):
            sp.run_iq(bad)
    with pytest.raises(lib.GlferHipError):
        sp.run_iq(good, first_frame=6, nframes=3)                         # a frame past the stream
    sp.close()
    mean = lib.Spectrogram(lib.FftParams(n=1024, window_type=0, overlap=0.5, sub_mean=1))
    with pytest.raises(lib.GlferHipError):
        mean.run_iq(torch.zeros(4096, dtype=torch.complex64, device="cuda"))
    mean.close()


def test_graph_capture_and_replay(lib, oracle, torch_cuda):
    """One capture of run_iq on a non-default stream, replayed: the eager rows."""
    torch = torch_cuda
    c = Q.mtm(4096, 0.5, 2.5, 4, 7, "weak", "f32", 1)
    r = Q.reference(oracle, c)
    sp = _plan(lib, c)
    d = torch.from_numpy(r.z).cuda()
    eager = sp.run_iq(d)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    out = torch.full((c.frames, c.n), SENTINEL, dtype=torch.float32, device="cuda")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        sp.run_iq(d, out=out)
    torch.cuda.synchronize()
    out.fill_(SENTINEL)
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    assert _same(out, eager)
    check_rows(out.cpu().numpy(), r.exact, r.tau, "graph replay")
    sp.close()
