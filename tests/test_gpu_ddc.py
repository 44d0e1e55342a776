"""GPU tests (-m gpu): the digital down-converter, Ddc.run / run_batch (ddc.hip).

Accuracy: every output of every case of tests/_ddc_cases.py is held to

    | got[m] - exact[m] |  <=  tau * A[m],   A[m] = sum_t |g[t]| |x[n0 - t]|,   tau = 4 * max(tau_f32, 2**-24)

with `exact` the float64 definition of tests/_ddc_exact.py and tau_f32 what its float32 stand-in reaches, computed on the CPU per
case and never from device output (tests/test_ddc_criterion.py shows without a GPU what the rule rejects).  Every case is passed as a
piece by its virtual base, so the cases far into a stream (first_out near 2^36 / D) need no large memory.
Bit for bit (int32 views), guard regions keeping their sentinel: output ranges against the whole run with cuts inside and on tile
boundaries, batches of 1, 2 and 5 against the loop of single calls (pitched and overlapping streams), a pitched `out`, real s16 / u8
streams at odd element offsets against aligned copies.  Streams shorter than the filter and shorter than the step; the refusals of
tests/test_ddc_host.py's helper with real handles; one graph capture and replay.

Lines starting with 'ddc-rows' (run with -s) are the record kept in profiles/ddc_rows.txt.
"""
import ctypes as C

import numpy as np
import pytest

import _ddc_cases as Q
import _ddc_exact as X
from test_ddc_host import device_entry_refusals

pytestmark = pytest.mark.gpu
SENTINEL = complex(-7.25, 3.5)
ESZ = {"f32": 4, "s16": 2, "u8": 1}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _fmt(lib, c):
    return {"f32": lib.SAMPLES_F32, "s16": lib.SAMPLES_S16, "u8": lib.SAMPLES_U8}[c.fmt]


def _ddc(lib, c, taps=None):
    return lib.Ddc(c.D, c.freq, taps=X.design(c.D, c.T) if taps is None else taps, complex_in=bool(c.cplx), sample_format=_fmt(lib, c))


def _bits(x):
    import torch
    return torch.view_as_real(x.contiguous()).view(torch.int32)


def _same(a, b):
    import torch
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _kept(t):
    return bool((t == SENTINEL).all())


def _run_piece(lib, torch, ddc, c, d_piece):
    """The case's outputs through the C entry, the piece passed by its virtual base (the address sample 0 would have)."""
    out = torch.full((c.nout + 16,), SENTINEL, dtype=torch.complex64, device="cuda")
    esz = ESZ[c.fmt] * (2 if c.cplx else 1)
    base = (d_piece.data_ptr() - Q.base_of(c) * esz) % (1 << 64)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = lib.api.lib().glfer_hip_ddc_device(ddc._h, C.c_void_p(base), Q.nsamples_of(c), c.first, c.nout, C.c_void_p(out[8:].data_ptr()), st)
    assert rc == 0, rc
    torch.cuda.synchronize()
    guard = torch.cat([out[:8], out[8 + c.nout:]])
    assert _kept(guard)
    return out[8:8 + c.nout]


# ---- accuracy, output by output ----------------------------------------------------------------------------------------------
WORST = {}


@pytest.mark.parametrize("c", Q.CASES, ids=Q.case_id)
def test_outputs_under_the_rule(lib, torch_cuda, c):
    torch = torch_cuda
    r = Q.reference(c)
    ddc = _ddc(lib, c, r.taps)
    assert ddc.phase_word == r.W
    assert np.array_equal(ddc.tables().view(np.int32), r.g.view(np.int32))
    d = torch.from_numpy(np.array(r.raw)).cuda()
    got = _run_piece(lib, torch, ddc, c, d)
    if c.first == 0:                                             # the wrapper, on the stream itself (D = 1: its tail is an output more)
        assert ddc.num_out(len(r.raw)) == len(r.raw) // c.D >= c.nout
        assert _same(ddc.run(d)[:c.nout], got)
    ddc.close()
    y = got.cpu().numpy()
    dev = X.tau_of(y, r.exact, r.A)
    inst = ("complex" if c.cplx else "real") + "-" + c.fmt
    WORST[inst] = max(WORST.get(inst, 0.0), dev / r.tau)
    print("ddc-rows %-52s device tau %.3e bound %.3e fraction %.3f tau_f32 %.3e | largest so far %s %.3f" % (
        Q.case_id(c), dev, r.tau, dev / r.tau, r.tau_f32, inst, WORST[inst]))
    X.check(y, r.exact, r.A, r.tau, Q.case_id(c))


def test_streams_shorter_than_the_filter_and_the_step(lib, torch_cuda):
    torch = torch_cuda
    c = Q.Case(4, 33, 0.1234567, 0, "f32", "noise", 5, 0)        # 23 samples under 33 taps: every output sees the zero history
    r = Q.reference(c)
    assert len(r.raw) < c.T
    ddc = _ddc(lib, c, r.taps)
    got = ddc.run(torch.from_numpy(np.array(r.raw)).cuda())
    assert got.shape == (5,)
    X.check(got.cpu().numpy(), r.exact, r.A, r.tau, "shorter than the filter")
    short = torch.from_numpy(r.raw[:3].copy()).cuda()            # shorter than the step: no output, nothing launched
    assert ddc.num_out(3) == 0 and ddc.run(short).shape == (0,)
    assert ddc.run_batch(torch.stack([short, short])).shape == (2, 0)
    silent = ddc.run(torch.zeros(64, dtype=torch.float32, device="cuda"))
    assert not torch.view_as_real(silent).any()                  # A = 0: exactly zero
    ddc.close()


@pytest.mark.parametrize("fmt", ["s16", "u8"])
def test_real_integer_streams_at_odd_element_offsets(lib, torch_cuda, fmt):
    torch = torch_cuda
    c = Q.Case(8, 65, -0.49, 0, fmt, "noise", 300, 0)
    r = Q.reference(c)
    ddc = _ddc(lib, c, r.taps)
    d = torch.from_numpy(np.array(r.raw)).cuda()
    whole = ddc.run(d)
    X.check(whole.cpu().numpy(), r.exact, r.A, r.tau, Q.case_id(c))
    for off in (1, 3, 5):
        buf = torch.zeros(len(r.raw) + 8, dtype=d.dtype, device="cuda")
        buf[off:off + len(r.raw)] = d
        view = buf[off:off + len(r.raw)]
        assert (view.data_ptr() - buf.data_ptr()) == off * ESZ[fmt]
        assert _same(ddc.run(view), whole), off
    ddc.close()


# ---- bit for bit -------------------------------------------------------------------------------------------------------------
BIT_CASES = [Q.Case(16, 129, 0.1234567, 0, "f32", "noise", 2300, 0), Q.Case(3, 17, 0.25 + 2.0 ** -40, 1, "s16", "noise", 2300, 0),
             Q.Case(64, 513, -0.49, 0, "u8", "noise", 1100, 0), Q.Case(1, 33, 0.1234567, 1, "f32", "noise", 2300, 0)]
bit_cases = pytest.mark.parametrize("c", BIT_CASES, ids=Q.case_id)


def _device_input(torch, c):
    raw, _ = Q.make_input(c)
    return torch.from_numpy(raw).cuda()


@bit_cases
def test_output_ranges_equal_the_whole_run(lib, torch_cuda, c):
    """Cuts inside tiles and on their boundaries (a tile is 1024 outputs from the call's first)."""
    torch = torch_cuda
    ddc = _ddc(lib, c)
    d = _device_input(torch, c)
    whole = ddc.run(d)
    cuts = sorted({0, 1, 7, 1000, 1024, 1025, 2048, 2049, c.nout - 1, c.nout} & set(range(c.nout + 1)))
    guard = 64
    for a, b in zip(cuts, cuts[1:]):
        buf = torch.full((guard + (b - a) + guard,), SENTINEL, dtype=torch.complex64, device="cuda")
        out = ddc.run(d, first_out=a, nout=b - a, out=buf[guard:guard + b - a])
        assert out.data_ptr() == buf[guard:].data_ptr()
        assert _same(out, whole[a:b]), (a, b)
        assert _kept(buf[:guard]) and _kept(buf[guard + b - a:])
    assert ddc.run(d, first_out=c.nout, nout=0).shape == (0,)
    ddc.close()


@bit_cases
def test_batch_equals_loop_of_single_calls(lib, torch_cuda, c):
    """B = 1, 2 and 5; streams a pitch larger than S apart; overlapping streams cut from one buffer; a pitched `out`."""
    torch = torch_cuda
    ddc = _ddc(lib, c)
    S = c.nout * c.D + c.D // 2 + 1
    step = 3 * c.D + 1
    big = _device_input(torch, c._replace(nout=c.nout + 16))
    assert big.shape[0] >= S + 4 * step
    tail = (2,) if c.cplx else ()
    for B in (1, 2, 5):
        pitched = torch.zeros((B, S + 37) + tail, dtype=big.dtype, device="cuda")
        for b in range(B):
            pitched[b, :S] = big[b * step:b * step + S]
        es = 2 if c.cplx else 1
        overl = big.as_strided((B, S) + tail, (step * es, es) + ((1,) if c.cplx else ()))
        for v in (pitched[:, :S], overl):
            got = ddc.run_batch(v)
            assert got.shape == (B, S // c.D)
            for b in range(B):
                assert _same(got[b], ddc.run(v[b])), (B, b)
            a, n = 5, c.nout - 9
            guard, pitch = 32, n + 11
            buf = torch.full((guard + B * pitch + guard,), SENTINEL, dtype=torch.complex64, device="cuda")
            rows = buf[guard:guard + B * pitch].view(B, pitch)
            ddc.run_batch(v, first_out=a, nout=n, out=rows[:, :n])
            for b in range(B):
                assert _same(rows[b, :n], ddc.run(v[b], first_out=a, nout=n)), (B, b)
            assert _kept(rows[:, n:])
            assert _kept(buf[:guard]) and _kept(buf[guard + B * pitch:])
    ddc.close()


# ---- refusals, graph capture ----------------------------------------------------------------------------------------------------
def test_device_entry_refusals_with_real_handles(lib, torch_cuda):
    assert device_entry_refusals(lib) == 6


def test_wrapper_refuses_wrong_inputs(lib, torch_cuda):
    torch = torch_cuda
    ddc = lib.Ddc(8, 0.1, sample_format=lib.SAMPLES_S16)
    assert len(ddc.taps) == 65
    good = torch.zeros(4096, dtype=torch.int16, device="cuda")
    assert ddc.run(good).shape == (512,)
    for bad in (torch.zeros(4096, dtype=torch.float32, device="cuda"), torch.zeros((4096, 2), dtype=torch.int16, device="cuda"),
                torch.zeros(8192, dtype=torch.int16, device="cuda")[::2]):
        with pytest.raises(AssertionError):
            ddc.run(bad)
    with pytest.raises(lib.GlferHipError):
        ddc.run(good, first_out=500, nout=13)                     # an output past the stream
    ddc.close()
    with pytest.raises(lib.GlferHipError):
        lib.Ddc(2048, 0.1)
    with pytest.raises(lib.GlferHipError):
        lib.Ddc(8, 0.5)
    cz = lib.Ddc(8, 0.1, complex_in=True)
    with pytest.raises(AssertionError):
        cz.run(torch.zeros(4096, dtype=torch.float32, device="cuda"))
    assert cz.run(torch.zeros(4096, dtype=torch.complex64, device="cuda")).shape == (512,)
    cz.close()


def test_graph_capture_and_replay(lib, torch_cuda):
    """One capture of Ddc.run on a non-default stream, replayed: the eager outputs."""
    torch = torch_cuda
    c = Q.Case(16, 129, 0.1234567, 0, "f32", "tone", 1500, 0)
    r = Q.reference(c)
    ddc = _ddc(lib, c, r.taps)
    d = torch.from_numpy(np.array(r.raw)).cuda()
    eager = ddc.run(d)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    out = torch.full((c.nout,), SENTINEL, dtype=torch.complex64, device="cuda")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        ddc.run(d, out=out)
    torch.cuda.synchronize()
    out.fill_(SENTINEL)
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    assert _same(out, eager)
    X.check(out.cpu().numpy(), r.exact, r.A, r.tau, "graph replay")
    ddc.close()
