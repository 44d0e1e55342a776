"""GPU tests (-m gpu): HP-ARMA rows bin by bin in amplitude against float64, on every input kind, option and route of hparma.hip.

The older HP-ARMA tests (test_hparma_parity, test_hparma_error_within_the_references_own_spread, test_hparma_over_many_streams,
test_hparma_schedule_over_matrix_shapes, test_hparma_block_sizes_outside_256_to_16384) hold |A(f)|^2 / N to max(1e-5, 3 s) of the
row's LARGEST bin on one kind of input (two tones over noise, f32); the row is the reciprocal of that quantity, and a spectral
line is a bin 1e4 ... 1e7 times below the largest.  Here every bin of every frame is held to tests/_hparma_check.py's rule

    | sqrt(q_got[k]) - sqrt(q64[k]) |  <=  (tau_eval + tau_cond) * sqrt( sum_k q64[k] )

q64 the float64 spectrum of the ORACLE's AR vector, tau_eval = 4 max(tau_f32, 2^-24), tau_cond = 3 s_amp -- all computed on the
CPU per case, never from device output -- together with the oracle's finiteness pattern (NaN rows of silence, inf at a zero of
A) and, where the oracle's rank is p_e or more, the bits of N and 1 / N.  tests/test_hparma_criterion.py judges the rule and
the matrix (tests/_hparma_cases.py) without a device.

Routes (tests/_hparma_cases.py kernel_route restates the launcher's choice; the record names the one a case runs):
  fixed<128,33>, fixed<96,17>    by default at those shapes            scheduled   the same under GLFER_HPARMA_GENERIC=1, and every
  scheduled-4lane                a plan made under GLFER_HPARMA_WIDTH=16             other t <= 128 (a multiple of 4), <= 64 columns
  fast-walk                      t = 66                                general-walk   t = 160 (looped autocorrelation), 65 columns

Lines starting with 'hparma-bin-by-bin' (run with -s) are the record kept in profiles/hparma_rows.txt: the device's fraction of
the bound, the oracle's own, and the older tests' peak-normalised figure beside their bound.
"""
import numpy as np
import pytest

import _hparma_cases as M
import _hparma_check as H
import _rows_cases as K

pytestmark = pytest.mark.gpu
ENV = ("GLFER_HPARMA_WIDTH", "GLFER_HPARMA_GENERIC", "GLFER_HPARMA_LDS_KB")
RECORD = ("hparma-bin-by-bin %-2s %-50s %-12s %-36s fraction %.3f bound %.3e tau_f32 %.3e s_amp %.3e oracle %.3f "
          "peak-normalised %.2e of %.2e")


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


@pytest.fixture(autouse=True)
def _product_kernels(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)


def _plan(lib, monkeypatch, c, sub_mean=None, **kw):
    """The case's plan on its route.  GLFER_HPARMA_WIDTH is read when the plan is made, GLFER_HPARMA_GENERIC at every launch."""
    if c.route == "w16":
        monkeypatch.setenv("GLFER_HPARMA_WIDTH", "16")
    if c.route == "generic":
        monkeypatch.setenv("GLFER_HPARMA_GENERIC", "1")
    fmt = {"f32": lib.SAMPLES_F32, "s16": lib.SAMPLES_S16, "u8": lib.SAMPLES_U8}[c.fmt]
    return lib.Spectrogram(lib.HparmaParams(n=c.n, overlap=c.ovl, t=c.t, p_e=c.p_e, sub_mean=c.sub_mean if sub_mean is None else sub_mean,
                                            history_mode=c.history_mode, sample_format=fmt, **kw))


def _upload(torch, raw, offset=0):
    """The stream on the device; offset > 0: that many samples into its allocation."""
    if not offset:
        return torch.from_numpy(raw).cuda()
    host = np.concatenate([np.full(offset, 77, raw.dtype), raw])
    return torch.from_numpy(host).cuda()[offset:]


def _judge(group, c, form, got, r, rows=slice(None)):
    """Device rows under the rule; prints the record line first, so that a failing case leaves its figures."""
    got = np.asarray(got)
    want, a, rank = r.want[rows], r.a[rows], r.rank[rows]
    assert got.shape == want.shape, (got.shape, want.shape)
    what = "%s %s %s" % (group, M.case_id(c), form)
    print(RECORD % (group, M.case_id(c), form, M.kernel_route(c), H.fraction(got, a, c.n, r.tau), r.tau, r.tau_f32, r.s_amp, r.oracle_frac,
                    H.peak_figure(got, want, c.n), r.old_bound))
    return H.check(got, want, a, rank, c.n, c.p_e, r.tau, what)


def _run(lib, oracle, torch, monkeypatch, c, sub_mean=None, offset=0, **kw):
    r = M.reference(oracle, c)
    sp = _plan(lib, monkeypatch, c, sub_mean)
    got = sp.run(_upload(torch, r.raw, offset), **kw).cpu().numpy()
    sp.close()
    return got, r


# ---- (a) every signal at the two fixed shapes; (b) every route; (c) silence around prank < p_e; (d) the block sizes -----------
@pytest.mark.parametrize("c", M.SIGNAL_CASES, ids=M.case_id)
def test_every_signal_at_the_fixed_shapes(lib, oracle, torch_cuda, monkeypatch, c):
    got, r = _run(lib, oracle, torch_cuda, monkeypatch, c)
    _judge("a", c, "default", got, r)


@pytest.mark.parametrize("c", M.ROUTE_CASES, ids=M.case_id)
def test_every_route(lib, oracle, torch_cuda, monkeypatch, c):
    got, r = _run(lib, oracle, torch_cuda, monkeypatch, c)
    _judge("b", c, c.route, got, r)


@pytest.mark.parametrize("c", M.SILENCE_CASES, ids=M.case_id)
def test_silence_on_both_sides_of_the_initial_rank(lib, oracle, torch_cuda, monkeypatch, c):
    """Digital silence leaves the rank at its initial 4: p_e <= 4 gives a = e_0 (rows of N and 1 / N), p_e >= 5 a NaN row."""
    got, r = _run(lib, oracle, torch_cuda, monkeypatch, c)
    _judge("c", c, "default", got, r)
    assert np.isnan(got).all() if c.p_e >= 5 else (got[:, :-1] == c.n).all()


@pytest.mark.parametrize("c", M.SIZE_CASES, ids=M.case_id)
def test_block_sizes(lib, oracle, torch_cuda, monkeypatch, c):
    got, r = _run(lib, oracle, torch_cuda, monkeypatch, c)
    _judge("d", c, "default", got, r)


# ---- (e) options, each against the oracle ---------------------------------------------------------------------------------
@pytest.mark.parametrize("c", M.FORMAT_CASES, ids=M.case_id)
def test_integer_sample_formats(lib, oracle, torch_cuda, monkeypatch, c):
    off = M.FORMAT_OFFSETS.get(M.case_id(c), 0)
    got, r = _run(lib, oracle, torch_cuda, monkeypatch, c, offset=off)
    assert r.raw.dtype == (np.int16 if c.fmt == "s16" else np.uint8)
    _judge("e", c, "offset%d" % off, got, r)


@pytest.mark.parametrize("c", M.OVERLAP_CASES + M.HISTORY_CASES, ids=M.case_id)
def test_overlaps_and_zeroed_history(lib, oracle, torch_cuda, monkeypatch, c):
    got, r = _run(lib, oracle, torch_cuda, monkeypatch, c)
    _judge("e", c, "default", got, r)


@pytest.mark.parametrize("c", M.MEAN_CASES, ids=M.case_id)
def test_mean_removal_in_the_references_order(lib, oracle, torch_cuda, monkeypatch, c):
    got, r = _run(lib, oracle, torch_cuda, monkeypatch, c, sub_mean=lib.SUBMEAN_EXACT)
    _judge("e", c, "m1", got, r)


@pytest.mark.parametrize("c", M.MEAN2_CASES, ids=M.case_id)
def test_mean_removal_with_the_in_kernel_sums(lib, oracle, torch_cuda, monkeypatch, c):
    """sub_mean = 2 gives the reference's rows where every hop's mean is small against its rms (include/glfer_hip.h)."""
    assert K.mean2_condition(c, M.reference(oracle, c).xf)
    got, r = _run(lib, oracle, torch_cuda, monkeypatch, c, sub_mean=lib.SUBMEAN_FAST)
    _judge("e", c, "m2", got, r)


# ---- (f) a launch inside the stream; rows on a pitch ----------------------------------------------------------------------
@pytest.mark.parametrize("cf", M.RANGE_CASES, ids=lambda cf: "%s-first%d" % (M.case_id(cf[0]), cf[1]))
def test_frame_range_inside_the_stream(lib, oracle, torch_cuda, monkeypatch, cf):
    c, first = cf
    nframes = c.frames - first - 2
    got, r = _run(lib, oracle, torch_cuda, monkeypatch, c, first_frame=first, nframes=nframes)
    _judge("f", c, "first%d" % first, got, r, rows=slice(first, first + nframes))


@pytest.mark.parametrize("cp", M.PITCH_CASES, ids=lambda cp: "%s-pitch%d" % (M.case_id(cp[0]), cp[1]))
def test_rows_on_a_pitch_between_sentinels(lib, oracle, torch_cuda, monkeypatch, cp):
    c, pitch = cp
    r = M.reference(oracle, c)
    sp = _plan(lib, monkeypatch, c, psd_pitch=pitch)
    bins = c.n // 2 + 1
    assert sp.pitch == pitch and sp.bins == bins
    out = torch_cuda.full((c.frames, pitch), -77.0, device="cuda")
    got = sp.run(_upload(torch_cuda, r.raw), out=out).cpu().numpy()
    sp.close()
    assert (got[:, bins:] == -77.0).all()                                # nothing between the rows
    _judge("f", c, "pitch%d" % pitch, got[:, :bins], r)


# ---- (g) placement ---------------------------------------------------------------------------------------------------------
def test_a_batch_of_unlike_streams(lib, oracle, torch_cuda, monkeypatch):
    """run_batch over tones, silence, noise and a constant side by side: every stream under the rule (a NaN row beside finite ones)."""
    c = M.BATCH_CASE
    members = [c._replace(signal=s) for s in M.BATCH_SIGNALS]
    whole = c.frames * K.X.hop_len(c.n, c.ovl)
    refs = [M.reference(oracle, m) for m in members]
    sp = _plan(lib, monkeypatch, c)
    got = sp.run_batch(torch_cuda.from_numpy(np.stack([r.raw[:whole] for r in refs])).cuda()).cpu().numpy()
    sp.close()
    assert got.shape == (len(members), c.frames, c.n // 2 + 1)
    for b, (m, r) in enumerate(zip(members, refs)):
        _judge("g", m, "batch[%d]" % b, got[b], r)


def test_ragged_streams_of_unlike_kinds(lib, oracle, torch_cuda, monkeypatch):
    """run_ragged over streams of 7, 1, 4, 0 and 6 hops at even offsets of one buffer with gaps between them."""
    c = M.RAGGED_CASE
    h = K.X.hop_len(c.n, c.ovl)
    members = [c._replace(signal=s, frames=k) for s, k in zip(M.RAGGED_SIGNALS, M.RAGGED_HOPS)]
    refs = [M.reference(oracle, m) if m.frames else None for m in members]
    buf = np.full(sum(M.RAGGED_HOPS) * h + 64, np.nan, np.float32)
    offs, lens, at = [], [], 6
    for m, r in zip(members, refs):
        k = m.frames * h
        if k:
            buf[at:at + k] = r.raw[:k]
        offs.append(at)
        lens.append(k)
        at += k + 10
    sp = _plan(lib, monkeypatch, c)
    rows, starts = sp.run_ragged(torch_cuda.from_numpy(buf).cuda(), offs, lens)
    rows = rows.cpu().numpy()
    sp.close()
    assert list(np.diff(starts)) == M.RAGGED_HOPS
    for b, (m, r) in enumerate(zip(members, refs)):
        if m.frames:
            _judge("g", m, "ragged[%d]" % b, rows[starts[b]:starts[b + 1]], r)
