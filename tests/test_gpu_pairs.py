"""GPU tests (-m gpu): multitaper rows of odd taper counts, bin by bin, when the two frames that share a transform differ in
level -- keyed input (tests/_pairs_cases.py) through spectro16xl.hip (N = 256 ... 2048), spectro16x.hip (23 tapers at
N = 1024) and spectro16y.hip (N = 4096: five tapers NW 2.5 the half-table form with its frame-pair queue, GLFER_Y_TAPERS=full
and 3 / 9 tapers the full-table form; mean removal inside the kernel takes it off the queue).

Every bin of every frame is held to tests/_rows_check.py's rule at tau = 4 max(tau_f32, 2^-24) with tau_f32 from the UNPAIRED
float32 stand-in: odd_taper.hpp promises each frame the rounding of a transform of its own, so sharing one gets no allowance.
A row whose exact sum is 0 must be 0 in every bin.  Beside it the per-frame peak rule against the oracle (1e-5) stays
asserted.  tests/test_pairs_criterion.py shows on the CPU that every case has partners 10^6 apart in both orders, silent
frames beside loud ones, and that a stand-in without the scales, or with the partners' scales exchanged, fails this rule.

A frame range is checked against the float64 rows of the same frames only: rows are promised bit for bit across cuts on
multiples of GLFER_FRAME_ALIGN, which first_frame = 1, FPB - 1, FPB, FPB + 1 are not -- the frames of a
group cut in two go to the packed kernel.  Batch and ragged rows are the single-stream entry's bit for bit, as everywhere.

Lines starting with 'rows-keyed-pairs' (run with -s) are the record kept in profiles/rows_keyed_pairs.txt.
"""
import numpy as np
import pytest

import _pairs_cases as P
import _rows_cases as K
from _rows_check import bound, check_rows, tau_of
from _rows_device import _plan, _select, _upload
from _signals import rel_err

pytestmark = pytest.mark.gpu
SENTINEL = -7.25


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _judge(c, route, got, r, rows=slice(None), paired=None):
    """Device rows under the rule and under the oracle's; prints the record line.  paired: the paired stand-in's tau / bound."""
    exact, want = r.exact[rows], r.want[rows]
    got = np.asarray(got)
    assert got.shape == exact.shape, (got.shape, exact.shape)
    what = "%s %s" % (K.case_id(c), route)
    dev_tau = tau_of(got, exact)
    print("rows-keyed-pairs %-66s %-16s device tau %.3e bound %.3e fraction %.3f tau_f32 %.3e paired stand-in tau %s" % (
        K.case_id(c), route, dev_tau, r.tau, dev_tau / r.tau, r.tau_f32, "-" if paired is None else "%.3e" % (paired * r.tau)))
    frac = check_rows(got, exact, r.tau, what)
    for f in range(len(want)):
        if want[f].any():
            assert max(rel_err(got[f], want[f])) <= K.TOL, (what, f)
        else:
            assert not got[f].any(), (what, f)                  # silence stays silence
    return frac


def _case(oracle, c, slot=0):
    fg = P.figures(oracle, c, P.seed_of(c, slot))
    return fg.ref, (fg.scaled if P.shares_transforms(c) else None)


def _forms_of(c):
    return ("default",) + (("full",) if (c.n, c.kmax, c.nw) == (4096, 4, 2.5) else ()) + (("w",) if c.n >= 2048 else ())


# ---- the whole stream, every form of the size --------------------------------------------------------------------------
@pytest.mark.parametrize("c,form", [pytest.param(c, f, id="%s-%s" % (K.case_id(c), f)) for c in P.SIZE_CASES + P.CONTROL_CASES for f in _forms_of(c)])
def test_keyed_stream(lib, oracle, torch_cuda, monkeypatch, c, form):
    _select(monkeypatch, form)
    r, paired = _case(oracle, c)
    sp = _plan(lib, oracle, c)
    got = sp.run(_upload(torch_cuda, r.raw)).cpu().numpy()
    sp.close()
    _judge(c, form, got, r, paired=paired if form != "w" else None)


# ---- frame ranges: the head and the tail move, the groups stay on the stream's frame indices ----------------------------------
@pytest.mark.parametrize("c", P.RANGE_CASES, ids=K.case_id)
def test_frame_ranges_against_the_keying(lib, oracle, torch_cuda, monkeypatch, c):
    _select(monkeypatch, "default")
    r, paired = _case(oracle, c)
    sp = _plan(lib, oracle, c)
    dx = _upload(torch_cuda, r.raw)
    _judge(c, "whole", sp.run(dx).cpu().numpy(), r, paired=paired)
    for a in P.range_firsts(c):
        lo, hi = P.range_of(c, a)
        _judge(c, "first%d" % a, sp.run(dx, first_frame=lo, nframes=hi - lo).cpu().numpy(), r, rows=slice(lo, hi))
    sp.close()


# ---- batches: a frame never takes a partner from another stream -------------------------------------------------------
@pytest.mark.parametrize("c", P.BATCH_CASES, ids=K.case_id)
def test_batch_of_keyed_streams_and_silence(lib, oracle, torch_cuda, monkeypatch, c):
    _select(monkeypatch, "default")
    refs = [_case(oracle, c, s) for s in range(P.BATCH_SLOTS)]
    raws = [r.raw for r, _ in refs]
    raws.insert(2, np.zeros_like(raws[0]))                      # (silence between two keyed streams)
    d = torch_cuda.from_numpy(np.stack(raws)).cuda()
    sp = _plan(lib, oracle, c)
    got = sp.run_batch(d)
    assert tuple(got.shape) == (4, c.frames, c.n // 2 + 1)
    assert not bool(got[2].any())
    for b, s in ((0, 0), (1, 1), (3, 2)):
        _judge(c, "batch%d" % b, got[b].cpu().numpy(), refs[s][0], paired=refs[s][1])
    for b in range(4):
        assert torch_cuda.equal(got[b], sp.run(d[b])), b
    sp.close()


# ---- ragged: loud and quiet streams side by side ------------------------------------------------------------------------------
@pytest.mark.parametrize("c", P.RAGGED_CASES, ids=K.case_id)
def test_ragged_loud_and_quiet_streams(lib, oracle, torch_cuda, monkeypatch, c):
    _select(monkeypatch, "default")
    streams = P.ragged_streams(oracle, c)
    gap, offs, at = 5, [], 0
    for x, _ in streams:
        at += gap
        offs.append(at)
        at += len(x)
    buf = np.full(at + gap, np.nan, np.float32)
    for (x, _), o in zip(streams, offs):
        buf[o:o + len(x)] = x
    lens = [len(x) for x, _ in streams]
    total = sum(fr for _, fr in streams)
    sp = _plan(lib, oracle, c)
    d = torch_cuda.from_numpy(buf).cuda()
    got = torch_cuda.full((total + 3, sp.pitch), SENTINEL, dtype=torch_cuda.float32, device="cuda")
    _, starts = sp.run_ragged(d, offs, lens, out=got)
    assert list(starts) == [0] + list(np.cumsum([fr for _, fr in streams]))
    assert bool((got[total:] == SENTINEL).all())
    for i, ((x, fr), o) in enumerate(zip(streams, offs)):
        if not fr:
            continue
        rows = got[int(starts[i]):int(starts[i + 1])]
        assert torch_cuda.equal(rows, sp.run(d[o:o + len(x)])), i
        m = c._replace(frames=fr)
        exact, f32, want = K.rows_of(oracle, m, x)
        t32 = tau_of(f32, exact)
        r = K.Ref(x, x, exact, f32, want, t32, bound(t32), tau_of(want, exact), K.peak_err(want, exact))
        _judge(m, "ragged%d" % i, rows.cpu().numpy(), r)
    sp.close()


# ---- mean removal, history, sample formats ------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["default", "prepass"])
@pytest.mark.parametrize("c", P.MEAN_CASES, ids=K.case_id)
def test_mean_removal_in_the_references_order(lib, oracle, torch_cuda, monkeypatch, c, form):
    _select(monkeypatch, form)
    r, paired = _case(oracle, c)
    sp = _plan(lib, oracle, c, lib.SUBMEAN_EXACT)
    got = sp.run(_upload(torch_cuda, r.raw)).cpu().numpy()
    sp.close()
    _judge(c, "m1-" + form, got, r, paired=paired)


@pytest.mark.parametrize("c", P.HISTORY_CASES + P.FORMAT_CASES + P.FORMAT_PLAIN_CASES, ids=K.case_id)
def test_history_zeroed_and_integer_formats(lib, oracle, torch_cuda, monkeypatch, c):
    _select(monkeypatch, "default")
    r, paired = _case(oracle, c)
    off = P.FORMAT_OFFSETS.get(K.case_id(c), 0)
    assert c.history_mode == lib.HISTORY_ZERO_ALWAYS or r.raw.dtype == (np.int16 if c.fmt == "s16" else np.uint8)
    sp = _plan(lib, oracle, c)
    got = sp.run(_upload(torch_cuda, r.raw, off)).cpu().numpy()
    sp.close()
    _judge(c, "offset%d" % off, got, r, paired=paired)


# ---- long launches, judged on cuts --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cs", P.LONG_CASES, ids=lambda cs: K.case_id(cs[0]))
def test_long_keyed_launches_on_cuts(lib, oracle, torch_cuda, monkeypatch, cs):
    """N = 4096: the queue's ticketed chunks (its static chunks end at frame 4 096).  N = 256: spectro16xl.hip's second iteration
    starts at P.xl_second_pass_from = frame 65 568; the middle cut straddles it.  Cuts are widened to whole pairs."""
    _select(monkeypatch, "default")
    c, seam = cs
    raw, xf = K.make_input(oracle, c, P.seed_of(c))
    sp = _plan(lib, oracle, c)
    got = sp.run(_upload(torch_cuda, raw))
    assert got.shape[0] == c.frames and bool(torch_cuda.isfinite(got).all())
    for a, b in P.long_cuts(c, seam):
        r, _ = P.cut_reference(oracle, c, xf, a, b)
        _judge(c._replace(frames=b - a), "cut%d" % a, got[a:b].cpu().numpy(), r)
    sp.close()
