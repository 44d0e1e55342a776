"""GPU tests (-m gpu): the periodogram's register-walk forms, second units of work of the persistent kernels, and spectro_big.hip
past its grid cap and its first scratch group -- every judged row bin by bin in amplitude against float64 under the unchanged rule
of tests/_rows_check.py,

    | sqrt(got[k]) - sqrt(exact[k]) |  <=  tau * sqrt( sum_k exact[k] ),    tau = 4 * max(tau_f32, 2**-24),

tau_f32 per case from the CPU stand-ins of tests/_exact.py, and per frame under K.oracle_bound against the oracle; silent frames
must come out as exact zeros.  The cases and the schedule they are built on: tests/_walk_cases.py, tests/_grid_passes.py;
tests/test_walk_criterion.py shows on the CPU that the references pass, that the inputs are adversarial at every place of a
slot's walk, and that the rule rejects rows made with a wrong walk.

B  spectro16h.hip's SHIFT = 2 / 4 / 8 instantiations (launch16h_fmt: the periodogram at overlap 87.5 / 75 / 50 %, no mean removal,
   history from the stream, work >= 4 x resident): whole streams of 8 ... 13 M bins, all frames judged; three of the plans one work
   unit below the threshold (the plain form); range calls between sentinel rows; a two-stream batch and a ragged call, bit for
   bit the single-stream calls.
C  65 ... 71 units of work on 64 workgroups: spectro16xl, spectro16x, spectro16 (GLFER_FORM=x), spectro16h's multitaper form,
   spectro16w (default, GLFER_FORM=w, spectrum=True at N = 32768); all frames judged.
D  spectro_big.hip: N = 32768 past subfft_kernel's 4096-workgroup cap, N = 2^20 past the launcher's first scratch group; cuts.

Which instantiation a test really ran is not asked of the library: profiles/rows_walk_kernels_run.txt is the kernel trace of one
run of this module.  Lines starting with 'rows-walk' (run with -s) are the record kept in profiles/rows_walk.txt.
"""
import numpy as np
import pytest

import _pairs_cases as P
import _rows_cases as K
import _walk_cases as W
from _rows_check import check_rows, check_spectrum, from_halfcomplex, tau_of, tau_of_spectrum
from _rows_device import _plan, _select, _upload
from _signals import rel_err

pytestmark = pytest.mark.gpu
SENTINEL = -7.0


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _judge(group, name, form, c, got, r, rows=slice(None)):
    """Device rows against the float64 rows under (1) and against the oracle under the suite's rule; prints the record line."""
    exact, want = r.exact[rows], r.want[rows]
    got = np.asarray(got)
    assert got.shape == exact.shape, (got.shape, exact.shape)
    what = "%s %s %s" % (group, name, form)
    dev_tau = tau_of(got, exact)
    print("rows-walk %-2s %-86s %-16s device tau %.3e bound %.3e fraction %.3f tau_f32 %.3e oracle tau %.3e" % (
        group, name, form, dev_tau, r.tau, dev_tau / r.tau, r.tau_f32, r.tau_oracle))
    frac = check_rows(got, exact, r.tau, what)
    for f in range(len(want)):
        if want[f].any():
            e_dev, e_ref = max(rel_err(got[f], want[f])), max(rel_err(want[f], exact[f]))
            assert e_dev <= K.oracle_bound(c, e_ref), (what, f, e_dev, e_ref)
        else:
            assert not got[f].any(), (what, f)                  # silence stays silence
    return frac


def _form(w):
    return "shift%d-per%d" % (w.shift, w.per)


# ---- B: the walk forms ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", W.WALK_CASES, ids=K.case_id)
def test_walk_forms_every_frame(lib, oracle, torch_cuda, monkeypatch, c):
    """The whole stream: ceil(R / H) head frames through the packed kernel, the body through the SHIFT form with a partly filled
    last slot (and, with per = 5, slots and workgroups past the end that must store nothing)."""
    _select(monkeypatch, "default")
    r = K.reference(oracle, c, W.seed_of(c))
    off = W.WALK_OFFSETS.get(K.case_id(c), 0)
    sp = _plan(lib, oracle, c)
    got = sp.run(_upload(torch_cuda, r.raw, off)).cpu().numpy()
    sp.close()
    _judge("B", K.case_id(c), _form(W.walk_of(c)[1]) + ("-off%d" % off if off else ""), c, got, r)


@pytest.mark.parametrize("c", W.BELOW_CASES, ids=K.case_id)
def test_one_work_unit_below_the_threshold(lib, oracle, torch_cuda, monkeypatch, c):
    """work = 4 x resident - 1: the same plans in the plain form (SHIFT = 0 in the kernel trace), the longest launches it takes."""
    _select(monkeypatch, "default")
    r = K.reference(oracle, c, W.seed_of(c))
    sp = _plan(lib, oracle, c)
    got = sp.run(_upload(torch_cuda, r.raw)).cpu().numpy()
    sp.close()
    _judge("B", K.case_id(c), _form(W.walk_of(c)[1]), c, got, r)


@pytest.mark.parametrize("c", W.RANGE_CASES, ids=K.case_id)
def test_walk_forms_range_between_sentinel_rows(lib, oracle, torch_cuda, monkeypatch, c):
    """first_frame off the whole-stream call's slot grid, the end inside a slot: the rows are written between two sentinel rows,
    so a frame stored in front of the range or past its end is seen."""
    _select(monkeypatch, "default")
    r = K.reference(oracle, c, W.seed_of(c))
    lo, hi = W.range_of(c)
    sp = _plan(lib, oracle, c)
    buf = torch_cuda.full((hi - lo + 2, sp.pitch), SENTINEL, dtype=torch_cuda.float32, device="cuda")
    sp.run(_upload(torch_cuda, r.raw), first_frame=lo, nframes=hi - lo, out=buf[1:-1])
    sp.close()
    buf = buf.cpu().numpy()
    assert (buf[0] == SENTINEL).all() and (buf[-1] == SENTINEL).all()
    _judge("B", K.case_id(c), "%s-first%d-n%d" % (_form(W.walk_of(c, lo, hi)[1]), lo, hi - lo), c, buf[1:-1], r, rows=slice(lo, hi))


def test_walk_forms_batch_of_two_streams(lib, oracle, torch_cuda, monkeypatch):
    """run_batch: both streams per stream against float64, and bit for bit the single-stream calls."""
    _select(monkeypatch, "default")
    c = W.BATCH_CASE
    refs = [K.reference(oracle, c, W.seed_of(c, slot)) for slot in (0, 1)]
    sp = _plan(lib, oracle, c)
    d = torch_cuda.from_numpy(np.stack([r.raw for r in refs])).cuda()
    got = sp.run_batch(d).cpu().numpy()
    assert got.shape == (2, c.frames, c.n // 2 + 1)
    for b, r in enumerate(refs):
        _judge("B", K.case_id(c), "%s-batch%d" % (_form(W.walk_of(c, nbatch=2)[1]), b), c, got[b], r)
        single = sp.run(d[b].contiguous()).cpu().numpy()
        assert np.array_equal(single.view(np.uint32), got[b].view(np.uint32)), b
    sp.close()


def test_walk_forms_ragged_streams(lib, oracle, torch_cuda, monkeypatch):
    """run_ragged over two streams of unequal length, both bodies above the threshold (the launcher sizes the grid by the longer
    one; each stream walks it with its own `per`)."""
    _select(monkeypatch, "default")
    c0 = W.RAGGED_CASE
    cases = [c0, c0._replace(frames=c0.frames + W.RAGGED_MORE)]
    refs = [K.reference(oracle, c, W.seed_of(c0, slot)) for slot, c in enumerate(cases)]
    lengths = [len(r.raw) for r in refs]
    offsets = [0, lengths[0] + 6]                               # (a gap between the streams)
    host = np.zeros(offsets[1] + lengths[1], refs[0].raw.dtype)
    for o, r in zip(offsets, refs):
        host[o:o + len(r.raw)] = r.raw
    d = torch_cuda.from_numpy(host).cuda()
    sp = _plan(lib, oracle, c0)
    got, starts = sp.run_ragged(d, offsets, lengths)
    got = got.cpu().numpy()
    assert list(starts) == [0, cases[0].frames, cases[0].frames + cases[1].frames]
    for b, (c, r) in enumerate(zip(cases, refs)):
        mine = got[starts[b]:starts[b + 1]]
        _judge("B", K.case_id(c), "%s-ragged%d" % (_form(W.walk_of(c, nbatch=2)[1]), b), c, mine, r)
        single = sp.run(d[offsets[b]:offsets[b] + lengths[b]]).cpu().numpy()
        assert np.array_equal(single.view(np.uint32), mine.view(np.uint32)), b
    sp.close()


# ---- C: second units of work -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", W.SECOND_CASES, ids=W.second_id)
def test_second_units_of_work(lib, oracle, torch_cuda, monkeypatch, s):
    """65 ... 71 units of body work on a grid of 64: some workgroups take a second unit, whose frames differ in level from their
    first unit's (odd taper counts: whose partners differ in level)."""
    _select(monkeypatch, s.form)
    c = s.c
    r = W.second_reference(oracle, s)
    if s.dev_mean == 2:
        assert s.dev_mean == lib.SUBMEAN_FAST and K.mean2_condition(c, r.xf)
    sp = _plan(lib, oracle, c, s.dev_mean)
    dx = _upload(torch_cuda, r.raw, s.offset)
    b0, b1, p = W.second_passes(s)
    form = "%s-%s-u%d" % (s.kernel, s.form, p.work) + ("-m%d" % s.dev_mean if s.dev_mean else "") + ("-off%d" % s.offset if s.offset else "")
    if s.spectrum:
        psd, spec = sp.run(dx, spectrum=True)
        got_X = from_halfcomplex(spec.cpu().numpy())
        exact_X, t32, tau = W.second_spectrum_reference(oracle, s)
        dev = tau_of_spectrum(got_X, exact_X, c.n)
        print("rows-walk %-2s %-86s %-16s device tau %.3e bound %.3e fraction %.3f tau_f32 %.3e oracle tau %s" % (
            "C", K.case_id(c), form + "-X", dev, tau, dev / tau, t32, "-"))
        check_spectrum(got_X, exact_X, c.n, tau, W.second_id(s))
        got = psd.cpu().numpy()
    else:
        got = sp.run(dx).cpu().numpy()
    sp.close()
    _judge("C", K.case_id(c), form, c, got, r)


# ---- D: spectro_big.hip ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cc", W.BIG_CASES, ids=lambda cc: K.case_id(cc[0]))
def test_big_blocks_past_the_grid_cap_and_the_scratch_group(lib, oracle, torch_cuda, monkeypatch, cc):
    """Cuts only (as test_gpu_rows.py's long launch of the interleaved form): the float64, float32 and oracle rows of the cut
    frames from a sub-stream that carries their history; the whole launch must be finite, of the right shape, and without a
    silent row (the input has none)."""
    _select(monkeypatch, "default")
    c, cuts = cc
    raw, xf = K.make_input(oracle, c)
    sp = _plan(lib, oracle, c)
    got = sp.run(_upload(torch_cuda, raw))
    assert tuple(got.shape) == (c.frames, c.n // 2 + 1) and bool(torch_cuda.isfinite(got).all())
    assert bool((got.sum(dim=1) > 0).all())
    for a, b in cuts:
        r, _ = P.cut_reference(oracle, c, xf, a, b)
        _judge("D", K.case_id(c), "cut%d-%d" % (a, b), c._replace(frames=b - a), got[a:b].cpu().numpy(), r)
    sp.close()
