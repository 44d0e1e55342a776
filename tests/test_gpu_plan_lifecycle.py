"""A plan's life on the device (-m gpu): made, used and destroyed in every mode; the F-test's tables made once, on the first F
call of any entry, and shared by the others; and made once when two threads, each on a stream of its own, make their first F
call at the same time (glfer_amd/csrc/plan.cpp: the plan's device tables are owned by glfer::DeviceTable, ftest_tables runs
under the plan's mutex and publishes its tables only when all of them are there).

Rows are compared bit for bit (int32 views) wherever two calls must agree; the multitaper rows of the rows-and-F entry are
judged as tests/test_gpu_rows_ftest.py judges them: bin by bin against float64 (rule 2) and per frame against the oracle
(rule 3), with that file's cases and reference (tests/_rows_ftest_cases.py)."""
import threading

import pytest

import _rows_ftest_cases as R
from _rows_check import check_rows
from _signals import rel_err, synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _bits(torch, t):
    return t.contiguous().view(torch.int32)


MODES = {
    "fft512": lambda lib: lib.FftParams(n=512, window_type=lib.WINDOWS["hanning"], overlap=0.5),
    "mtm4096_k4": lambda lib: lib.MtmParams(n=4096, overlap=0.0, w=2.5, kmax=4),
    "hparma32": lambda lib: lib.HparmaParams(n=32, overlap=0.0, t=8, p_e=3),
    "lmp512": lambda lib: lib.LmpParams(n=512, overlap=0.5, avg=4),
}


@pytest.mark.parametrize("mode", sorted(MODES))
def test_create_use_destroy(lib, oracle, torch_cuda, mode):
    """One plan of each mode: made, run once on a few frames, destroyed -- and once more, with the same rows bit for bit."""
    torch = torch_cuda
    params = MODES[mode](lib)
    xh = synth(9 * params.n, seed=5)
    x = torch.from_numpy(xh).cuda()
    rows = []
    for _ in range(2):
        sp = lib.Spectrogram(params)
        got = sp.run(x)
        torch.cuda.synchronize()
        assert got.shape == (sp.num_frames(x.numel()), params.n // 2 + 1)
        rows.append(got.cpu())
        sp.close()
    assert torch.equal(_bits(torch, rows[0]), _bits(torch, rows[1]))
    want = {"fft512": lambda: oracle.spectrogram_fft(xh, 512, 0.5, window_type=lib.WINDOWS["hanning"]),
            "mtm4096_k4": lambda: oracle.spectrogram_mtm(xh, 4096, 0.0, 2.5, 4)}.get(mode)
    if want is not None:                                     # the two modes whose rows are the oracle's to 1e-5 frame by frame
        want = want()
        assert max(max(rel_err(rows[0][f].numpy(), want[f])) for f in range(len(want))) < 1e-5


def test_f_tables_made_once_and_shared(lib, oracle, torch_cuda):
    """Five tapers at N = 4096: two F calls and one rows-and-F call on one plan.  The F rows of all three are the same bits (and
    those of a plan whose first F call is the rows-and-F entry); the multitaper rows of the rows-and-F call pass the rules of
    tests/test_gpu_rows_ftest.py, and so do run()'s."""
    torch = torch_cuda
    c = R.shape_case("n4096")
    assert (c.n, c.kmax) == (4096, 4)
    r = R.reference(oracle, c)
    x = torch.from_numpy(r.raw).cuda()
    sp = lib.Spectrogram(lib.MtmParams(n=c.n, overlap=c.ovl, w=c.nw, kmax=c.kmax))
    f1 = sp.ftest(x)
    f2 = sp.ftest(x)
    psd, f3 = sp.rows_ftest(x)
    plain = sp.run(x)
    other = lib.Spectrogram(lib.MtmParams(n=c.n, overlap=c.ovl, w=c.nw, kmax=c.kmax))
    _, f4 = other.rows_ftest(x)
    torch.cuda.synchronize()
    for f in (f2, f3, f4):
        assert torch.equal(_bits(torch, f), _bits(torch, f1))
    for name, rows in (("rows_ftest", psd), ("run", plain)):
        got = rows.cpu().numpy()
        check_rows(got, r.exact, r.tau, "plan lifecycle %s" % name)
        R.check_against_oracle(got, r, what="plan lifecycle %s" % name)
    sp.close()
    other.close()


def test_two_threads_make_their_first_f_call_at_once(lib, torch_cuda):
    """Five tapers at N = 2048, the smallest size that takes the paired tables: two threads, each on its own stream, make the
    plan's first F call together.  Both results are the bits of a single-threaded call on a fresh plan."""
    torch = torch_cuda
    n = 2048
    params = lib.MtmParams(n=n, overlap=0.0, w=2.5, kmax=4)
    x = torch.from_numpy(synth(9 * n, seed=7)).cuda()
    ref = lib.Spectrogram(params)
    want = ref.ftest(x)
    torch.cuda.synchronize()
    sp = lib.Spectrogram(params)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    gate = threading.Barrier(2)
    got, errors = [None, None], []

    def work(k):
        try:
            with torch.cuda.stream(streams[k]):
                gate.wait(timeout=30)
                got[k] = sp.ftest(x)
                streams[k].synchronize()
        except Exception as e:                               # (reported by the test's thread below)
            errors.append(e)

    threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for k in range(2):
        assert torch.equal(_bits(torch, got[k]), _bits(torch, want))
    # and the tables the two calls left behind serve the next call
    assert torch.equal(_bits(torch, sp.ftest(x)), _bits(torch, want))
    torch.cuda.synchronize()
    sp.close()
    ref.close()
