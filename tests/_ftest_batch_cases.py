"""Inputs of the batched F-test's oracle parity (tests only): per in-launch form one case of tests/_ftest_cases.py's matrix,
four streams each.  Stream 0 is the matrix input itself; the others are the same kind of signal from another seed, at another
amplitude and on a small DC level, so that no two streams of a batch share a row.  tests/test_ftest_batch_host.py holds the
reference alone to the acceptance rule on every one of these streams, without a GPU; tests/test_gpu_ftest_batch.py then
judges the device's batched rows by the same rule."""
import functools

import numpy as np

import _ftest_cases as K
from _exact import ftest64, hop_len
from _signals import synth

# one per in-launch form by default: one sequence per transform (N = 1024), two per transform (N = 4096)
PARITY_CASES = [K.case(1024, 0.0, 2.5, 4, 13, "noise"), K.case(4096, 0.0, 4.5, 8, 7)]
NSTREAMS = 4
AMPS = (1.0, 0.7, 0.55, 0.85)                 # (no powers of two: F is invariant under those, bit for bit)
DCS = (0.0, 0.02, -0.03, 0.01)


def stream(oracle, c, b):
    """float32 samples of stream b of the case's batch."""
    assert c.fmt == "f32" and 0 <= b < NSTREAMS
    x0 = K.make_input(oracle, c)[1]
    if b == 0:
        return x0
    count = len(x0)
    assert count == c.frames * hop_len(c.n, c.ovl) + min(3, hop_len(c.n, c.ovl) - 1)
    seed = c.n + 7 * c.kmax + c.frames + 100 * b
    if c.signal == "noise":
        x = 0.25 * np.random.default_rng(seed).standard_normal(count)
    else:
        x = synth(count, fs=8000.0, seed=seed).astype(np.float64)
    x = AMPS[b] * x + DCS[b]
    return np.clip(x, -1.0, np.nextafter(1.0, 0.0)).astype(np.float32)


@functools.lru_cache(maxsize=8)
def reference(oracle, c, b):
    """(x, want, num, den) of stream b: the samples, the oracle's F rows (mu live) and the float64 weights of the bound."""
    x = stream(oracle, c, b)
    _, want = oracle.spectrogram_mtm_ftest(x, c.n, c.ovl, c.nw, c.kmax, sub_mean=0, history_mode=0, mu_live=1)
    num, den, _ = ftest64(x, c.n, c.ovl, K._tapers(oracle, c.n, c.kmax, c.nw), c.kmax, sub_mean=0, history_mode=0)
    assert want.shape == num.shape == (c.frames, c.n // 2 + 1)
    return x, want, num, den
