"""Shared by the ragged moving-average and waterfall tests: packed rows, and a numpy restatement of the chunked sliding sum.

The kernels cut a stream's frames into chunks of `avg_chunk(nframes)` frames.  Within a chunk the sliding sum is the
reference's recurrence (avg.c:116-127) in double; a chunk starts from a direct sum, in frame order, of the (up to depth) rows
before it.  The two agree only while every addition is exact, so with rows that swing by more than 2^26 inside a window the
sums carry their chunk length in their last bits -- which is why a ragged call must take every stream's OWN chunk length.
"""
import numpy as np


def avg_chunk(nframes):
    """the chunk length the single-stream launchers take for a stream of nframes frames"""
    chunk = 128
    while chunk > 8 and nframes // chunk < 1024:
        chunk //= 2
    return chunk


def chunked_sums(x, depth, chunk):
    """x: float32 [frames][bins].  The sliding sums [frames][bins] in float64, chunk by chunk: restart, then the recurrence."""
    x = np.asarray(x, np.float32)
    frames = x.shape[0]
    out = np.empty(x.shape, np.float64)
    for f0 in range(0, frames, chunk):
        cum = np.zeros(x.shape[1], np.float64)
        for g in range(max(f0 - depth, 0), f0):
            cum = cum + x[g].astype(np.float64)
        for f in range(f0, min(f0 + chunk, frames)):
            if f < depth:
                cum = cum + x[f].astype(np.float64)
            else:
                cum = cum + (x[f].astype(np.float64) - x[f - depth].astype(np.float64))
            out[f] = cum
    return out


def swinging_rows(frames, bins, seed):
    """float32 rows whose bins swing between ~1e-8 and ~1e8 from frame to frame, irregularly: more than 2^26 inside any window
    of a few frames, and no period that would let the differences of the recurrence cancel exactly"""
    rng = np.random.default_rng(seed)
    high = rng.random((frames, bins)) < 0.5
    mant = 1.0 + rng.random((frames, bins))
    return np.where(high, 1e8 * mant, 1e-8 * mant).astype(np.float32)


def row_starts(lengths):
    return np.concatenate([[0], np.cumsum(np.asarray(lengths, np.int64))]).astype(np.int64)


def psd_rows(torch, lengths, bins, seed, width=None):
    """PSD-like packed rows [sum(lengths)][width or bins] on the GPU: non-negative, another scale and floor per stream"""
    total = int(sum(lengths))
    g = torch.Generator(device="cuda:0").manual_seed(seed)
    x = torch.rand((total, width or bins), generator=g, device="cuda:0", dtype=torch.float32)
    x = x * x * x * x
    at = 0
    for b, n in enumerate(lengths):
        x[at:at + n] = x[at:at + n] * 10.0 ** ((b * 37) % 7 - 3) + 1e-4 * ((b * 13) % 5)
        at += n
    return x.contiguous()
