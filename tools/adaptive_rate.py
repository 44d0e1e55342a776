#!/usr/bin/env python3
"""What Spectrogram.adaptive costs on one GPU (profiles/adaptive_rate.txt is a run of this on an MI355X).

    adaptive_rate.py SHAPE            adaptive at 1, 8 and 32 sweeps against run() on the same plan and against the torch composition
    adaptive_rate.py SHAPE --run-only run() alone, one line: for alternating processes of two builds (GLFER_LIB_PATH names the other)

SHAPE: c3 (N = 4096, hop 4096, 5 tapers, w = 2.5: the benchmark's flagship) or mtm1024 (N = 1024, hop 512, 8 tapers, w = 4.5), on
2^28 f32 samples.  Events on the launch stream, six alternating repetitions after a warm-up, median (min max).  The composition:
unfold, float32 tapers, torch.fft.rfft, the same sweeps, in chunks of frames; it needs whole frames, so it skips the first frames
that reach into history and is timed on the rest."""
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, __import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.abspath(__file__))))
import glfer_amd as G  # noqa: E402

SHAPES = {"c3": (4096, 0.0, 2.5, 4), "mtm1024": (1024, 0.5, 4.5, 7)}
NSAMPLES = 1 << 28
REPS = 6


def timed(fns):
    """Median (min max) milliseconds of each function, run alternately."""
    for f in fns:
        f()
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for _ in range(REPS):
        for i, f in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            b.synchronize()
            ms[i].append(a.elapsed_time(b))
    return [(statistics.median(m), min(m), max(m)) for m in ms]


def compose(x, n, hop, taps32, lam, beta, iters, chunk=4096):
    """The torch composition on whole frames: returns the rows of frames first .. (first: the first frame without history)."""
    first = -(-(n - hop) // hop)
    frames = x[first * hop - (n - hop):].unfold(0, n, hop)
    lam_t, beta_t = torch.from_numpy(lam).cuda(), torch.from_numpy(beta).cuda()
    out = torch.empty((frames.shape[0], n // 2 + 1), device="cuda")
    for c0 in range(0, frames.shape[0], chunk):
        fr = frames[c0:c0 + chunk]
        X = torch.fft.rfft(fr[:, None, :] * taps32[None, :, :], dim=2)
        E = (X.real * X.real + X.imag * X.imag) / n                                   # [F][K][bins]
        B = beta_t[None, :] * ((fr * fr).sum(dim=1) / n)[:, None] / n                 # [F][K]
        S = 0.5 * (E[:, 0] + E[:, 1])
        for _ in range(iters):
            num = lam_t[0] * S + B[:, 0, None]
            den = lam_t[None, :, None] * S[:, None, :] + B[:, :, None]
            u = torch.where(den == 0, torch.ones_like(den), num[:, None, :] / den)
            w = lam_t[None, :, None] * u * u
            S = (w * E).sum(dim=1) / w.sum(dim=1)
        out[c0:c0 + chunk] = S
    return first, out


def main():
    shape = sys.argv[1]
    n, overlap, w, kmax = SHAPES[shape]
    params = G.MtmParams(n=n, overlap=overlap, w=w, kmax=kmax)
    sp = G.Spectrogram(params)
    x = torch.randn(NSAMPLES, device="cuda:0") * 0.2
    nframes = sp.num_frames(NSAMPLES)
    rows = torch.empty((nframes, sp.pitch), device="cuda:0")
    if "--run-only" in sys.argv:
        (t,) = timed([lambda: sp.run(x, out=rows)])
        print("%s run %8.3f ms (%.3f %.3f) %9.3f M frames/s  lib %s" % (shape, t[0], t[1], t[2], nframes / t[0] / 1e3, G.api.LIB_PATH))
        return
    outs = {"psd": torch.empty((nframes, n // 2 + 1), device="cuda:0"), "dof": torch.empty((nframes, n // 2 + 1), device="cuda:0")}
    psd_only = {"psd": outs["psd"]}
    fns = [lambda: sp.run(x, out=rows)]
    names = ["run"]
    for it in (1, 8, 32):
        fns.append(lambda it=it: sp.adaptive(x, iters=it, out=outs))
        names.append("adaptive %2d" % it)
    fns.append(lambda: sp.adaptive(x, iters=8, want=("psd",), out=psd_only))
    names.append("psd only  8")
    res = timed(fns)
    print("## %s: N = %d, hop %d, %d tapers, w = %.1f, 2^28 f32 samples, %d frames" % (shape, n, sp.hop, kmax + 1, w, nframes))
    for nm, t in zip(names, res):
        print("%-12s %8.3f ms (%.3f %.3f) %9.3f M frames/s   %.2fx run" % (nm, t[0], t[1], t[2], nframes / t[0] / 1e3, t[0] / res[0][0]))
    # the composition on a sixteenth of the stream (it allocates [frames][K][bins] complex per chunk)
    lam, beta = G.adaptive_weights(params)
    taps32 = torch.from_numpy(np.asarray(sp.tapers()[0], np.float32)).cuda()
    xs = x[:NSAMPLES // 16]
    for it in (1, 8, 32):
        (t,) = timed([lambda it=it: compose(xs, n, sp.hop, taps32, lam, beta, it)])
        first, got = compose(xs, n, sp.hop, taps32, lam, beta, it)
        want = sp.adaptive(xs, iters=it, want=("psd",)).psd[first:]
        err = ((got.sqrt() - want.sqrt()).abs().max(dim=1).values / want.sqrt().max(dim=1).values)[:64].max().item()
        fps = got.shape[0] / t[0] / 1e3
        print("compose   %2d %8.3f ms (%.3f %.3f) %9.3f M frames/s on %d frames; adaptive: %.1fx its frames/s; max amplitude difference / row max over 64 rows %.2e"
              % (it, t[0], t[1], t[2], fps, got.shape[0], nframes / res[1 + (1, 8, 32).index(it)][0] / 1e3 / fps, err))
    hop_bytes = 4 * sp.hop + 8 * (n // 2 + 1)
    print("algorithmic bytes %d per frame (4 H + 8 (N/2 + 1), both outputs): %.2f TB/s at 8 sweeps" % (hop_bytes, hop_bytes * nframes / res[2][0] / 1e9))


if __name__ == "__main__":
    main()
