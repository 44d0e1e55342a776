#!/usr/bin/env python3
"""What Spectrogram.jackknife costs on one GPU (profiles/jackknife_rate.txt is a run of this on an MI355X).

    jackknife_rate.py SHAPE                  jackknife at 0 and 8 sweeps against adaptive at 8 and run() on the same plan and samples
    jackknife_rate.py SHAPE --adaptive-only  adaptive at 8 sweeps alone, one line: for alternating processes of two builds
                                             (GLFER_LIB_PATH names the other build's library)
    jackknife_rate.py batch                  jackknife_batch on 4096 one-second streams against the loop of jackknife

SHAPE: c3 (N = 4096, hop 4096, 5 tapers, w = 2.5: the benchmark's flagship) or mtm1024 (N = 1024, hop 512, 8 tapers, w = 4.5), on
2^28 f32 samples.  Events on the launch stream, six alternating repetitions after a warm-up, median (min max)."""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
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


def shape(name):
    n, overlap, w, kmax = SHAPES[name]
    sp = G.Spectrogram(G.MtmParams(n=n, overlap=overlap, w=w, kmax=kmax))
    x = torch.randn(NSAMPLES, device="cuda:0") * 0.2
    nframes = sp.num_frames(NSAMPLES)
    bins = n // 2 + 1
    outs = {f: torch.empty((nframes, bins), device="cuda:0") for f in G.Jackknife._fields}
    two = {f: outs[f] for f in G.Adaptive._fields}
    if "--adaptive-only" in sys.argv:
        (t,) = timed([lambda: sp.adaptive(x, iters=8, out=two)])
        print("%s adaptive 8 %8.3f ms (%.3f %.3f) %9.3f M frames/s  lib %s" % (name, t[0], t[1], t[2], nframes / t[0] / 1e3, G.api.LIB_PATH))
        return
    rows = torch.empty((nframes, sp.pitch), device="cuda:0")
    fns = [lambda: sp.run(x, out=rows), lambda: sp.adaptive(x, iters=8, out=two), lambda: sp.jackknife(x, iters=0, out=outs),
           lambda: sp.jackknife(x, iters=8, out=outs), lambda: sp.jackknife(x, iters=8, want=("logvar",), out={"logvar": outs["logvar"]})]
    names = ["run", "adaptive   8", "jackknife  0", "jackknife  8", "logvar only 8"]
    res = timed(fns)
    print("## %s: N = %d, hop %d, %d tapers, w = %.1f, 2^28 f32 samples, %d frames" % (name, n, sp.hop, kmax + 1, w, nframes))
    for nm, t in zip(names, res):
        print("%-13s %8.3f ms (%.3f %.3f) %9.3f M frames/s   %.2fx run   %.2fx adaptive 8"
              % (nm, t[0], t[1], t[2], nframes / t[0] / 1e3, t[0] / res[0][0], t[0] / res[1][0]))
    print("the statistic itself: jackknife 8 - adaptive 8 = %.3f ms, %.2f ps a bin; jackknife 0 - run = %.3f ms"
          % (res[3][0] - res[1][0], (res[3][0] - res[1][0]) * 1e9 / (nframes * bins), res[2][0] - res[0][0]))


def batch():
    B, S = 4096, 48000
    sp = G.Spectrogram(G.MtmParams(n=1024, overlap=0.5, w=4.5, kmax=7))
    x = torch.randn((B, S), device="cuda:0") * 0.2
    frames = sp.num_frames(S)
    outs = {f: torch.empty((B, frames, 513), device="cuda:0") for f in G.Jackknife._fields}

    def loop():
        for b in range(B):
            sp.jackknife(x[b], iters=8, out={f: o[b] for f, o in outs.items()})
    res = timed([lambda: sp.jackknife_batch(x, iters=8, out=outs), loop])
    print("## batch: %d streams of %d f32 samples (one second at 48 kHz), N = 1024, 8 tapers, 50 %%, 8 sweeps: %d frames a stream" % (B, S, frames))
    for nm, t in zip(("jackknife_batch", "loop of jackknife"), res):
        print("%-18s %9.3f ms (%.3f %.3f) %9.3f M frames/s" % (nm, t[0], t[1], t[2], B * frames / t[0] / 1e3))
    print("the batch: %.1fx the loop" % (res[1][0] / res[0][0]))


if __name__ == "__main__":
    batch() if sys.argv[1] == "batch" else shape(sys.argv[1])
