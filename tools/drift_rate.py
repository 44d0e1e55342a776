"""The drift search (drift_sums, drift_sums_batch, Spectrogram.run_drift) timed on one MI355X: device-resident float32 rows, events on
the launch stream, --reps repetitions after a warm-up call, medians and ranges.  Every figure is printed beside the arithmetic it
is judged by: the HBM time of the algorithmic bytes (the rows read once, the outputs written; 6.29 TB/s, the measured float4 copy
rate), the LDS time of T words per sum (ds_read_b32: 75 TB/s over the chip) and the time of T float adds per sum (78.6 T adds/s).
    python tools/drift_rate.py                 the table of profiles/drift_rate.txt
    python tools/drift_rate.py --run-headline  Spectrogram.run alone on the headline shape (multitaper N = 4096, K = 4, 2^28 samples):
                                               run in alternating processes with GLFER_LIB_PATH at the parent commit's library
    python tools/drift_rate.py --small         the same code paths at toy sizes (a rehearsal, not a measurement)"""
import argparse
import sys

sys.path.insert(0, ".")
import numpy as np
import torch
import glfer_amd as G

HBM, LDS32, ADDS = 6.29e12, 75e12, 78.6e12


def once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = sorted(once(fn) for _ in range(reps))
    return ts[len(ts) // 2], ts[0], ts[-1]


def ms(t):
    return "%9.3f ms (min %.3f max %.3f)" % t


def composition(rows, T, dmin, dmax):
    """what a caller had: one shifted slice-add per (d, t) over all disjoint blocks at once, then max / argmax (the largest sum;
    torch's argmax has its own tie rule)"""
    F, bins = rows.shape
    nb, D = F // T, dmax - dmin + 1
    blocks = rows[:nb * T].view(nb, T, bins)
    offs = G.drift_offsets(T, dmin, dmax)
    acc = torch.zeros((nb, D, bins), dtype=torch.float32, device=rows.device)
    for j in range(D):
        for t in range(T):
            o = int(offs[j, t])
            lo, hi = max(0, -o), min(bins, bins - o)
            acc[:, j, lo:hi] += blocks[:, t, lo + o:hi + o]
    best, arg = acc.max(dim=1)
    return acc, best, arg


def table(F, bins, reps, with_torch):
    g = torch.Generator(device="cuda").manual_seed(1)
    rows = torch.empty((F, bins), device="cuda").exponential_(generator=g)
    print("rows: %d x %d float32 (%.2f GB), resident" % (F, bins, F * bins * 4 / 1e9))
    for T, reach in ((16, 15), (64, 32), (64, 63)):
        D = 2 * reach + 1
        for step in (T, T // 4):
            nb = G.drift_blocks(F, T, step)
            sums = nb * D * bins
            print("T = %d, drifts -%d .. %d (%d), step %d: %d blocks, %.3g sums of %d terms" % (T, reach, reach, D, step, nb, sums, T))
            print("    arithmetic: %.3f ms of LDS words, %.3f ms of float adds" % (sums * T * 4 / LDS32 * 1e3, sums * T / ADDS * 1e3))
            for want in (("best", "drift"), ("sums", "best", "drift")):
                out_bytes = nb * bins * 6 + (sums * 4 if "sums" in want else 0)
                out = G.api._drift_outs(want, None, (), nb, D, bins, rows.device)
                t = timed(lambda: G.drift_sums(rows, T, step, -reach, reach, want=want, out=out), reps)
                hbm = (F * bins * 4 + out_bytes) / HBM * 1e3
                print("    %-18s %s  %8.2f M rows/s  HBM time of the bytes %.3f ms (x%.1f)" %
                      ("+".join(want), ms(t), F / t[0] / 1e3, hbm, t[0] / hbm))
                del out
            if with_torch and step == T:
                small = rows[:min(F, 4096 * T)]                    # 4 096 blocks: the composition's sums alone take 4 D bins bytes a block
                t = timed(lambda: composition(small, T, -reach, reach), max(2, reps // 3))
                lib_t = timed(lambda: G.drift_sums(small, T, T, -reach, reach, want=("sums", "best", "drift")), reps)
                print("    torch composition over %d blocks (%d slice-adds, max, argmax) %s; drift_sums with sums on the same rows %s: x%.0f" %
                      (small.shape[0] // T, D * T, ms(t), ms(lib_t), t[0] / lib_t[0]))
    del rows


def batch(nstreams, F, bins, reps):
    g = torch.Generator(device="cuda").manual_seed(2)
    rows = torch.empty((nstreams, F, bins), device="cuda").exponential_(generator=g)
    T, reach = 16, 15
    one = timed(lambda: G.drift_sums_batch(rows, T, T, -reach, reach), reps)

    def loop():
        for b in range(nstreams):
            G.drift_sums(rows[b], T, T, -reach, reach)
    many = timed(loop, max(2, reps // 3))
    got, ref = G.drift_sums_batch(rows, T, T, -reach, reach), [G.drift_sums(rows[b], T, T, -reach, reach) for b in (0, nstreams - 1)]
    assert torch.equal(got.best[0], ref[0].best) and torch.equal(got.drift[-1], ref[1].drift)
    print("%d streams of %d rows x %d bins, T = 16, -15 .. 15, best + drift" % (nstreams, F, bins))
    print("    drift_sums_batch   %s" % ms(one))
    print("    loop of drift_sums %s   loop / batch x%.1f" % (ms(many), many[0] / one[0]))


def run_drift(nsamples, reps):
    sp = G.Spectrogram(G.FftParams(n=4096, window_type=G.WINDOWS["hanning"], overlap=0.0))
    g = torch.Generator(device="cuda").manual_seed(3)
    x = torch.randn(nsamples, device="cuda", generator=g) * 0.2
    T = 16
    fused = timed(lambda: sp.run_drift(x, T), reps)

    def two():
        return G.drift_sums(sp.run(x), T)
    both = timed(two, reps)
    rows_only = timed(lambda: sp.run(x), reps)
    a, b = sp.run_drift(x, T), two()
    assert torch.equal(a.best, b.best) and torch.equal(a.drift, b.drift)
    print("periodogram N = 4096, %d frames, T = 16, -15 .. 15, best + drift" % sp.num_frames(nsamples))
    print("    run_drift          %s" % ms(fused))
    print("    run + drift_sums   %s   (run alone %s)" % (ms(both), ms(rows_only)))


def run_headline(reps):
    sp = G.Spectrogram(G.MtmParams(n=4096, overlap=0.0, w=2.5, kmax=4))
    g = torch.Generator(device="cuda").manual_seed(4)
    x = torch.randn(1 << 28, device="cuda", generator=g) * 0.2
    out = torch.empty((sp.num_frames(x.numel()), sp.pitch), device="cuda")
    t = timed(lambda: sp.run(x, out=out), reps)
    print("run, multitaper N = 4096 K = 4, %d frames: %s  %s" % (out.shape[0], ms(t), G.api.LIB_PATH))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--run-headline", action="store_true")
    ap.add_argument("--small", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    if a.run_headline:
        return run_headline(a.reps)
    if a.small:
        table(1 << 10, 257, 2, True)
        batch(8, 64, 257, 2)
        return run_drift(1 << 20, 2)
    table(1 << 17, 2049, a.reps, True)
    batch(4096, 64, 2049, a.reps)
    run_drift(1 << 28, a.reps)


if __name__ == "__main__":
    main()
