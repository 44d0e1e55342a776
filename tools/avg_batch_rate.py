"""One batched estimator-plus-average call (Spectrogram.run_avg_batch, glfer_hip_spectrogram_avg_batch_device) against B
single-stream calls queued back to back on one stream (Spectrogram.run_avg), on the same data.  update_avg_plain, depth 4,
over the whole band, return values on, PSD rows not stored.  GPU time per call from events around the whole call
sequence (median of --reps, batch and loop interleaved).
    python tools/avg_batch_rate.py [--case a|b0|b1|c ...] [--reps 5]
  b0  C2 shape (Hanning N=4096, 75 %): 4 096 streams x 48 000 samples (one second at 48 kHz), sub_mean 0: the two launches
  b1  the same, sub_mean 1 (the reference's mean removal)
  a   C2 shape, 256 streams x 7 200 000 samples (ten minutes at 12 kHz), sub_mean 0: the average inside the estimator launch
  c   C2 shape, 1 stream of 2^28 samples: B = 1 is the single-stream path itself"""
import argparse
import sys

sys.path.insert(0, ".")
import torch
import glfer_amd as G

C2 = dict(n=4096, window_type=0, overlap=0.75)
CASES = {
    "b0": ("C2 + avg, B=4096 x 48 000, sub_mean 0", dict(C2), 4096, 48000),
    "b1": ("C2 + avg, B=4096 x 48 000, sub_mean 1", dict(C2, sub_mean=1), 4096, 48000),
    "a": ("C2 + avg, B=256 x 7 200 000", dict(C2), 256, 7200000),
    "c": ("C2 + avg, B=1 x 2^28", dict(C2), 1, 1 << 28),
}
DEPTH = 4


def once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def stats(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2], ts[0], ts[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", action="append", choices=sorted(CASES))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batch-only", action="store_true", help="time the batch call only (profiler runs)")
    ap.add_argument("--streams", type=int, default=0, help="B other than the case's own")
    args = ap.parse_args()
    for key in args.case or ["b0", "b1", "a", "c"]:
        name, kw, nb, nsamples = CASES[key]
        if args.streams:
            nb, name = args.streams, name.replace("B=%d" % nb, "B=%d" % args.streams)
        sp = G.Spectrogram(G.FftParams(**kw))
        g = torch.Generator(device="cuda").manual_seed(1)
        x = torch.randn((nb, nsamples), device="cuda", generator=g) * 0.2
        x += torch.linspace(-0.1, 0.1, nb, device="cuda")[:, None]
        nf = sp.num_frames(nsamples)
        bins = sp.bins
        res = {}

        def batch():
            res["batch"] = sp.run_avg_batch(x, G.AVG_PLAIN, DEPTH, 0, bins)

        def loop():
            res["loop"] = [sp.run_avg(x[b], G.AVG_PLAIN, DEPTH, 0, bins) for b in range(nb)]

        batch()
        torch.cuda.synchronize()
        if args.batch_only:
            tb = stats([once(batch) for _ in range(args.reps)])
        else:
            loop()
            torch.cuda.synchronize()
            avg, ret, _ = res["batch"]
            for b, (wa, wr, _) in enumerate(res["loop"]):
                assert torch.equal(avg[b], wa) and torch.equal(ret[b], wr), "batch stream %d differs from the loop's" % b
            res.clear()
            tbs, tls = [], []
            for _ in range(args.reps):                   # interleaved, so that neither side gets the box's better moments
                tbs.append(once(batch))
                res.clear()
                tls.append(once(loop))
                res.clear()
            tb, tl = stats(tbs), stats(tls)
        line = "%-40s frames %9d  batch %9.3f ms (min %.3f max %.3f)  %8.2f M frames/s" % (
            name, nb * nf, tb[0], tb[1], tb[2], nb * nf / tb[0] / 1e3)
        if not args.batch_only:
            line += "  |  loop of %d calls %9.3f ms (min %.3f max %.3f)  speed-up x%.2f" % (nb, tl[0], tl[1], tl[2], tl[0] / tb[0])
        print(line, flush=True)
        res.clear()
        del x
        sp.close()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
