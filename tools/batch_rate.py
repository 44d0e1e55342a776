"""One batch call (Spectrogram.run_batch, glfer_hip_spectrogram_batch_device) against B single-stream calls queued back to
back on one stream (Spectrogram.run), on the same data and into the same rows.  GPU time per call from events around
the whole call sequence (median of --reps).
    python tools/batch_rate.py [--case a|b0|b1|c ...] [--reps 5]
  a   C3 shape (MTM N=4096, 5 tapers, overlap 0): 256 streams x 7 200 000 f32 samples (10 min at 12 kHz)
  b0  C2 shape (Hanning N=4096, 75 %): 4 096 streams x 48 000 samples, sub_mean 0
  b1  the same, sub_mean 1 (the reference's mean removal)
  c   C3 shape, 1 stream of 2^30 samples (bench.py's stream)"""
import argparse
import sys

sys.path.insert(0, ".")
import torch
import glfer_amd as G

CASES = {
    "a": ("C3 shape, B=256 x 7 200 000", G.MtmParams, dict(n=4096, overlap=0.0, w=2.5, kmax=4), 256, 7200000),
    "b0": ("C2 shape, B=4096 x 48 000, sub_mean 0", G.FftParams, dict(n=4096, window_type=0, overlap=0.75), 4096, 48000),
    "b1": ("C2 shape, B=4096 x 48 000, sub_mean 1", G.FftParams, dict(n=4096, window_type=0, overlap=0.75, sub_mean=1), 4096, 48000),
    "c": ("C3 shape, B=1 x 2^30", G.MtmParams, dict(n=4096, overlap=0.0, w=2.5, kmax=4), 1, 1 << 30),
}


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
    for key in args.case or ["a", "b0", "b1", "c"]:
        name, P, kw, nb, nsamples = CASES[key]
        if args.streams:
            nb, name = args.streams, name.replace("B=%d" % nb, "B=%d" % args.streams)
        sp = G.Spectrogram(P(**kw))
        g = torch.Generator(device="cuda").manual_seed(1)
        x = torch.randn((nb, nsamples), device="cuda", generator=g) * 0.2
        x += torch.linspace(-0.1, 0.1, nb, device="cuda")[:, None]
        nf = sp.num_frames(nsamples)
        out = torch.empty((nb, nf, sp.pitch), device="cuda")

        def batch():
            sp.run_batch(x, out=out)

        def loop():
            for b in range(nb):
                sp.run(x[b], out=out[b])

        batch()
        torch.cuda.synchronize()
        if args.batch_only:
            tb = stats([once(batch) for _ in range(args.reps)])
        else:
            ref = out.clone()
            loop()
            torch.cuda.synchronize()
            assert torch.equal(out, ref), "batch rows differ from the loop's"
            tbs, tls = [], []
            for _ in range(args.reps):                   # interleaved, so that neither side gets the box's better moments
                tbs.append(once(batch))
                tls.append(once(loop))
            tb, tl = stats(tbs), stats(tls)
        line = "%-40s frames %9d  batch %9.3f ms (min %.3f max %.3f)  %8.2f M frames/s" % (
            name, nb * nf, tb[0], tb[1], tb[2], nb * nf / tb[0] / 1e3)
        if not args.batch_only:
            line += "  |  loop of %d calls %9.3f ms (min %.3f max %.3f)  speed-up x%.2f" % (nb, tl[0], tl[1], tl[2], tl[0] / tb[0])
        print(line, flush=True)
        del x, out
        sp.close()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
