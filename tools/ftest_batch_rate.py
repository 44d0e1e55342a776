"""The batched harmonic F-test (Spectrogram.ftest_batch, glfer_hip_mtm_ftest_batch_device) against B single-stream calls queued
back to back on one stream (Spectrogram.ftest), on the same data, same library, same process.  GPU time per call sequence from
events (median of --reps, batch and loop interleaved).
    python tools/ftest_batch_rate.py [--case KEY ...] [--reps 5]
  shapes   s: 4 096 streams x 48 000 f32 samples (one second at 48 kHz)      l: 256 streams x 28 800 000 (ten minutes at 48 kHz)
  plans    4096: MTM N=4096, 5 tapers (NW 2.5), overlap 0                    1024: MTM N=1024, 8 tapers (NW 4), overlap 0
  means    m0: sub_mean 0        m1: sub_mean 1 (the reference's mean removal)
  a case key is shape + plan + means, e.g. s4096m0, l1024m1
    python tools/ftest_batch_rate.py --single [--reps 7]
  the single-stream entry alone on one stream of 2^28 samples per plan (the rate an A/B of two builds compares; GLFER_LIB_PATH
  selects the library)
    python tools/ftest_batch_rate.py --case KEY --streams B --batch-only --reps 2       (under rocprofv3 --kernel-trace --stats)
    python tools/ftest_batch_rate.py --count DIR --calls 3
  the library's dispatches in the newest *_kernel_stats.csv under DIR, per batched call"""
import argparse
import csv
import glob
import os
import sys

sys.path.insert(0, ".")

SHAPES = {"s": (4096, 48000), "l": (256, 28800000)}
PLANS = {"4096": ("MTM N=4096, 5 tapers", dict(n=4096, overlap=0.0, w=2.5, kmax=4)),
         "1024": ("MTM N=1024, 8 tapers", dict(n=1024, overlap=0.0, w=4.0, kmax=7))}
KEYS = [s + p + m for s in "sl" for p in ("4096", "1024") for m in ("m0", "m1")]


def once(torch, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def stats(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2], ts[0], ts[-1]


def count(directory, calls):
    files = glob.glob(os.path.join(directory, "**", "*_kernel_stats.csv"), recursive=True)
    rows = list(csv.DictReader(open(max(files, key=os.path.getmtime))))
    ours = [(r["Name"], int(r["Calls"])) for r in rows if "glfer" in r["Name"]]
    total = sum(c for _, c in ours)
    print("%d glfer dispatches over %d batched calls = %g per call" % (total, calls, total / calls))
    for name, c in sorted(ours):
        print("    %-110s x%d" % (name[:110], c))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", action="append", choices=KEYS)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batch-only", action="store_true", help="time the batched call only (profiler runs)")
    ap.add_argument("--streams", type=int, default=0, help="B other than the shape's own")
    ap.add_argument("--single", action="store_true", help="the single-stream entry's rate on one long stream")
    ap.add_argument("--count", metavar="DIR", help="summarise a rocprofv3 --kernel-trace --stats output directory")
    ap.add_argument("--calls", type=int, default=3, help="batched calls the traced run made (with --count)")
    args = ap.parse_args()
    if args.count:
        return count(args.count, args.calls)
    import torch
    import glfer_amd as G
    if args.single:
        for key in ("4096", "1024"):
            name, kw = PLANS[key]
            sp = G.Spectrogram(G.MtmParams(**kw))
            x = torch.randn(1 << 28, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1)) * 0.2
            nf = sp.num_frames(x.numel())
            sp.ftest(x)
            torch.cuda.synchronize()
            t = stats([once(torch, lambda: sp.ftest(x)) for _ in range(args.reps)])
            print("single %-24s frames %8d  %8.3f ms (min %.3f max %.3f)  %7.2f M frames/s (best %.2f)  %s" % (
                name, nf, t[0], t[1], t[2], nf / t[0] / 1e3, nf / t[1] / 1e3, os.environ.get("GLFER_LIB_PATH") or "this tree"),
                flush=True)
            del x
            sp.close()
            torch.cuda.empty_cache()
        return
    for key in args.case or KEYS:
        nb, nsamples = SHAPES[key[0]]
        pname, kw = PLANS[key[1:5]]
        sub = int(key[-1])
        nb = args.streams or nb
        name = "%s, sub_mean %d, B=%d x %d" % (pname, sub, nb, nsamples)
        sp = G.Spectrogram(G.MtmParams(sub_mean=sub, **kw))
        g = torch.Generator(device="cuda").manual_seed(1)
        x = torch.empty((nb, nsamples), device="cuda")
        for b in range(nb):                            # (stream by stream: no second copy of a 29 GB batch)
            x[b].normal_(0.1 * (2.0 * b / max(nb - 1, 1) - 1.0), 0.2, generator=g)
        nf = sp.num_frames(nsamples)
        out = torch.empty((nb, nf, sp.bins), device="cuda")

        def batch():
            sp.ftest_batch(x, out=out)

        def loop():
            return [sp.ftest(x[b]) for b in range(nb)]

        batch()
        torch.cuda.synchronize()
        if args.batch_only:
            tb = stats([once(torch, batch) for _ in range(args.reps)])
        else:
            rows = loop()
            torch.cuda.synchronize()
            for b in (0, nb // 2, nb - 1):
                assert torch.equal(out[b].view(torch.int32), rows[b].view(torch.int32)), "batch rows differ from the loop's"
            del rows
            tbs, tls = [], []
            for _ in range(args.reps):                   # interleaved, so that neither side gets the box's better moments
                tbs.append(once(torch, batch))
                tls.append(once(torch, loop))
            tb, tl = stats(tbs), stats(tls)
        line = "%-52s frames %8d  batch %9.3f ms (min %.3f max %.3f) %7.2f M frames/s" % (
            name, nb * nf, tb[0], tb[1], tb[2], nb * nf / tb[0] / 1e3)
        if not args.batch_only:
            line += "  |  loop of %d calls %9.3f ms (min %.3f max %.3f)  x%.2f" % (nb, tl[0], tl[1], tl[2], tl[0] / tb[0])
        print(line, flush=True)
        del x, out
        sp.close()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
