"""LMP plans through the batch and ragged entries in one launch set, against what a caller had before: a loop of run().
Device-resident f32 streams, events on the launch stream, --reps alternating repetitions, medians and ranges (the method of
tools/ragged_ftest_rate.py).  N = 1024, lmp_av = 4, overlap 0 (the bench.py row "lmp").
    python tools/lmp_batch_rate.py [--case short|long ...] [--reps 6]
  short  4 096 streams of 1 s at 48 kHz (run_batch) and of 0.5 .. 1.5 s (run_ragged), with and without sub_mean = 1
  long   256 streams of ten minutes at 12 kHz
    python tools/lmp_batch_rate.py --loop        the loop of run() alone (also on another build: GLFER_LIB_PATH)
    python tools/lmp_batch_rate.py --single      single-stream run(), 2^20 frames (run in alternating processes, GLFER_LIB_PATH
                                                 at another build)
    python tools/lmp_batch_rate.py --stage       the statistic alone (lmp_statistic, _batch, _ragged) over 65 536 rows at ring sizes
                                                 the plans above do not reach: lmp_av = 100 (frame by frame) and 16 (the ring in
                                                 LDS), one stream, 16 streams as a batch and ragged (alternating processes as --single)
    python tools/lmp_batch_rate.py --launches B --entry batch|ragged [--sub-mean]
                                                 one call of B streams and nothing else (under rocprofv3 --kernel-trace)"""
import argparse
import sys

sys.path.insert(0, ".")
import numpy as np
import torch
import glfer_amd as G

N, AV = 1024, 4


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


def show(name, t):
    return "%-28s %9.3f ms (min %.3f max %.3f)" % (name, t[0], t[1], t[2])


def plan(sub_mean):
    return G.Spectrogram(G.LmpParams(n=N, overlap=0.0, avg=AV, sub_mean=sub_mean))


def bits(t):
    return t.view(torch.int32)


def streams(nb, lo, hi, seed):
    lens = np.full(nb, lo) if lo == hi else np.random.RandomState(seed).randint(lo, hi + 1, nb)
    offs = np.concatenate([[0], np.cumsum(lens)])[:-1]
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(int(lens.sum()), device="cuda", generator=g) * 0.2
    return x, offs, lens


def case(title, nb, lo, hi, sub_mean, reps, loop_only=False):
    sp = plan(sub_mean)
    x, offs, lens = streams(nb, lo, hi, 1)
    total, starts = sp.ragged_frames(lens)
    out = torch.empty((total, sp.bins), device="cuda")
    views = [x[int(o):int(o + n)] for o, n in zip(offs, lens)]
    span = [(int(starts[b]), int(starts[b + 1])) for b in range(nb)]

    def loop():
        for v, (r0, r1) in zip(views, span):
            if r1 > r0:
                sp.run(v, out=out[r0:r1])

    fns = [("loop of %d run() calls" % nb, loop)]
    if not loop_only:
        if lo == hi:
            fns.insert(0, ("run_batch", lambda: sp.run_batch(x.view(nb, lo), out=out)))
        fns.insert(0, ("run_ragged", lambda: sp.run_ragged(x, offs, lens, out=out)))
        loop()
        torch.cuda.synchronize()
        ref = out.clone()
        for name, fn in fns[:-1]:
            out.zero_()
            fn()
            torch.cuda.synchronize()
            assert torch.equal(bits(out), bits(ref)), "%s rows differ from the loop's" % name
        del ref
    for _, fn in fns:
        fn()
    torch.cuda.synchronize()
    ts = {name: [] for name, _ in fns}
    for _ in range(reps):                                    # alternating, so that no side gets the machine's better moments
        for name, fn in fns:
            ts[name].append(once(fn))
    tl = stats(ts[fns[-1][0]])
    print("%s, sub_mean %d: streams %d frames %d" % (title, sub_mean, nb, total))
    for name, _ in fns:
        t = stats(ts[name])
        print("    %s %8.2f M frames/s  loop / this x%.2f" % (show(name, t), total / t[0] / 1e3, tl[0] / t[0]))
    sys.stdout.flush()
    sp.close()
    del x, out, views
    torch.cuda.empty_cache()


def single(reps):
    sp = plan(0)
    frames = 1 << 20
    g = torch.Generator(device="cuda").manual_seed(3)
    x = torch.randn(frames * sp.hop, device="cuda", generator=g) * 0.2
    out = torch.empty((frames, sp.bins), device="cuda")
    for _ in range(3):
        sp.run(x, out=out)
    torch.cuda.synchronize()
    t = stats([once(lambda: sp.run(x, out=out)) for _ in range(reps)])
    print("single-stream run, N=%d lmp_av=%d, %d frames: %s %8.2f M frames/s" % (N, AV, frames, show("", t), frames / t[0] / 1e3), flush=True)


def stage(reps):
    frames, nb = 1 << 16, 16
    g = torch.Generator(device="cuda").manual_seed(5)
    P = torch.rand((frames, N // 2 + 1), device="cuda", generator=g) * 0.1 + 1e-3
    starts = np.arange(nb + 1) * (frames // nb)
    for avg in (100, 16):
        fns = [("one stream", lambda: G.lmp_statistic(P, avg)), ("batch of %d" % nb, lambda: G.lmp_statistic_batch(P.view(nb, frames // nb, -1), avg)),
               ("ragged, %d streams" % nb, lambda: G.lmp_statistic_ragged(P, starts, avg))]
        for _, fn in fns:
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        ts = {name: [] for name, _ in fns}
        for _ in range(reps):
            for name, fn in fns:
                ts[name].append(once(fn))
        for name, _ in fns:
            print("stage N=%d lmp_av=%d, %d rows, %s" % (N, avg, frames, show(name, stats(ts[name]))), flush=True)


def launches(nb, entry, sub_mean):
    sp = plan(sub_mean)
    if entry == "batch":
        x, offs, lens = streams(nb, 48000, 48000, 1)
        sp.run_batch(x.view(nb, 48000))
    else:
        x, offs, lens = streams(nb, 24000, 72000, 1)
        sp.run_ragged(x, offs, lens)
    torch.cuda.synchronize()
    print("one %s call, sub_mean %d, %d streams" % (entry, sub_mean, nb))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", action="append", choices=["short", "long"])
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--loop", action="store_true")
    ap.add_argument("--single", action="store_true")
    ap.add_argument("--stage", action="store_true")
    ap.add_argument("--launches", type=int, default=0)
    ap.add_argument("--entry", default="batch", choices=["batch", "ragged"])
    ap.add_argument("--sub-mean", action="store_true")
    args = ap.parse_args()
    if args.launches:
        return launches(args.launches, args.entry, 1 if args.sub_mean else 0)
    if args.single:
        return single(args.reps)
    if args.stage:
        return stage(args.reps)
    for c in args.case or ["short", "long"]:
        for sub_mean in (0, 1):
            if c == "short":
                case("4096 x 1 s at 48 kHz", 4096, 48000, 48000, sub_mean, args.reps, args.loop)
                case("4096 x 0.5-1.5 s at 48 kHz", 4096, 24000, 72000, sub_mean, args.reps, args.loop)
            else:
                case("256 x 10 min at 12 kHz", 256, 7200000, 7200000, sub_mean, args.reps, args.loop)


if __name__ == "__main__":
    main()
