"""HP-ARMA plans through the batch and ragged entries in one launch over all streams' frames, against what a caller had before:
a loop of run().  Device-resident f32 streams, events on the launch stream, --reps alternating repetitions, medians and ranges
(the method of tools/lmp_batch_rate.py).  BASELINE config 5: N = 4096, t = 128, p_e = 32, overlap 0 (the bench.py row "hparma").
    python tools/hparma_batch_rate.py [--case short|ragged|long ...] [--reps 3]
  short   4 096 streams of 1 s at 48 kHz: run_batch, without and with sub_mean = 1
  ragged  4 096 streams of 0.5 .. 1.5 s at 48 kHz: run_ragged
  long    256 streams of ten minutes at 12 kHz: run_batch and run_ragged
    python tools/hparma_batch_rate.py --loop        the loop of run() alone (also on another build: GLFER_LIB_PATH)
    python tools/hparma_batch_rate.py --ratio       256 streams of 2 frames: run_batch against the loop (the test's measurement)
    python tools/hparma_batch_rate.py --launches B --entry batch|ragged [--sub-mean S]
                                                    one call of B streams and nothing else (under rocprofv3 --kernel-trace)
The single-stream rate, parent against this tree: python bench.py --workload hparma in alternating processes, GLFER_LIB_PATH at
the parent's build for every other one."""
import argparse
import sys

sys.path.insert(0, ".")
import numpy as np
import torch
import glfer_amd as G

N, T, P_E = 4096, 128, 32


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
    return "%-28s %10.3f ms (min %.3f max %.3f)" % (name, t[0], t[1], t[2])


def plan(sub_mean):
    return G.Spectrogram(G.HparmaParams(n=N, overlap=0.0, t=T, p_e=P_E, sub_mean=sub_mean))


def bits(t):
    return t.view(torch.int32)


def streams(nb, lo, hi, seed):
    lens = np.full(nb, lo) if lo == hi else np.random.RandomState(seed).randint(lo, hi + 1, nb)
    offs = np.concatenate([[0], np.cumsum(lens)])[:-1]
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(int(lens.sum()), device="cuda", generator=g) * 0.2
    return x, offs, lens


def case(title, nb, lo, hi, sub_mean, reps, entries, loop_only=False):
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
        if "batch" in entries and lo == hi:
            fns.insert(0, ("run_batch", lambda: sp.run_batch(x.view(nb, lo), out=out)))
        if "ragged" in entries:
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
    print("%s, sub_mean %d: streams %d frames %d (rows bit for bit the loop's)" % (title, sub_mean, nb, total))
    for name, _ in fns:
        t = stats(ts[name])
        print("    %s %8.3f M frames/s  loop / this x%.2f" % (show(name, t), total / t[0] / 1e3, tl[0] / t[0]))
    sys.stdout.flush()
    sp.close()
    del x, out, views
    torch.cuda.empty_cache()


def ratio():
    """tests/test_gpu_hparma_batch.py::test_one_launch_not_one_per_stream: one warm-up each, the median of five"""
    sp = plan(0)
    B = 256
    x, offs, lens = streams(B, 2 * N, 2 * N, 2)
    xs = x.view(B, 2 * N)
    out = torch.empty((B, 2, sp.bins), device="cuda")
    views = [xs[b] for b in range(B)]

    def loop():
        for b in range(B):
            sp.run(views[b], out=out[b])

    res = {}
    for name, fn in (("run_batch", lambda: sp.run_batch(xs, out=out)), ("loop of 256 run() calls", loop)):
        fn()
        torch.cuda.synchronize()
        res[name] = stats([once(fn) for _ in range(5)])
        print("    %s" % show(name, res[name]))
    print("256 streams x 2 frames: loop / run_batch x%.1f (the test asserts >= 8)" % (res["loop of 256 run() calls"][0] / res["run_batch"][0]), flush=True)


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
    ap.add_argument("--case", action="append", choices=["short", "ragged", "long"])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--loop", action="store_true")
    ap.add_argument("--ratio", action="store_true")
    ap.add_argument("--launches", type=int, default=0)
    ap.add_argument("--entry", default="batch", choices=["batch", "ragged"])
    ap.add_argument("--sub-mean", type=int, default=0)
    args = ap.parse_args()
    if args.launches:
        return launches(args.launches, args.entry, args.sub_mean)
    if args.ratio:
        return ratio()
    for c in args.case or ["short", "ragged", "long"]:
        if c == "short":
            for sub_mean in (0, 1):
                case("4096 x 1 s at 48 kHz", 4096, 48000, 48000, sub_mean, args.reps, ("batch",), args.loop)
        elif c == "ragged":
            case("4096 x 0.5-1.5 s at 48 kHz", 4096, 24000, 72000, 0, args.reps, ("ragged",), args.loop)
        else:
            case("256 x 10 min at 12 kHz", 256, 7200000, 7200000, 0, args.reps, ("batch", "ragged"), args.loop)


if __name__ == "__main__":
    main()
