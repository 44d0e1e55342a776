"""One ragged call (Spectrogram.run_ragged, glfer_hip_spectrogram_ragged_device) against what a caller with streams of
unequal length had before: a loop of single-stream calls (Spectrogram.run), and one run_batch over the streams zero-padded to
the longest, the copy into the padded buffer counted.  Device-resident streams, events on the launch stream, --reps
alternating repetitions, medians and ranges (the method of tools/batch_rate.py).
    python tools/ragged_rate.py [--case short|long|equal ...] [--reps 6]
  short  4 096 streams of 0.5 .. 1.5 s at 48 kHz (uniform, fixed seed): C2, C2 with sub_mean 1, C3
  long   256 streams of 5 .. 15 min at 12 kHz: C3 (against the loop only)
  equal  4 096 streams of 48 000 samples: run_ragged against run_batch -- what the table costs
    python tools/ragged_rate.py --unchanged      the routes this work leaves alone (run twice, GLFER_LIB_PATH at another build)
    python tools/ragged_rate.py --launches B     one ragged call of B streams and nothing else (under rocprofv3 --kernel-trace)"""
import argparse
import sys

sys.path.insert(0, ".")
import numpy as np
import torch
import glfer_amd as G

PLANS = {
    "C2": (G.FftParams, dict(n=4096, window_type=0, overlap=0.75)),
    "C2 sub_mean 1": (G.FftParams, dict(n=4096, window_type=0, overlap=0.75, sub_mean=1)),
    "C3": (G.MtmParams, dict(n=4096, overlap=0.0, w=2.5, kmax=4)),
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


def show(name, t):
    return "%s %9.3f ms (min %.3f max %.3f)" % (name, t[0], t[1], t[2])


def collection(lens, seed=1):
    """the streams back to back in one buffer (even offsets), a DC level per stream"""
    offs = np.concatenate([[0], np.cumsum(lens + (lens & 1))])[:-1]
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(int(offs[-1] + lens[-1] + 1), device="cuda", generator=g) * 0.2
    return x, offs


def ragged_case(title, plan, lens, reps, padded):
    P, kw = PLANS[plan]
    sp = G.Spectrogram(P(**kw))
    x, offs = collection(lens)
    nb, longest = len(lens), int(lens.max())
    total, starts = sp.ragged_frames(lens)
    out = torch.empty((total, sp.pitch), device="cuda")
    views = [x[int(o):int(o + n)] for o, n in zip(offs, lens)]
    rows = [out[int(starts[b]):int(starts[b + 1])] for b in range(nb)]

    def ragged():
        sp.run_ragged(x, offs, lens, out=out)

    def loop():
        for v, r in zip(views, rows):
            if r.size(0):
                sp.run(v, out=r)

    ragged()
    torch.cuda.synchronize()
    ref = out.clone()
    loop()
    torch.cuda.synchronize()
    assert torch.equal(out, ref), "ragged rows differ from the loop's"
    del ref
    fns = [("ragged", ragged), ("loop of %d calls" % nb, loop)]
    if padded:
        nfp = sp.num_frames(longest)
        pad = torch.empty((nb, longest + (longest & 1)), device="cuda")
        pout = torch.empty((nb, nfp, sp.pitch), device="cuda")

        def padded_batch():                                  # what the caller does today: zero, copy every stream in, one batch call
            pad.zero_()
            for b, v in enumerate(views):
                pad[b, :v.numel()] = v
            sp.run_batch(pad[:, :longest], out=pout)

        padded_batch()
        torch.cuda.synchronize()
        fns.append(("padded run_batch (%d of %d frames are padding)" % (nb * nfp - total, nb * nfp), padded_batch))
    ts = {name: [] for name, _ in fns}
    for _ in range(reps):                                    # alternating, so that no side gets the machine's better moments
        for name, fn in fns:
            ts[name].append(once(fn))
    tr = stats(ts["ragged"])
    line = "%-34s streams %5d frames %9d  %s %8.2f M frames/s" % (title + ", " + plan, nb, total, show("ragged", tr), total / tr[0] / 1e3)
    for name, _ in fns[1:]:
        t = stats(ts[name])
        line += "  |  %s  x%.2f" % (show(name, t), t[0] / tr[0])
    print(line, flush=True)
    sp.close()
    torch.cuda.empty_cache()


def equal_case(plan, reps, nb=4096, n=48000):
    P, kw = PLANS[plan]
    sp = G.Spectrogram(P(**kw))
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randn((nb, n), device="cuda", generator=g) * 0.2
    nf = sp.num_frames(n)
    out = torch.empty((nb, nf, sp.pitch), device="cuda")
    offs, lens = np.arange(nb) * n, np.full(nb, n)
    flat = x.view(-1)
    ragged = lambda: sp.run_ragged(flat, offs, lens, out=out.view(-1, sp.pitch))
    batch = lambda: sp.run_batch(x, out=out)
    batch()
    torch.cuda.synchronize()
    ref = out.clone()
    ragged()
    torch.cuda.synchronize()
    assert torch.equal(out, ref)
    tr, tb = [], []
    for _ in range(reps):
        tr.append(once(ragged))
        tb.append(once(batch))
    tr, tb = stats(tr), stats(tb)
    print("%-34s streams %5d frames %9d  %s  |  %s  ragged / batch x%.3f" % ("equal lengths, " + plan, nb, nb * nf, show("ragged", tr), show("run_batch", tb), tr[0] / tb[0]), flush=True)
    sp.close()
    torch.cuda.empty_cache()


def unchanged(reps):
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randn(4096 * 72000, device="cuda", generator=g) * 0.2
    for plan in ("C3", "C2"):
        P, kw = PLANS[plan]
        sp = G.Spectrogram(P(**kw))
        out = torch.empty((sp.num_frames(x.numel()), sp.pitch), device="cuda")
        sp.run(x, out=out)
        torch.cuda.synchronize()
        t = stats([once(lambda: sp.run(x, out=out)) for _ in range(reps)])
        print("unchanged  single stream 4096 x 72000, %-14s %s  %8.2f M frames/s" % (plan, show("run", t), out.size(0) / t[0] / 1e3), flush=True)
        sp.close()
        del out
    lens = np.random.RandomState(1).randint(24000, 72001, 4096)
    longest = int(lens.max())
    xb = x[:4096 * longest].view(4096, longest)
    for plan in ("C2", "C2 sub_mean 1", "C3"):
        P, kw = PLANS[plan]
        sp = G.Spectrogram(P(**kw))
        out = torch.empty((4096, sp.num_frames(longest), sp.pitch), device="cuda")
        sp.run_batch(xb, out=out)
        torch.cuda.synchronize()
        t = stats([once(lambda: sp.run_batch(xb, out=out)) for _ in range(reps)])
        print("unchanged  run_batch 4096 x %d, %-14s %s  %8.2f M frames/s" % (longest, plan, show("run_batch", t), out.size(0) * out.size(1) / t[0] / 1e3), flush=True)
        sp.close()
        del out


def launches(nb):
    P, kw = PLANS["C2 sub_mean 1"]
    sp = G.Spectrogram(P(**kw))
    lens = np.random.RandomState(1).randint(24000, 72001, nb)
    offs = np.concatenate([[0], np.cumsum(lens)])[:-1]
    x = torch.zeros(int(lens.sum()), device="cuda")
    sp.run_ragged(x, offs, lens)
    torch.cuda.synchronize()
    print("one ragged call, C2 sub_mean 1, %d streams" % nb)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", action="append", choices=["short", "long", "equal"])
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--unchanged", action="store_true")
    ap.add_argument("--launches", type=int, default=0)
    args = ap.parse_args()
    if args.launches:
        return launches(args.launches)
    if args.unchanged:
        return unchanged(args.reps)
    for case in args.case or ["short", "equal", "long"]:
        if case == "short":
            lens = np.random.RandomState(1).randint(24000, 72001, 4096)
            for plan in PLANS:
                ragged_case("4096 x 0.5-1.5 s at 48 kHz", plan, lens, args.reps, True)
        elif case == "equal":
            for plan in PLANS:
                equal_case(plan, args.reps)
        else:
            lens = np.random.RandomState(2).randint(5 * 60 * 12000, 15 * 60 * 12000 + 1, 256)
            ragged_case("256 x 5-15 min at 12 kHz", "C3", lens, args.reps, False)


if __name__ == "__main__":
    main()
