"""One ragged F call (Spectrogram.ftest_ragged / rows_ftest_ragged) against what a caller with streams of unequal length had
before: a loop of single-stream calls (ftest / rows_ftest), and one ftest_batch / rows_ftest_batch over the streams
zero-padded to the longest, with the copies into the padded buffer counted and without.  Device-resident f32 streams, events on
the launch stream, --reps alternating repetitions, medians and ranges (the method of tools/ragged_rate.py).
    python tools/ragged_ftest_rate.py [--case short|long ...] [--reps 6]
  short  4 096 streams of 0.5 .. 1.5 s at 48 kHz (uniform, fixed seed)
  long   256 streams of 5 .. 15 min at 12 kHz (against the loop only)
  each for N = 4096 with 5 tapers and N = 1024 with 8 tapers, with and without sub_mean = 1, F alone and rows-and-F
    python tools/ragged_ftest_rate.py --unchanged    the entries this work leaves alone: single-stream ftest and ftest_batch
                                                      (run in alternating processes, GLFER_LIB_PATH at another build)
    python tools/ragged_ftest_rate.py --launches B [--plan NAME] [--rows]
                                                      one ragged F call of B streams and nothing else (under rocprofv3 --kernel-trace)"""
import argparse
import sys

sys.path.insert(0, ".")
import numpy as np
import torch
import glfer_amd as G

PLANS = {
    "N=4096 T=5": dict(n=4096, overlap=0.0, w=2.5, kmax=4),
    "N=4096 T=5 sub_mean 1": dict(n=4096, overlap=0.0, w=2.5, kmax=4, sub_mean=1),
    "N=1024 T=8": dict(n=1024, overlap=0.0, w=4.0, kmax=7),
    "N=1024 T=8 sub_mean 1": dict(n=1024, overlap=0.0, w=4.0, kmax=7, sub_mean=1),
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


def bits(t):
    return t.view(torch.int32)


def ragged_case(title, plan, rows, lens, reps, padded):
    sp = G.Spectrogram(G.MtmParams(**PLANS[plan]))
    offs = np.concatenate([[0], np.cumsum(lens + (lens & 1))])[:-1]
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randn(int(offs[-1] + lens[-1] + 1), device="cuda", generator=g) * 0.2
    nb, longest = len(lens), int(lens.max())
    total, starts = sp.ragged_frames(lens)
    ft = torch.empty((total, sp.bins), device="cuda")
    psd = torch.empty((total, sp.pitch), device="cuda") if rows else None
    views = [x[int(o):int(o + n)] for o, n in zip(offs, lens)]
    span = [(int(starts[b]), int(starts[b + 1])) for b in range(nb)]

    if rows:
        def ragged():
            sp.rows_ftest_ragged(x, offs, lens, out=(psd, ft))

        def loop():
            for v, (r0, r1) in zip(views, span):
                if r1 > r0:
                    sp.rows_ftest(v, out=(psd[r0:r1], ft[r0:r1]))
    else:
        def ragged():
            sp.ftest_ragged(x, offs, lens, out=ft)

        def loop():                                          # (ftest allocates its rows, as a caller's loop does)
            for v, (r0, r1) in zip(views, span):
                if r1 > r0:
                    ft[r0:r1] = sp.ftest(v)

    ragged()
    torch.cuda.synchronize()
    ref = (ft.clone(), psd.clone() if rows else None)
    loop()
    torch.cuda.synchronize()
    assert torch.equal(bits(ft), bits(ref[0])), "ragged F rows differ from the loop's"
    assert not rows or torch.equal(bits(psd), bits(ref[1])), "ragged PSD rows differ from the loop's"
    del ref
    fns = [("ragged", ragged), ("loop of %d calls" % nb, loop)]
    if padded:
        nfp = sp.num_frames(longest)
        pad = torch.empty((nb, longest + (longest & 1)), device="cuda")
        pft = torch.empty((nb, nfp, sp.bins), device="cuda")
        ppsd = torch.empty((nb, nfp, sp.pitch), device="cuda") if rows else None

        def batch():
            if rows:
                sp.rows_ftest_batch(pad[:, :longest], out=(ppsd, pft))
            else:
                sp.ftest_batch(pad[:, :longest], out=pft)

        def padded_batch():                                  # zero, copy every stream in, one batch call
            pad.zero_()
            for b, v in enumerate(views):
                pad[b, :v.numel()] = v
            batch()

        padded_batch()
        torch.cuda.synchronize()
        fns.append(("padded batch, %d copies counted (%d of %d frames are padding)" % (nb, nb * nfp - total, nb * nfp), padded_batch))
        fns.append(("padded batch, the call alone", batch))
    ts = {name: [] for name, _ in fns}
    for _ in range(reps):                                    # alternating, so that no side gets the machine's better moments
        for name, fn in fns:
            ts[name].append(once(fn))
    tr = stats(ts["ragged"])
    print("%s, %s, %s: streams %d frames %d" % (title, plan, "rows_ftest_ragged" if rows else "ftest_ragged", nb, total))
    print("    %s %8.2f M frames/s" % (show("ragged", tr), total / tr[0] / 1e3))
    for name, _ in fns[1:]:
        t = stats(ts[name])
        print("    %s  x%.2f" % (show(name, t), t[0] / tr[0]))
    sys.stdout.flush()
    sp.close()
    del x, ft, psd, views
    torch.cuda.empty_cache()


def unchanged(reps):
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randn(4096 * 72000, device="cuda", generator=g) * 0.2
    xb = x.view(4096, 72000)
    for plan in PLANS:
        sp = G.Spectrogram(G.MtmParams(**PLANS[plan]))
        nf = sp.num_frames(x.numel())
        sp.ftest(x)
        torch.cuda.synchronize()
        t = stats([once(lambda: sp.ftest(x)) for _ in range(reps)])
        print("unchanged  ftest, one stream of 4096 x 72000, %-22s %s  %8.2f M frames/s" % (plan, show("", t), nf / t[0] / 1e3), flush=True)
        out = torch.empty((4096, sp.num_frames(72000), sp.bins), device="cuda")
        sp.ftest_batch(xb, out=out)
        torch.cuda.synchronize()
        t = stats([once(lambda: sp.ftest_batch(xb, out=out)) for _ in range(reps)])
        print("unchanged  ftest_batch 4096 x 72000,             %-22s %s  %8.2f M frames/s" % (plan, show("", t), out.size(0) * out.size(1) / t[0] / 1e3), flush=True)
        sp.close()
        del out
        torch.cuda.empty_cache()


def launches(nb, plan, rows):
    sp = G.Spectrogram(G.MtmParams(**PLANS[plan]))
    lens = np.random.RandomState(1).randint(24000, 72001, nb)
    offs = np.concatenate([[0], np.cumsum(lens)])[:-1]
    x = torch.zeros(int(lens.sum()), device="cuda")
    (sp.rows_ftest_ragged if rows else sp.ftest_ragged)(x, offs, lens)
    torch.cuda.synchronize()
    print("one %s call, %s, %d streams" % ("rows_ftest_ragged" if rows else "ftest_ragged", plan, nb))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", action="append", choices=["short", "long"])
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--unchanged", action="store_true")
    ap.add_argument("--launches", type=int, default=0)
    ap.add_argument("--plan", default="N=4096 T=5 sub_mean 1", choices=sorted(PLANS))
    ap.add_argument("--rows", action="store_true")
    args = ap.parse_args()
    if args.launches:
        return launches(args.launches, args.plan, args.rows)
    if args.unchanged:
        return unchanged(args.reps)
    for case in args.case or ["short", "long"]:
        for plan in PLANS:
            for rows in (False, True):
                if case == "short":
                    lens = np.random.RandomState(1).randint(24000, 72001, 4096)
                    ragged_case("4096 x 0.5-1.5 s at 48 kHz", plan, rows, lens, args.reps, True)
                else:
                    lens = np.random.RandomState(2).randint(5 * 60 * 12000, 15 * 60 * 12000 + 1, 256)
                    ragged_case("256 x 5-15 min at 12 kHz", plan, rows, lens, args.reps, False)


if __name__ == "__main__":
    main()
