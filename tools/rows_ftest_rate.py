"""The multitaper rows and F rows from one pass over the samples (Spectrogram.rows_ftest, glfer_hip_mtm_rows_ftest_device)
against the two calls it replaces (Spectrogram.run followed by Spectrogram.ftest), the F entry alone under two builds, and the
batch form against a loop of single calls.  GPU time from events around --iters calls queued back to back (a window of a
single call is a millisecond or two: too short to time).
    python tools/rows_ftest_rate.py --single [--reps 5] [--iters 40]
  one process, one library (GLFER_LIB_PATH selects it; a library without the new entries prints the first two lines only):
  per plan, on one stream of 2^28 f32 samples, the median / min / max over --reps windows of
      ftest       Spectrogram.ftest alone
      run+ftest   Spectrogram.run then Spectrogram.ftest
      rows_ftest  Spectrogram.rows_ftest alone
    python tools/rows_ftest_rate.py --ab PARENT_LIB [--pairs 6]
  --single in fresh child processes, the parent's library and this tree's alternating over --pairs pairs; prints every child's
  lines and, per plan and line, the range of the medians on each side
    python tools/rows_ftest_rate.py --batch [--case KEY ...] [--reps 5]
  the batch form against a loop of rows_ftest calls on the same streams (interleaved; bits compared first)
  shapes   s: 4 096 streams x 48 000 f32 samples (one second at 48 kHz)      l: 256 streams x 28 800 000 (ten minutes at 48 kHz)
  plans    4096: MTM N=4096, 5 tapers (NW 2.5), overlap 0                    1024: MTM N=1024, 8 tapers (NW 4), overlap 0"""
import argparse
import os
import re
import subprocess
import sys

sys.path.insert(0, ".")

SHAPES = {"s": (4096, 48000), "l": (256, 28800000)}
PLANS = {"4096": ("MTM N=4096, 5 tapers", dict(n=4096, overlap=0.0, w=2.5, kmax=4)),
         "1024": ("MTM N=1024, 8 tapers", dict(n=1024, overlap=0.0, w=4.0, kmax=7))}
KEYS = [s + p for s in "sl" for p in ("4096", "1024")]


def once(torch, fn, iters=1):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def stats(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2], ts[0], ts[-1]


def single(args):
    import torch
    import glfer_amd as G
    which = os.environ.get("GLFER_LIB_PATH") or "this tree"
    for key in ("4096", "1024"):
        name, kw = PLANS[key]
        sp = G.Spectrogram(G.MtmParams(**kw))
        x = torch.randn(1 << 28, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1)) * 0.2
        nf = sp.num_frames(x.numel())
        psd = torch.empty((nf, sp.pitch), device="cuda")
        ft = torch.empty((nf, sp.bins), device="cuda")
        forms = [("ftest", lambda: sp.ftest(x)), ("run+ftest", lambda: (sp.run(x, out=psd), sp.ftest(x)))]
        if hasattr(G.api.lib(), "glfer_hip_mtm_rows_ftest_device"):
            forms.append(("rows_ftest", lambda: sp.rows_ftest(x, out=(psd, ft))))
        for _, fn in forms:                              # warm up every form
            fn()
        torch.cuda.synchronize()
        ts = {nm: [] for nm, _ in forms}
        for _ in range(args.reps):                       # the forms interleaved, window by window
            for nm, fn in forms:
                ts[nm].append(once(torch, fn, args.iters))
        for nm, _ in forms:
            t = stats(ts[nm])
            print("single %-22s %-10s frames %8d  %8.3f ms (min %.3f max %.3f)  %7.2f M frames/s  %s" % (
                name, nm, nf, t[0], t[1], t[2], nf / t[0] / 1e3, which), flush=True)
        del x, psd, ft
        sp.close()
        torch.cuda.empty_cache()


def ab(args):
    line = re.compile(r"^single (.{22}) (\S+)\s+frames\s+\d+\s+([\d.]+) ms .*?([\d.]+) M frames/s")
    got = {}
    for i in range(args.pairs):
        for side, path in (("parent", args.ab), ("new", None)):
            env = dict(os.environ)
            env.pop("GLFER_LIB_PATH", None)
            if path:
                env["GLFER_LIB_PATH"] = os.path.abspath(path)
            r = subprocess.run([sys.executable, __file__, "--single", "--reps", str(args.reps), "--iters", str(args.iters)],
                               env=env, capture_output=True, text=True, timeout=600)
            if r.returncode != 0:                        # (a failed child ends the comparison: nothing more is started)
                sys.exit("pair %d %s: exit %d\n%s" % (i, side, r.returncode, r.stderr[-2000:]))
            for ln in r.stdout.splitlines():
                m = line.match(ln)
                if m:
                    print("pair %d %-6s %s" % (i, side, ln), flush=True)
                    got.setdefault((m.group(1).strip(), m.group(2), side), []).append(float(m.group(4)))
    print()
    for (plan, form, side), v in sorted(got.items()):
        print("range %-22s %-10s %-6s %7.2f .. %7.2f M frames/s over %d runs" % (plan, form, side, min(v), max(v), len(v)))


def batch(args):
    import torch
    import glfer_amd as G
    for key in args.case or KEYS:
        nb, nsamples = SHAPES[key[0]]
        pname, kw = PLANS[key[1:5]]
        name = "%s, B=%d x %d" % (pname, nb, nsamples)
        sp = G.Spectrogram(G.MtmParams(**kw))
        g = torch.Generator(device="cuda").manual_seed(1)
        x = torch.empty((nb, nsamples), device="cuda")
        for b in range(nb):                              # (stream by stream: no second copy of a 29 GB batch)
            x[b].normal_(0.1 * (2.0 * b / max(nb - 1, 1) - 1.0), 0.2, generator=g)
        nf = sp.num_frames(nsamples)
        out = (torch.empty((nb, nf, sp.pitch), device="cuda"), torch.empty((nb, nf, sp.bins), device="cuda"))
        lout = (torch.empty((nf, sp.pitch), device="cuda"), torch.empty((nf, sp.bins), device="cuda"))

        def one_batch():
            sp.rows_ftest_batch(x, out=out)

        def loop():
            for b in range(nb):
                sp.rows_ftest(x[b], out=lout)

        one_batch()
        torch.cuda.synchronize()
        for b in (0, nb // 2, nb - 1):
            sp.rows_ftest(x[b], out=lout)
            for o, w in zip(out, lout):
                assert torch.equal(o[b].view(torch.int32), w.view(torch.int32)), "batch rows differ from the loop's"
        tbs, tls = [], []
        for _ in range(args.reps):                       # interleaved, so that neither side gets the box's better moments
            tbs.append(once(torch, one_batch))
            tls.append(once(torch, loop))
        tb, tl = stats(tbs), stats(tls)
        print("%-44s frames %8d  batch %9.3f ms (min %.3f max %.3f) %7.2f M frames/s  |  loop of %d calls %9.3f ms (min %.3f max %.3f)  x%.2f" % (
            name, nb * nf, tb[0], tb[1], tb[2], nb * nf / tb[0] / 1e3, nb, tl[0], tl[1], tl[2], tl[0] / tb[0]), flush=True)
        del x, out, lout
        sp.close()
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--single", action="store_true")
    ap.add_argument("--ab", metavar="PARENT_LIB")
    ap.add_argument("--pairs", type=int, default=6)
    ap.add_argument("--batch", action="store_true")
    ap.add_argument("--case", action="append", choices=KEYS)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=40)
    args = ap.parse_args()
    if args.ab:
        return ab(args)
    if args.batch:
        return batch(args)
    return single(args)


if __name__ == "__main__":
    main()
