"""One batched waterfall call (waterfall_batch, glfer_hip_waterfall_batch_device) against B single-stream calls
(waterfall, glfer_hip_waterfall_device) on the same PSD rows: floor statistics, level tracking (log scale, autoscale), the
optional moving average and the pixel map, levbuf on.  GPU time per call sequence from device events around it (both
entries synchronise inside: the loop pays one synchronisation per stream); median, min and max of --reps, batch and loop
interleaved.  The outputs and carried states are checked equal first.
    python tools/waterfall_batch_rate.py [--case s0|s4|a0|a4|c0|c4 ...] [--reps 5] [--batch-only] [--streams B]
  s0 / s4  4 096 one-second C2-shaped streams (46 rows of 2 049 bins), no average / plain average depth 4
  a0 / a4  256 ten-minute streams (7 031 rows of 2 049 bins each), no average / plain average depth 4
  c0 / c4  B = 1: one ten-minute stream"""
import argparse
import sys

sys.path.insert(0, ".")
import torch
import glfer_amd as G

BINS = 2049
CASES = {
    "s0": ("B=4096 x 46 rows, no average", 4096, 46, 0),
    "s4": ("B=4096 x 46 rows, plain depth 4", 4096, 46, 4),
    "a0": ("B=256 x 7031 rows, no average", 256, 7031, 0),
    "a4": ("B=256 x 7031 rows, plain depth 4", 256, 7031, 4),
    "c0": ("B=1 x 7031 rows, no average", 1, 7031, 0),
    "c4": ("B=1 x 7031 rows, plain depth 4", 1, 7031, 4),
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


def displays(nb):
    out = []
    for b in range(nb):
        d = G.Display(scale_type=G.SCALE_LOG, autoscale=1, overlap=0.75, palette=0, first_buffer=1 if b % 2 == 0 else 0)
        d.display_max_lvl, d.display_min_lvl = 0.01 * (1 + b % 7), 1e-4 * (1 + b % 3)
        out.append(d)
    return out


def copies(ds):
    return [G.Display.from_buffer_copy(d) for d in ds]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", action="append", choices=sorted(CASES))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batch-only", action="store_true", help="time the batch call only (profiler runs)")
    ap.add_argument("--streams", type=int, default=0, help="B other than the case's own")
    args = ap.parse_args()
    for key in args.case or ["s0", "s4", "a0", "a4", "c0", "c4"]:
        name, nb, nf, depth = CASES[key]
        if args.streams:
            nb, name = args.streams, name.replace("B=%d" % nb, "B=%d" % args.streams)
        g = torch.Generator(device="cuda").manual_seed(1)
        psd = torch.rand((nb, nf, BINS), device="cuda", generator=g)
        psd = psd * psd * psd * psd * torch.logspace(-3, 1, nb, device="cuda")[:, None, None]
        av = dict(avg_mode=G.AVG_PLAIN, depth=depth, minbin=0, maxbin=BINS) if depth else dict(avg_mode=0)
        base = displays(nb)
        res = {}

        def batch():
            res["batch"] = G.waterfall_batch(copies(base), psd, **av)

        def loop():
            res["loop"] = [G.waterfall(d, psd[b], **av) for b, d in enumerate(copies(base))]

        batch()
        torch.cuda.synchronize()
        if args.batch_only:
            tb = stats([once(batch) for _ in range(args.reps)])
        else:
            bd, ld = copies(base), copies(base)
            rgb, lev, _ = G.waterfall_batch(bd, psd, **av)
            want = [G.waterfall(ld[b], psd[b], **av) for b in range(nb)]
            torch.cuda.synchronize()
            for b, (w_rgb, w_lev, _) in enumerate(want):
                assert torch.equal(rgb[b], w_rgb) and torch.equal(lev[b], w_lev), "batch stream %d differs from the loop's" % b
                assert (bd[b].first_buffer, bd[b].display_max_lvl, bd[b].display_min_lvl) == \
                       (ld[b].first_buffer, ld[b].display_max_lvl, ld[b].display_min_lvl), "state of stream %d" % b
            del rgb, lev, want
            res.clear()
            tbs, tls = [], []
            for _ in range(args.reps):                   # interleaved, so that neither side gets the box's better moments
                tbs.append(once(batch))
                res.clear()
                tls.append(once(loop))
                res.clear()
            tb, tl = stats(tbs), stats(tls)
        line = "%-34s columns %9d  batch %9.3f ms (min %.3f max %.3f)  %8.2f M columns/s" % (
            name, nb * nf, tb[0], tb[1], tb[2], nb * nf / tb[0] / 1e3)
        if not args.batch_only:
            line += "  |  loop of %d calls %9.3f ms (min %.3f max %.3f)  speed-up x%.2f" % (nb, tl[0], tl[1], tl[2], tl[0] / tb[0])
        print(line, flush=True)
        res.clear()
        del psd
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
