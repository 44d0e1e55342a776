"""Every launcher of glfer_hip.cpp on fixed inputs, one line per case with the SHA-256 of each output buffer: two builds of the
library compute the same thing exactly when their outputs of this tool are equal line for line, and launch the same thing
when the kernel traces of two runs are (rocprofv3 --kernel-trace -- python tools/launcher_identity.py).
    python tools/launcher_identity.py                        this tree's library
    GLFER_LIB_PATH=<other libglfer_hip.so> python tools/launcher_identity.py
The cases: the cut-edge calls of tests/test_gpu_frame_cuts.py (plans A .. D, sub_mean 0 / 1 / fast, rows and batch at every
(first, nframes), the ragged call, plan A's F entries), then one 4 096-frame call per plan through the rows, batch, ragged,
average, average-batch, F and F-batch entries.  Inputs come from fixed seeds on the host; nothing is timed."""
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import glfer_amd as G

# name: (kind, n, overlap, sample format, history_mode, G, first_inside)
PLANS = {
    "A": ("mtm", 1024, 0.5, 0, 0, 8, 1), "A_s16": ("mtm", 1024, 0.5, 1, 0, 8, 1),
    "B": ("mtm", 4096, 0.75, 0, 0, 2, 3),
    "C": ("fft", 1024, 0.75, 0, 0, 1, 3), "C_zero_always": ("fft", 1024, 0.75, 0, 1, 1, 3),
    "D": ("fft", 256, 0.5, 0, 0, 1, 1),
}
SUB_MEANS = (0, G.SUBMEAN_EXACT, G.SUBMEAN_FAST)


def sha(*tensors):
    torch.cuda.synchronize()
    return " ".join(hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()[:32] for t in tensors if t is not None)


def uniq(values):
    return [v for i, v in enumerate(values) if v not in values[:i]]


def calls(Gf, fi):
    return [(f, c) for f in uniq([0, 1, fi, Gf - 1, Gf, Gf + 1]) for c in uniq([1, Gf - 1, Gf, 2 * Gf + 1]) if c > 0]


def plan(name, sub):
    kind, n, overlap, fmt, hm, _, _ = PLANS[name]
    common = dict(n=n, overlap=overlap, sub_mean=sub, history_mode=hm, sample_format=fmt)
    return G.Spectrogram(G.MtmParams(w=2.5, kmax=4, **common) if kind == "mtm" else G.FftParams(window_type=0, **common))


def streams(nb, nsamples, fmt, seed):
    rng = np.random.default_rng(seed)
    x = 0.25 * rng.standard_normal((nb, nsamples)) + np.linspace(-0.1, 0.1, nb)[:, None]
    x = np.clip(np.round(x * 20000.0), -32768, 32767).astype(np.int16) if fmt == 1 else x.astype(np.float32)
    return torch.from_numpy(x).to("cuda")


def ragged(sp, x, frames, spare):
    """streams of these frame counts cut out of x's rows, back to back at even offsets in one buffer"""
    lens = [max(f * sp.hop + s, 0) for f, s in zip(frames, spare)]
    offs, at = [], 0
    for n in lens:
        offs.append(at)
        at += n + (n & 1)
    buf = torch.zeros(max(at, 1), dtype=x.dtype, device="cuda")
    for b, (o, n) in enumerate(zip(offs, lens)):
        buf[o:o + n] = x[b % x.size(0), 3 * b:3 * b + n]
    return sp.run_ragged(buf, offs, lens)[0]


def main():
    for name, (kind, n, overlap, fmt, hm, Gf, fi) in sorted(PLANS.items()):
        for sub in SUB_MEANS:
            sp = plan(name, sub)
            tag = "%s sub_mean %d" % (name, sub)
            x = streams(3, (48 * sp.hop + sp.hop // 3) & ~1, fmt, 11)
            for first, count in calls(Gf, fi):
                print("%s rows first %d nframes %d: %s" % (tag, first, count, sha(sp.run(x[1], first_frame=first, nframes=count))))
                print("%s batch first %d nframes %d: %s" % (tag, first, count, sha(sp.run_batch(x, first_frame=first, nframes=count))))
                if name == "A" and sub == G.SUBMEAN_EXACT:
                    print("%s F first %d nframes %d: %s" % (tag, first, count, sha(sp.ftest(x[1], first_frame=first, nframes=count))))
                    print("%s F-batch first %d nframes %d: %s" % (tag, first, count, sha(sp.ftest_batch(x, first_frame=first, nframes=count))))
            print("%s ragged: %s" % (tag, sha(ragged(sp, x, [0, fi, fi + Gf - 1, 2 * Gf + 3, 4 * Gf], [sp.hop - 1, 0, sp.hop // 2, 1, 0]))))
            # 4 096 frames a stream
            x = streams(3, 4096 * sp.hop + 2 * (sp.hop // 6), fmt, 12)
            print("%s rows 4096: %s" % (tag, sha(sp.run(x[2]))))
            print("%s batch 4096: %s" % (tag, sha(sp.run_batch(x))))
            print("%s ragged 4096: %s" % (tag, sha(ragged(sp, x, [4096, 1000, 4090], [0, 5, 0]))))
            for depth in (4, 7):                        # (the average inside the estimator launch takes depths up to 4)
                print("%s average depth %d 4096: %s" % (tag, depth, sha(*sp.run_avg(x[0], G.AVG_PLAIN, depth, 3, sp.bins - 5, want_psd=True))))
                print("%s average-batch depth %d 4096: %s" % (tag, depth, sha(*sp.run_avg_batch(x, G.AVG_PLAIN, depth, 3, sp.bins - 5, want_psd=True))))
            print("%s average no rows, first 37, 4096: %s" % (tag, sha(*sp.run_avg(x[0], G.AVG_PLAIN, 4, 0, sp.bins, first_frame=37))))
            print("%s average-batch no rows, first 37, 4096: %s" % (tag, sha(*sp.run_avg_batch(x, G.AVG_PLAIN, 4, 0, sp.bins, first_frame=37))))
            if kind == "mtm":
                print("%s F 4096: %s" % (tag, sha(sp.ftest(x[1]))))
                print("%s F-batch 4096: %s" % (tag, sha(sp.ftest_batch(x))))
                print("%s rows-and-F 4096: %s" % (tag, sha(*sp.rows_ftest(x[1]))))
                print("%s rows-and-F-batch 4096: %s" % (tag, sha(*sp.rows_ftest_batch(x))))
            sys.stdout.flush()
            sp.close()
            del x
    # the LMP statistic over rows with the mean removal in the kernel (glfer_run_device's second user of the driver)
    for sub in SUB_MEANS:
        sp = G.Spectrogram(G.LmpParams(n=1024, overlap=0.5, avg=4, sub_mean=sub))
        x = streams(1, 4096 * sp.hop, 0, 13)
        print("lmp sub_mean %d rows 4096: %s; first 5 nframes 9: %s" % (sub, sha(sp.run(x[0])), sha(sp.run(x[0], first_frame=5, nframes=9))))
        sp.close()


if __name__ == "__main__":
    main()
