"""Complex I/Q rows: what run_iq / run_iq_batch cost on one MI355X.
    python tools/iq_rate.py --step rows --case fft4096|mtm4096|fft1024
        frames/s of run_iq on a device-resident stream of 2^29 complex f32 samples, beside
          compose  the same rows on the same GPU from torch: frames cut with unfold, times the table, torch.fft.fft, abs()**2, the
                   taper sum (in chunks of frames, so that its temporaries fit; the frames that reach back before sample 0 are left
                   out of it -- it has no zero history -- and its rate is over the frames it did)
          real     this library's real-input entry (run) at the same N and overlap on 2^29 real f32 samples: half the bytes, the
                   same number of frames -- what complex input costs
        and the algorithmic HBM bytes of the I/Q rows, 8 H + 4 N per frame, over 8 TB/s against the measured time.
        fft4096: N = 4096 Hanning, 75 % overlap;  mtm4096: N = 4096, 5 tapers (NW 2.5), overlap 0;  fft1024: N = 1024 Hanning, 50 %.
    python tools/iq_rate.py --step batch
        4096 streams of one second at 48 kHz (N = 1024 Hanning, 50 %): run_iq_batch against the loop of run_iq.
Events on the launch stream, --reps alternating repetitions in ONE process, median (min max).  Each step is a process of its own,
meant to run under its own time limit."""
import argparse
import sys

sys.path.insert(0, ".")
import torch
import glfer_amd as G

HBM_BYTES_PER_S = 8.0e12
CASES = {
    "fft4096": lambda: G.FftParams(n=4096, window_type=G.WINDOWS["hanning"], overlap=0.75),
    "mtm4096": lambda: G.MtmParams(n=4096, overlap=0.0, w=2.5, kmax=4),
    "fft1024": lambda: G.FftParams(n=1024, window_type=G.WINDOWS["hanning"], overlap=0.5),
}


def once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3


def med(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2], ts[0], ts[-1]


def alternate(fns, reps):
    """every fn once as warm-up, then reps rounds of all of them in turn"""
    for _, fn in fns:
        fn()
    torch.cuda.synchronize()
    ts = {name: [] for name, _ in fns}
    for _ in range(reps):
        for name, fn in fns:
            ts[name].append(once(fn))
    return {name: med(v) for name, v in ts.items()}


def rows(case, reps, log2_samples):
    params = CASES[case]()
    n = params.n
    sp = G.Spectrogram(params)
    hop, ntap = sp.hop, sp.ntapers
    S = 1 << log2_samples
    g = torch.Generator(device="cuda").manual_seed(1)
    z = torch.view_as_complex((torch.rand((S, 2), device="cuda", generator=g) - 0.5).contiguous())
    x = torch.rand(S, device="cuda", generator=g) - 0.5
    frames = sp.num_frames(S)
    out = torch.empty((frames, n), dtype=torch.float32, device="cuda")
    out_real = torch.empty((frames, sp.pitch), dtype=torch.float32, device="cuda")
    table = torch.from_numpy(G.iq_tables(params)).cuda()                  # [ntap][n], the scale folded in
    first_inside = -(-(n - hop) // hop)
    chunk = 8192

    def compose():
        for a in range(first_inside, frames, chunk):
            b = min(a + chunk, frames)
            fr = z[a * hop - (n - hop):(b - 1) * hop + hop].unfold(0, n, hop)
            acc = None
            for j in range(ntap):
                p = torch.fft.fft(fr * table[j]).abs() ** 2
                acc = p if acc is None else acc + p
            out[a:b] = acc

    # the composition's rows are the library's, to float32 rounding, on the frames it does
    sp.run_iq(z, out=out)
    mine = out[first_inside:first_inside + 64].clone()
    compose()
    torch.cuda.synchronize()
    theirs = out[first_inside:first_inside + 64]
    rel = float(((mine - theirs).abs().max() / mine.abs().max()).item())
    assert rel < 1e-4, rel

    res = alternate([("run_iq", lambda: sp.run_iq(z, out=out)), ("compose", compose), ("real", lambda: sp.run(x, out=out_real))], reps)
    by = 8 * hop + 4 * n
    print("## %s: N = %d, hop %d, %d taper(s), 2^%d complex f32 samples, %d frames (compose: %d)" % (
        case, n, hop, ntap, log2_samples, frames, frames - first_inside))
    for name, nf in (("run_iq", frames), ("compose", frames - first_inside), ("real", frames)):
        m, lo, hi = res[name]
        print("%-8s %9.3f ms (%.3f %.3f)  %8.3f M frames/s" % (name, m * 1e3, lo * 1e3, hi * 1e3, nf / m * 1e-6))
    m = res["run_iq"][0]
    print("run_iq against compose: %.2fx the frames/s; against the real-input entry: %.2fx its time" % (
        (frames / m) / ((frames - first_inside) / res["compose"][0]), m / res["real"][0]))
    floor = frames * by / HBM_BYTES_PER_S
    print("algorithmic bytes %d per frame (8 H + 4 N): %.3f GB, %.3f ms at 8 TB/s = %.1f %% of the measured time; %.2f TB/s achieved" % (
        by, frames * by * 1e-9, floor * 1e3, 100.0 * floor / m, frames * by / m * 1e-12))
    print("transforms: %.2f M N-point complex transforms/s" % (frames * ntap / m * 1e-6))
    print("max |run_iq - compose| / max over 64 rows: %.2e" % rel)
    sp.close()


def batch(reps):
    params = CASES["fft1024"]()
    sp = G.Spectrogram(params)
    B, S = 4096, 48000
    g = torch.Generator(device="cuda").manual_seed(2)
    z = torch.view_as_complex((torch.rand((B, S, 2), device="cuda", generator=g) - 0.5).contiguous())
    frames = sp.num_frames(S)
    out = torch.empty((B, frames, params.n), dtype=torch.float32, device="cuda")

    def loop():
        for b in range(B):
            sp.run_iq(z[b], out=out[b])

    sp.run_iq_batch(z, out=out)
    ref = out.clone()
    loop()
    torch.cuda.synchronize()
    assert torch.equal(ref.view(torch.int32), out.view(torch.int32))
    res = alternate([("batch", lambda: sp.run_iq_batch(z, out=out)), ("loop", loop)], reps)
    print("## batch: %d streams of %d complex f32 samples (one second at 48 kHz), N = 1024 Hanning, 50 %%: %d frames a stream" % (B, S, frames))
    for name in ("batch", "loop"):
        m, lo, hi = res[name]
        print("%-8s %9.3f ms (%.3f %.3f)  %8.3f M frames/s" % (name, m * 1e3, lo * 1e3, hi * 1e3, B * frames / m * 1e-6))
    print("run_iq_batch against the loop of run_iq: %.1fx (rows equal bit for bit)" % (res["loop"][0] / res["batch"][0]))
    sp.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=["rows", "batch"], required=True)
    ap.add_argument("--case", choices=sorted(CASES), default="fft4096")
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--log2-samples", type=int, default=29)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    if a.step == "rows":
        rows(a.case, a.reps, a.log2_samples)
    else:
        batch(a.reps)
