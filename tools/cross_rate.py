"""Two channels' cross-spectrum and coherence: what Spectrogram.cross / cross_batch cost on one MI355X.
    python tools/cross_rate.py --step rows --case mtm4096|mtm4096o75|mtm1024
        frames/s of cross on a device-resident stream of 2^28 pairs of f32, all four outputs and coh alone, beside
          run_iq    the complex I/Q rows on the same bytes: the same transforms without the exchange through the mirror bins and with
                    one sum instead of four -- the price of the separation (it writes N bins a frame, cross 5 (N/2 + 1) floats)
          channels  run_channels with the same plan: the two power rows, no Sxy (a de-interleave, then the real-input kernels)
          compose   the same four outputs on the same GPU from torch: frames cut with unfold, float32 tapers, torch.fft.rfft, the
                    weighted einsum, the quotient (in chunks of frames; the frames that reach back before sample 0 are left out of
                    it and its rate is over the frames it did)
        mtm4096: N = 4096, 5 tapers (NW 2.5), overlap 0;  mtm4096o75: the same at 75 %;  mtm1024: N = 1024, 8 tapers (NW 4), 50 %.
    python tools/cross_rate.py --step batch
        4096 stereo streams of one second at 48 kHz (N = 1024, 8 tapers, 50 %): cross_batch against the loop of cross.
Events on the launch stream, --reps alternating repetitions in ONE process, median (min max).  Each step is a process of its own,
meant to run under its own time limit."""
import argparse
import sys

sys.path.insert(0, ".")
import torch
import glfer_amd as G

ALL = ("sxx", "syy", "sxy", "coh")
CASES = {
    "mtm4096": lambda: G.MtmParams(n=4096, overlap=0.0, w=2.5, kmax=4),
    "mtm4096o75": lambda: G.MtmParams(n=4096, overlap=0.75, w=2.5, kmax=4),
    "mtm1024": lambda: G.MtmParams(n=1024, overlap=0.5, w=4.0, kmax=7),
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


def rows(case, reps, log2_pairs):
    params = CASES[case]()
    n, bins = params.n, params.n // 2 + 1
    sp = G.Spectrogram(params)
    hop, ntap = sp.hop, sp.ntapers
    S = 1 << log2_pairs
    g = torch.Generator(device="cuda").manual_seed(1)
    xy = (torch.rand((S, 2), device="cuda", generator=g) - 0.5).contiguous()
    xy[:, 1] += 0.5 * xy[:, 0]                                              # partly coherent channels
    frames = sp.num_frames(S)
    outs = {k: torch.empty((frames, bins), dtype=torch.complex64 if k == "sxy" else torch.float32, device="cuda") for k in ALL}
    out_iq = torch.empty((frames, n), dtype=torch.float32, device="cuda")
    out_ch = torch.empty((2, frames, sp.pitch), dtype=torch.float32, device="cuda")
    tapers, sig = sp.tapers()
    v = torch.from_numpy(tapers).to(torch.float32).cuda()                   # [ntap][n]
    cj = torch.from_numpy(1.0 / (n * (1.0 + sig))).to(torch.float32).cuda()
    first_inside = -(-(n - hop) // hop)
    chunk = 8192
    comp = {k: torch.empty_like(t) for k, t in outs.items()}

    def compose():
        for a in range(first_inside, frames, chunk):
            b = min(a + chunk, frames)
            fr = xy[a * hop - (n - hop):(b - 1) * hop + hop].unfold(0, n, hop)          # [frames][2][n]
            X = torch.fft.rfft(fr[:, 0, None, :] * v)                                   # [frames][ntap][bins]
            Y = torch.fft.rfft(fr[:, 1, None, :] * v)
            sxx = torch.einsum("j,fjk->fk", cj, X.real ** 2 + X.imag ** 2)
            syy = torch.einsum("j,fjk->fk", cj, Y.real ** 2 + Y.imag ** 2)
            sxy = torch.einsum("j,fjk->fk", cj.to(torch.complex64), X * Y.conj())
            comp["sxx"][a:b], comp["syy"][a:b], comp["sxy"][a:b] = sxx, syy, sxy
            comp["coh"][a:b] = (sxy.real ** 2 + sxy.imag ** 2) / (sxx * syy)

    # the composition's rows are the library's, to float32 rounding, on the frames it does
    sp.cross(xy, want=ALL, out=outs)
    compose()
    torch.cuda.synchronize()
    sl = slice(first_inside, first_inside + 64)
    rel = max(float(((outs[k][sl] - comp[k][sl]).abs().max() / outs[k][sl].abs().max()).item()) for k in ALL)
    assert rel < 1e-3, rel

    res = alternate([("cross", lambda: sp.cross(xy, want=ALL, out=outs)),
                     ("coh", lambda: sp.cross(xy, want=("coh",), out={"coh": outs["coh"]})),
                     ("run_iq", lambda: sp.run_iq(xy, out=out_iq)),
                     ("channels", lambda: sp.run_channels(xy, out=out_ch)),
                     ("compose", compose)], reps)
    print("## %s: N = %d, hop %d, %d tapers, 2^%d pairs of f32, %d frames (compose: %d)" % (
        case, n, hop, ntap, log2_pairs, frames, frames - first_inside))
    for name in ("cross", "coh", "run_iq", "channels", "compose"):
        m, lo, hi = res[name]
        nf = frames - first_inside if name == "compose" else frames
        print("%-8s %9.3f ms (%.3f %.3f)  %8.3f M frames/s" % (name, m * 1e3, lo * 1e3, hi * 1e3, nf / m * 1e-6))
    m = res["cross"][0]
    print("cross against run_iq (the price of the separation): %.2fx its time; coh alone: %.2fx; against run_channels: %.2fx its time; "
          "against compose: %.2fx the frames/s" % (m / res["run_iq"][0], res["coh"][0] / res["run_iq"][0], m / res["channels"][0],
                                                 (frames / m) / ((frames - first_inside) / res["compose"][0])))
    by = 8 * hop + 20 * bins
    print("algorithmic bytes %d per frame (8 H + 20 (N/2 + 1), all four outputs): %.3f GB, %.2f TB/s achieved" % (
        by, frames * by * 1e-9, frames * by / m * 1e-12))
    print("transforms: %.2f M N-point complex transforms/s" % (frames * ntap / m * 1e-6))
    print("max |cross - compose| / max over 64 rows, the four outputs: %.2e" % rel)
    sp.close()


def batch(reps):
    params = CASES["mtm1024"]()
    sp = G.Spectrogram(params)
    B, S = 4096, 48000
    g = torch.Generator(device="cuda").manual_seed(2)
    xy = (torch.rand((B, S, 2), device="cuda", generator=g) - 0.5).contiguous()
    frames, bins = sp.num_frames(S), params.n // 2 + 1
    outs = {k: torch.empty((B, frames, bins), dtype=torch.complex64 if k == "sxy" else torch.float32, device="cuda") for k in ALL}

    def loop():
        for b in range(B):
            sp.cross(xy[b], want=ALL, out={k: t[b] for k, t in outs.items()})

    sp.cross_batch(xy, want=ALL, out=outs)
    ref = {k: t.clone() for k, t in outs.items()}
    loop()
    torch.cuda.synchronize()
    for k in ALL:
        a, b = (torch.view_as_real(t) if t.is_complex() else t for t in (ref[k], outs[k]))
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), k
    res = alternate([("batch", lambda: sp.cross_batch(xy, want=ALL, out=outs)), ("loop", loop)], reps)
    print("## batch: %d stereo streams of %d pairs of f32 (one second at 48 kHz), N = 1024, 8 tapers, 50 %%: %d frames a stream" % (B, S, frames))
    for name in ("batch", "loop"):
        m, lo, hi = res[name]
        print("%-8s %9.3f ms (%.3f %.3f)  %8.3f M frames/s" % (name, m * 1e3, lo * 1e3, hi * 1e3, B * frames / m * 1e-6))
    print("cross_batch against the loop of cross: %.1fx (the four outputs equal bit for bit)" % (res["loop"][0] / res["batch"][0]))
    sp.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=["rows", "batch"], required=True)
    ap.add_argument("--case", choices=sorted(CASES), default="mtm4096")
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--log2-pairs", type=int, default=28)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    if a.step == "rows":
        rows(a.case, a.reps, a.log2_pairs)
    else:
        batch(a.reps)
