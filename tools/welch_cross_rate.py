"""Welch cross-spectrum and coherence: what Spectrogram.cross_welch / cross_welch_batch cost on one MI355X.
    python tools/welch_cross_rate.py --step rows --case fft4096o75|fft1024o50|mtm4096L4
        transforms/s (frames x tapers) of cross_welch on a device-resident stream of 2^28 pairs of f32, all four outputs and coh alone,
        beside
          run_iq    the complex I/Q rows on the same bytes: the same transforms, one row per frame and no averaging
          compose   the same four outputs on the same GPU from torch: frames cut with unfold, the float32 window, torch.fft.rfft,
                    the segment means, the quotient (in chunks of frames; the rows whose frames reach back before sample 0 are left
                    out of it and its rate is over the frames it did)
        fft4096o75: Hanning, N = 4096, 75 % overlap, L = step = 16;  fft1024o50: Hanning, N = 1024, 50 %, L = step = 16;
        mtm4096L4: five tapers (NW 2.5), N = 4096, no overlap, L = step = 4 (beside cross on the same plan: L = 1).
    python tools/welch_cross_rate.py --step cross
        Spectrogram.cross alone (N = 4096, five tapers, no overlap, 2^28 pairs): one line, for runs of this step in alternating
        processes on two builds of the library (GLFER_LIB_PATH names the other one).
    python tools/welch_cross_rate.py --step batch
        4096 stereo streams of one second at 48 kHz (Hanning, N = 1024, 50 %, L = step = 16): cross_welch_batch against the loop.
Events on the launch stream, --reps alternating repetitions in ONE process, median (min max).  Each step is a process of its own,
meant to run under its own time limit."""
import argparse
import sys

sys.path.insert(0, ".")
import torch
import glfer_amd as G

ALL = ("sxx", "syy", "sxy", "coh")
CASES = {
    "fft4096o75": (lambda: G.FftParams(n=4096, window_type=G.WINDOWS["hanning"], overlap=0.75), 16),
    "fft1024o50": (lambda: G.FftParams(n=1024, window_type=G.WINDOWS["hanning"], overlap=0.5), 16),
    "mtm4096L4": (lambda: G.MtmParams(n=4096, overlap=0.0, w=2.5, kmax=4), 4),
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


def stream(log2_pairs, seed=1):
    g = torch.Generator(device="cuda").manual_seed(seed)
    xy = (torch.rand((1 << log2_pairs, 2), device="cuda", generator=g) - 0.5).contiguous()
    xy[:, 1] += 0.5 * xy[:, 0]                                              # partly coherent channels
    return xy


def rows(case, reps, log2_pairs):
    make, L = CASES[case]
    params = make()
    n, bins = params.n, params.n // 2 + 1
    sp = G.Spectrogram(params)
    hop, ntap = sp.hop, sp.ntapers
    xy = stream(log2_pairs)
    S = xy.size(0)
    frames = sp.num_frames(S)
    nrows = sp.welch_rows(S, L)
    used = nrows * L                                                        # frames the rows are made of
    outs = {k: torch.empty((nrows, bins), dtype=torch.complex64 if k == "sxy" else torch.float32, device="cuda") for k in ALL}
    out_iq = torch.empty((frames, n), dtype=torch.float32, device="cuda")
    fns = [("welch", lambda: sp.cross_welch(xy, L, want=ALL, out=outs)),
           ("coh", lambda: sp.cross_welch(xy, L, want=("coh",), out={"coh": outs["coh"]})),
           ("run_iq", lambda: sp.run_iq(xy, out=out_iq))]
    nfr = {"welch": used, "coh": used, "run_iq": frames}
    rel = None
    if params.mode == G.MODE_FFT:
        w = torch.from_numpy(sp.window()).cuda()
        row0 = -(-(-(-(n - hop) // hop)) // L)                              # the first row whose frames lie inside the stream
        chunk = 8192 // L * L
        comp = {k: torch.empty_like(t) for k, t in outs.items()}

        def compose():
            for a in range(row0 * L, used, chunk):
                b = min(a + chunk, used)
                fr = xy[a * hop - (n - hop):(b - 1) * hop + hop].unfold(0, n, hop)          # [frames][2][n]
                X = torch.fft.rfft(fr[:, 0, :] * w)
                Y = torch.fft.rfft(fr[:, 1, :] * w)
                sxx = ((X.real ** 2 + X.imag ** 2) / n).view(-1, L, bins).mean(1)
                syy = ((Y.real ** 2 + Y.imag ** 2) / n).view(-1, L, bins).mean(1)
                sxy = ((X * Y.conj()) / n).view(-1, L, bins).mean(1)
                r = slice(a // L, b // L)
                comp["sxx"][r], comp["syy"][r], comp["sxy"][r] = sxx, syy, sxy
                comp["coh"][r] = (sxy.real ** 2 + sxy.imag ** 2) / (sxx * syy)

        # the composition's rows are the library's, to float32 rounding, on the rows it does
        sp.cross_welch(xy, L, want=ALL, out=outs)
        compose()
        torch.cuda.synchronize()
        sl = slice(row0, row0 + 64)
        rel = max(float(((outs[k][sl] - comp[k][sl]).abs().max() / outs[k][sl].abs().max()).item()) for k in ALL)
        assert rel < 1e-3, rel
        fns.append(("compose", compose))
        nfr["compose"] = used - row0 * L
    else:
        per = {k: torch.empty((frames, bins), dtype=torch.complex64 if k == "sxy" else torch.float32, device="cuda") for k in ALL}
        fns.append(("cross", lambda: sp.cross(xy, want=ALL, out=per)))
        nfr["cross"] = frames
    res = alternate(fns, reps)
    print("## %s: N = %d, hop %d, %d taper%s, L = step = %d, 2^%d pairs of f32, %d frames, %d rows" % (
        case, n, hop, ntap, "" if ntap == 1 else "s", L, log2_pairs, frames, nrows))
    for name, _ in fns:
        m, lo, hi = res[name]
        print("%-8s %9.3f ms (%.3f %.3f)  %8.3f M frames/s  %8.2f M transforms/s" % (
            name, m * 1e3, lo * 1e3, hi * 1e3, nfr[name] / m * 1e-6, nfr[name] * ntap / m * 1e-6))
    m = res["welch"][0]
    line = "cross_welch against run_iq on the same bytes: %.2fx its time; coh alone: %.2fx" % (m / res["run_iq"][0], res["coh"][0] / res["run_iq"][0])
    if "compose" in res:
        line += "; against compose: %.2fx the frames/s" % ((used / m) / (nfr["compose"] / res["compose"][0]))
    if "cross" in res:
        line += "; per transform against cross (L = 1): %.2fx its time" % ((m / used) / (res["cross"][0] / frames))
    print(line)
    by = 8 * hop + 20 * bins / L
    print("algorithmic bytes %.0f per frame (8 H + 20 (N/2 + 1) / L, all four outputs): %.3f GB, %.2f TB/s achieved" % (
        by, used * by * 1e-9, used * by / m * 1e-12))
    if rel is not None:
        print("max |cross_welch - compose| / max over 64 rows, the four outputs: %.2e" % rel)
    sp.close()


def cross(reps, log2_pairs):
    params = G.MtmParams(n=4096, overlap=0.0, w=2.5, kmax=4)
    sp = G.Spectrogram(params)
    xy = stream(log2_pairs)
    frames, bins = sp.num_frames(xy.size(0)), params.n // 2 + 1
    outs = {k: torch.empty((frames, bins), dtype=torch.complex64 if k == "sxy" else torch.float32, device="cuda") for k in ALL}
    m, lo, hi = alternate([("cross", lambda: sp.cross(xy, want=ALL, out=outs))], reps)["cross"]
    print("cross N = 4096, 5 tapers, 2^%d pairs, %d frames: %9.3f ms (%.3f %.3f)  %8.2f M transforms/s  [%s]" % (
        log2_pairs, frames, m * 1e3, lo * 1e3, hi * 1e3, frames * sp.ntapers / m * 1e-6, G.api.LIB_PATH))
    sp.close()


def batch(reps):
    make, L = CASES["fft1024o50"]
    params = make()
    sp = G.Spectrogram(params)
    B, S = 4096, 48000
    g = torch.Generator(device="cuda").manual_seed(2)
    xy = (torch.rand((B, S, 2), device="cuda", generator=g) - 0.5).contiguous()
    nrows, bins = sp.welch_rows(S, L), params.n // 2 + 1
    outs = {k: torch.empty((B, nrows, bins), dtype=torch.complex64 if k == "sxy" else torch.float32, device="cuda") for k in ALL}

    def loop():
        for b in range(B):
            sp.cross_welch(xy[b], L, want=ALL, out={k: t[b] for k, t in outs.items()})

    sp.cross_welch_batch(xy, L, want=ALL, out=outs)
    ref = {k: t.clone() for k, t in outs.items()}
    loop()
    torch.cuda.synchronize()
    for k in ALL:
        a, b = (torch.view_as_real(t) if t.is_complex() else t for t in (ref[k], outs[k]))
        assert torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)), k
    res = alternate([("batch", lambda: sp.cross_welch_batch(xy, L, want=ALL, out=outs)), ("loop", loop)], reps)
    print("## batch: %d stereo streams of %d pairs of f32 (one second at 48 kHz), Hanning, N = 1024, 50 %%, L = step = %d: %d rows a stream (%d frames)" % (
        B, S, L, nrows, nrows * L))
    for name in ("batch", "loop"):
        m, lo, hi = res[name]
        print("%-8s %9.3f ms (%.3f %.3f)  %8.3f M transforms/s" % (name, m * 1e3, lo * 1e3, hi * 1e3, B * nrows * L / m * 1e-6))
    print("cross_welch_batch against the loop of cross_welch: %.1fx (the four outputs equal bit for bit)" % (res["loop"][0] / res["batch"][0]))
    sp.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=["rows", "cross", "batch"], required=True)
    ap.add_argument("--case", choices=sorted(CASES), default="fft4096o75")
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--log2-pairs", type=int, default=28)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    if a.step == "rows":
        rows(a.case, a.reps, a.log2_pairs)
    elif a.step == "cross":
        cross(a.reps, a.log2_pairs)
    else:
        batch(a.reps)
