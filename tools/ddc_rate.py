"""The digital down-converter and the zoom: what they cost on one MI355X.
    python tools/ddc_rate.py --step ddc --case 16x129|64x513|1x1 --fmt f32|s16
        Ddc.run on a device-resident real stream of 2^28 samples, beside
          memcpy   a device-to-device copy of the input bytes (hipMemcpyAsync through torch's copy_): the roof of the mixer case
          compose  the same outputs on the same GPU from torch: the stream times a precomputed cos and sin table (the mixer), then
                   conv1d with stride D on both parts (T = 1: the mixer alone); integer input is converted first, as it must be
        input samples/s, read-plus-written bytes/s (4 or 2 bytes a sample in, 8 bytes an output), and the two bounds: HBM at 8 TB/s
        over those bytes, and 2 T / D FP32 multiply-adds per input sample at the packed rate of 256 CUs x 128 a clock x 2.4 GHz.
    python tools/ddc_rate.py --step zoom
        run_zoom at D = 64, N = 16384, 50 % overlap against Spectrogram(FftParams(n=1048576, overlap=0.5)).run on the same 2^28
        samples: frames/s of equal resolution (fs / 2^20 per bin), 512 frames each.
Events on the launch stream; a timed sample repeats its call until it spans at least 0.3 s; --reps alternating repetitions in ONE
process, median (min max).  Each step is a process of its own, meant to run under its own time limit."""
import argparse
import sys

sys.path.insert(0, ".")
import numpy as np
import torch
import glfer_amd as G

HBM_BYTES_PER_S = 8.0e12
FMA_PER_S = 256 * 128 * 2.4e9              # a CU retires 64 lanes a clock, v_pk_fma_f32 two multiply-adds a lane
FREQ = 0.1234567


def timed(fn, k):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(k):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3 / k


def alternate(fns, reps):
    """every fn warmed up and sized to 0.3 s, then reps rounds of all of them in turn: {name: (median, min, max)}"""
    ks = {}
    for name, fn in fns:
        fn()
        torch.cuda.synchronize()
        ks[name] = max(1, int(np.ceil(0.3 / max(timed(fn, 2), 1e-6))))
    ts = {name: [] for name, _ in fns}
    for _ in range(reps):
        for name, fn in fns:
            ts[name].append(timed(fn, ks[name]))
    return {name: (sorted(v)[len(v) // 2], min(v), max(v)) for name, v in ts.items()}


def ddc(case, fmt, reps, log2_samples):
    D, T = (int(v) for v in case.split("x"))
    S = 1 << log2_samples
    g = torch.Generator(device="cuda").manual_seed(1)
    xf = torch.rand(S, device="cuda", generator=g) - 0.5
    if fmt == "s16":
        x = (xf * 40000).to(torch.int16)
        xf = x.float() / 32768.0
        esz, sfmt = 2, G.SAMPLES_S16
    else:
        x, esz, sfmt = xf, 4, G.SAMPLES_F32
    taps = G.ddc_design(D, T)
    d = G.Ddc(D, FREQ, taps=taps, sample_format=sfmt)
    nout = d.num_out(S)
    out = torch.empty(nout, dtype=torch.complex64, device="cuda")
    dst = torch.empty_like(x)
    # the composition's tables (not timed): the oscillator in double, the taps as conv1d weights
    n = torch.arange(S, device="cuda", dtype=torch.float64)
    ang = -2.0 * np.pi * torch.remainder(n * FREQ, 1.0)
    cs, sn = torch.cos(ang).float(), torch.sin(ang).float()
    del n, ang
    w = torch.from_numpy(taps[::-1].copy()).cuda()[None, None]
    outc = torch.empty((2, nout), dtype=torch.float32, device="cuda")

    def compose():
        v = x if fmt == "f32" else x.float() / 32768.0
        for i, osc in enumerate((cs, sn)):
            z = v * osc
            if T == 1:
                outc[i] = z[D - 1::D][:nout]
            else:
                outc[i] = torch.nn.functional.conv1d(z[None, None, D - 1:], w, stride=D, padding=T - 1)[0, 0, :nout]

    d.run(x, out=out)
    compose()
    torch.cuda.synchronize()
    lo = T                                                       # (past the zero history, where the float32 oscillator is still good)
    a, b = out[lo:lo + 4096], torch.complex(outc[0, lo:lo + 4096], outc[1, lo:lo + 4096])
    rel = float(((a - b).abs().max() / a.abs().max()).item())
    assert rel < 1e-3, rel

    res = alternate([("ddc", lambda: d.run(x, out=out)), ("memcpy", lambda: dst.copy_(x)), ("compose", compose)], reps)
    by = S * esz + nout * 8
    fma = 2.0 * T / D * S
    print("## ddc %s %s: D = %d, T = %d, 2^%d real %s samples, %d outputs" % (case, fmt, D, T, log2_samples, fmt, nout))
    for name in ("ddc", "memcpy", "compose"):
        m, mn, mx = res[name]
        print("%-8s %9.3f ms (%.3f %.3f)  %8.2f G samples/s" % (name, m * 1e3, mn * 1e3, mx * 1e3, S / m * 1e-9))
    m = res["ddc"][0]
    t_hbm, t_fma = by / HBM_BYTES_PER_S, fma / FMA_PER_S
    print("ddc: %.2f TB/s read plus written (%d bytes in, %d out); memcpy moves %.2f TB/s (read plus written); ddc takes %.2fx the copy's time" % (
        by / m * 1e-12, S * esz, nout * 8, 2 * S * esz / res["memcpy"][0] * 1e-12, m / res["memcpy"][0]))
    print("bounds: HBM %.3f ms at 8 TB/s, FP32 %.3f ms for %.1f multiply-adds per input sample at %.1f T/s: %s binds; measured is %.2fx it" % (
        t_hbm * 1e3, t_fma * 1e3, 2.0 * T / D, FMA_PER_S * 1e-12, "HBM" if t_hbm > t_fma else "FP32", m / max(t_hbm, t_fma)))
    print("ddc against the torch composition: %.2fx its samples/s (max difference over 4096 outputs %.1e of the largest)" % (res["compose"][0] / m, rel))
    d.close()


def zoom(reps, log2_samples):
    S = 1 << log2_samples
    g = torch.Generator(device="cuda").manual_seed(2)
    x = torch.rand(S, device="cuda", generator=g) - 0.5
    D, N, NB = 64, 16384, 1 << 20
    sp = G.Spectrogram(G.FftParams(n=N, window_type=G.WINDOWS["hanning"], overlap=0.5))
    big = G.Spectrogram(G.FftParams(n=NB, window_type=G.WINDOWS["hanning"], overlap=0.5))
    d = G.Ddc(D, FREQ)
    fz, fb = sp.num_frames(d.num_out(S)), big.num_frames(S)
    oz = torch.empty((fz, N), dtype=torch.float32, device="cuda")
    ob = torch.empty((fb, big.pitch), dtype=torch.float32, device="cuda")
    res = alternate([("zoom", lambda: sp.run_zoom(d, x, out=oz, centered=True)), ("big", lambda: big.run(x, out=ob))], reps)
    print("## zoom: 2^%d real f32 samples; run_zoom D = %d (T = %d), N = %d, 50 %% overlap: %d frames of %d bins; Spectrogram(n=%d, 50 %%).run: %d frames of %d bins" % (
        log2_samples, D, len(d.taps), N, fz, N, NB, fb, big.bins))
    for name, nf in (("zoom", fz), ("big", fb)):
        m, mn, mx = res[name]
        print("%-5s %9.3f ms (%.3f %.3f)  %9.1f frames/s  %7.2f G samples/s" % (name, m * 1e3, mn * 1e3, mx * 1e3, nf / m, S / m * 1e-9))
    print("run_zoom against the N = %d run: %.2fx the frames/s at equal resolution" % (NB, (fz / res["zoom"][0]) / (fb / res["big"][0])))
    for h in (d, sp, big):
        h.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=["ddc", "zoom"], required=True)
    ap.add_argument("--case", default="16x129")
    ap.add_argument("--fmt", choices=["f32", "s16"], default="f32")
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--log2-samples", type=int, default=28)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    if a.step == "ddc":
        ddc(a.case, a.fmt, a.reps, a.log2_samples)
    else:
        zoom(a.reps, a.log2_samples)
