"""Every launcher of glfer_hip.cpp on fixed inputs, one line per case with the SHA-256 of each output buffer: two builds of the
library compute the same thing exactly when their outputs of this tool are equal line for line, and launch the same thing
when the kernel traces of two runs are (rocprofv3 --kernel-trace -- python tools/launcher_identity.py).
    python tools/launcher_identity.py                        this tree's library
    GLFER_LIB_PATH=<other libglfer_hip.so> python tools/launcher_identity.py
The cases: the cut-edge calls of tests/test_gpu_frame_cuts.py (plans A .. D, sub_mean 0 / 1 / fast, rows and batch at every
(first, nframes), the ragged call, plan A's F entries), then one 4 096-frame call per plan through the rows, batch, ragged,
average, average-batch, F and F-batch entries; then the column entries (column_cases: display, the waterfalls and their two
multi-GPU halves, the moving averages; `python tools/launcher_identity.py columns` runs these alone), and the LMP statistic's
three entries and LMP plans at every ring size's form (lmp_cases; `python tools/launcher_identity.py lmp` runs these alone);
then the estimator launchers' own branches (launcher_cases: every launch site of spectro16*.hip that the Python API and the
documented environment switches reach, each at the smallest frame count that takes it; `python tools/launcher_identity.py
launchers` runs these alone, and `... mtab` the few that need GLFER_MTAB_WPS=2, which the library reads once per process).
Inputs come from fixed seeds on the host; nothing is timed."""
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
    if fmt == 2:
        x = np.clip(np.round(x * 100.0 + 128.0), 0, 255).astype(np.uint8)
    else:
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


# ---- the column entries (waterfall.cpp and the update_avg entries): PSD-like rows from fixed seeds, the carried states in the line
AVERAGES = {0: dict(avg_mode=0), 1: dict(avg_mode=1, depth=4, minbin=10, maxbin=500), 2: dict(avg_mode=2, depth=4, minbin=0, maxbin=513),
            3: dict(avg_mode=3, depth=7, minbin=3, maxbin=511)}
DISPLAYS = {"lin auto": dict(scale_type=0, autoscale=1, overlap=0.75, palette=3, thr_level=10.0),
            "lin fixed": dict(scale_type=1, autoscale=0, max_level_db=-3.0, min_level_db=-40.0, palette=1),
            "log auto": dict(scale_type=2, autoscale=1, overlap=0.5, palette=0),
            "log fixed": dict(scale_type=3, autoscale=0, max_level_db=-20.0, min_level_db=-80.0, thr_level=5.0, palette=5)}
RAGGED_LENGTHS = [0, 1, 255, 256, 257, 1281, 3000]


def psd_rows(shape, seed):
    """non-negative floats with a floor and a few strong bins; the leading dimension (streams) differs in scale"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.rand(shape, generator=g, device="cuda", dtype=torch.float32)
    x = x * x * x * x * 0.1 + 2e-4
    if len(shape) == 3:
        x = x * torch.tensor([10.0 ** ((b * 37) % 7 - 3) for b in range(shape[0])], device="cuda", dtype=torch.float32)[:, None, None]
    return x.contiguous()


def displays(n, **options):
    """every third one a first buffer, the others carried levels of their own"""
    out = []
    for b in range(n):
        d = G.Display(first_buffer=1 if b % 3 == 0 else 0, **options)
        if b % 3:
            d.display_max_lvl, d.display_min_lvl = 0.05 + 0.01 * (b % 5), 0.002 + 0.0005 * (b % 4)
        out.append(d)
    return out


def states(disps):
    return "states " + " ".join("%d/%s/%s" % (d.first_buffer, float(d.display_max_lvl).hex(), float(d.display_min_lvl).hex()) for d in disps)


def with_env(fn, **env):
    """fn() with these environment switches set (the library reads them per call)"""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return fn()
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def halves(disp, rows, av, cut):
    """glfer_hip_levels_host over the whole call's statistics, then glfer_hip_waterfall_map_device over rows [0, cut) and [cut, end)"""
    import ctypes as C
    L = G.api.lib()
    n, bins = rows.shape
    stats = np.ascontiguousarray(G.compute_floor(rows).cpu().numpy())
    levels = np.empty((n, 4), np.float32)
    assert L.glfer_hip_levels_host(C.byref(disp), stats.ctypes.data, n, levels.ctypes.data, 0) == 0
    d_levels = torch.from_numpy(levels).to("cuda")
    rgb = torch.zeros((n, bins, 3), dtype=torch.uint8, device="cuda")
    lev = torch.zeros((n, bins), dtype=torch.int16, device="cuda")
    for first, count in ((0, cut), (cut, n - cut)):
        assert L.glfer_hip_waterfall_map_device(C.byref(disp), av["avg_mode"], av.get("depth", 1), av.get("minbin", 0), av.get("maxbin", 1), 0,
                                                rows.data_ptr(), first, count, bins, d_levels[first:].data_ptr(), rgb[first:].data_ptr(),
                                                lev[first:].data_ptr(), None) == 0
    return rgb, lev, d_levels


def column_cases():
    # display: from rows and from averaged rows
    rows = psd_rows((3000, 513), 21)
    stats = G.compute_floor(rows)
    avg = G.update_avg(G.AVG_PLAIN, rows, 4, 0, 513)[0]
    for dname, opt in sorted(DISPLAYS.items()):
        for sname, src in (("rows", rows), ("averaged rows", avg)):
            d = displays(2, **opt)[1]
            print("display %s, %s: %s %s" % (dname, sname, sha(*G.display(d, src, stats)), states([d])))
    # waterfall: each mode on lin / log and autoscale / fixed, two shapes, the two switches
    for shape in ((3000, 513), (300, 2049)):
        rows = psd_rows(shape, 22)
        for dname, opt in sorted(DISPLAYS.items()):
            for mode, av in sorted(AVERAGES.items()):
                av = dict(av, maxbin=min(av.get("maxbin", 1), shape[1]))
                for ename, env in (("", {}), (" TILE=1024", dict(GLFER_WATERFALL_TILE="1024")), (" FUSED=0", dict(GLFER_WATERFALL_FUSED="0"))):
                    d = displays(2, **opt)[1]
                    out = with_env(lambda: G.waterfall(d, rows, want_stats=True, **av), **env)
                    print("waterfall %dx%d %s mode %d%s: %s %s" % (shape[0], shape[1], dname, mode, ename, sha(*out), states([d])))
        sys.stdout.flush()
    # waterfall_batch: 5 streams x 1 281 rows
    rows = psd_rows((5, 1281, 513), 23)
    for dname, opt in sorted(DISPLAYS.items()):
        for mode, av in sorted(AVERAGES.items()):
            for ename, env in (("", {}), (" TILE=1024", dict(GLFER_WATERFALL_TILE="1024")), (" FUSED=0", dict(GLFER_WATERFALL_FUSED="0"))):
                ds = displays(5, **opt)
                out = with_env(lambda: G.waterfall_batch(ds, rows, want_stats=True, **av), **env)
                print("waterfall_batch 5x1281x513 %s mode %d%s: %s %s" % (dname, mode, ename, sha(*out), states(ds)))
    sys.stdout.flush()
    # waterfall_ragged: the lengths around the level chunk, once more by the stream-by-stream route; then a set whose short
    # streams take the staged class and whose long one takes the fused (depth 40, tests/test_gpu_waterfall_ragged.py)
    starts = np.concatenate([[0], np.cumsum(RAGGED_LENGTHS)])
    rows = psd_rows((int(starts[-1]), 513), 24)
    for dname, opt in sorted(DISPLAYS.items()):
        for mode, av in sorted(AVERAGES.items()):
            for ename, env in (("", {}), (" TILE=1024 (stream by stream)", dict(GLFER_WATERFALL_TILE="1024"))):
                ds = displays(len(RAGGED_LENGTHS), **opt)
                out = with_env(lambda: G.waterfall_ragged(ds, rows, starts, want_stats=True, **av)[:3], **env)
                print("waterfall_ragged %s mode %d%s: %s %s" % (dname, mode, ename, sha(*out), states(ds)))
    mixed = [100, 0, 3000, 17000, 40000]
    mstarts = np.concatenate([[0], np.cumsum(mixed)])
    mrows = psd_rows((int(mstarts[-1]), 129), 27)
    for dname in ("log auto", "lin fixed"):
        for mode in (1, 2):
            ds = displays(len(mixed), **DISPLAYS[dname])
            out = G.waterfall_ragged(ds, mrows, mstarts, avg_mode=mode, depth=40, minbin=3, maxbin=127, want_stats=True)[:3]
            print("waterfall_ragged fused and staged streams, %s mode %d depth 40: %s %s" % (dname, mode, sha(*out), states(ds)))
    del mrows
    sys.stdout.flush()
    # the averages, each mode
    batch = psd_rows((5, 1281, 513), 25)
    for mode in (G.AVG_SUMAVG, G.AVG_PLAIN, G.AVG_SUMEXTREME):
        for depth in (4, 7):
            print("update_avg mode %d depth %d: %s" % (mode, depth, sha(*G.update_avg(mode, rows, depth, 3, 511))))
            print("update_avg_batch mode %d depth %d: %s" % (mode, depth, sha(*G.update_avg_batch(mode, batch, depth, 3, 511))))
            print("update_avg_ragged mode %d depth %d: %s" % (mode, depth, sha(*G.update_avg_ragged(mode, rows, starts, depth, 3, 511)[:2])))
    for depth in (4, 7):
        print("avg_cum depth %d: %s" % (depth, sha(G.avg_cum(rows, depth, 3, 511))))
    # the two halves of a waterfall over several GPUs
    rows = psd_rows((700, 129), 26)
    for dname, opt in sorted(DISPLAYS.items()):
        for mode, av in sorted(AVERAGES.items()):
            av = dict(av, minbin=min(av.get("minbin", 0), 3), maxbin=min(av.get("maxbin", 1), 129))
            d = displays(2, **opt)[1]
            print("halves 700x129 cut 300 %s mode %d: %s %s" % (dname, mode, sha(*halves(d, rows, av, 300)), states([d])))
    sys.stdout.flush()


LMP_AVGS = (1, 2, 3, 4, 8, 7, 16, 65)


def lmp_cases():
    """the LMP statistic: the stage over one stream, a batch and ragged streams at every ring size's form (registers, LDS from
    64 frames, frame by frame), then LMP plans through run, run_batch and run_ragged"""
    for n in (256, 1024):
        rect = G.Spectrogram(G.FftParams(n=n, window_type=G.WINDOWS["rectangular"], overlap=0.0))
        x = streams(3, 70 * n, 0, 14)
        P70 = rect.run_batch(x)                                       # [3][70][bins]
        for frames in (5, 70):
            P = P70[:, :frames].contiguous()
            for avg in LMP_AVGS:
                for first in uniq([0, 1, avg, avg + 1]):
                    if first >= frames:
                        continue
                    lead = min(avg - 1, first)
                    view = P[:, first - lead:]
                    print("lmp stage n %d frames %d avg %d first %d: %s; batch of 3: %s" % (
                        n, frames, avg, first, sha(G.lmp_statistic(view[1].contiguous(), avg, first_frame=first, lead=lead)),
                        sha(G.lmp_statistic_batch(view, avg, first_frame=first, lead=lead))))
        for avg in LMP_AVGS:
            counts = [0, 1, 2, avg - 1, 15, 16, 17, 70]
            rows = torch.cat([P70[b % 3, :c] for b, c in enumerate(counts)])
            print("lmp stage ragged n %d avg %d: %s" % (n, avg, sha(G.lmp_statistic_ragged(rows, np.concatenate([[0], np.cumsum(counts)]), avg)[0])))
            for sub in (0, 1):
                sp = G.Spectrogram(G.LmpParams(n=n, overlap=0.0, avg=avg, sub_mean=sub))
                lens = [c * n + (7 if b % 3 == 0 else 0) for b, c in enumerate(counts)]
                offs = [(b % 3) * x.size(1) for b in range(len(lens))]
                print("lmp plan n %d avg %d sub_mean %d: run %s / %s; run_batch %s / %s; run_ragged %s" % (
                    n, avg, sub, sha(sp.run(x[1])), sha(sp.run(x[1], first_frame=avg + 1)), sha(sp.run_batch(x)),
                    sha(sp.run_batch(x, first_frame=avg + 1)), sha(sp.run_ragged(x.reshape(-1), offs, lens)[0])))
                sp.close()
        sys.stdout.flush()
        rect.close()


FMT_NAMES = {0: "f32", 1: "s16", 2: "u8"}


def case(label, fn):
    """one line: the hashes of what fn returns, or its refusal -- two builds must also refuse alike"""
    try:
        out = fn()
        print("%s: %s" % (label, sha(*(out if isinstance(out, (tuple, list)) else (out,)))))
    except (G.api.GlferHipError, AssertionError) as e:
        print("%s: refused (%s)" % (label, (str(e).splitlines() or [type(e).__name__])[0][:100]))


def three_ways(tag, sp, frames, fmt, seed, nb=3, batch=True):
    """the rows, batch and ragged entries over streams of `frames` frames"""
    x = streams(nb, frames * sp.hop + 2 * (sp.hop // 6) + 8, fmt, seed)
    case(tag + " rows", lambda: sp.run(x[nb - 1]))
    if batch:
        case(tag + " batch", lambda: sp.run_batch(x))
        case(tag + " ragged", lambda: ragged(sp, x, [frames, max(frames // 3, 1), frames - 6][:nb], [0, 5, 0][:nb]))
    return x


def launcher_cases(mtab=False):
    """The estimator launchers' branches beyond what main() reaches; profiles/launch_scaffold_identity.txt lists the launch
    sites with the case that reaches each."""
    fft = lambda **kw: G.Spectrogram(G.FftParams(window_type=0, **kw))
    mtm = lambda **kw: G.Spectrogram(G.MtmParams(**kw))
    produced = (dict(GLFER_FUSED_MIN_FRAMES="64", GLFER_MEANS_PRODUCERS="8"),
                dict(GLFER_FUSED_MIN_FRAMES="64", GLFER_MEANS_PRODUCERS="8", GLFER_FUSED_BLOCK_FRAMES="16", GLFER_FUSED_LOOK="64"))
    if mtab:
        # spectro16h's table form at two wavefronts per SIMD: the means given (reference order), one stream; every hop of the ladder
        for n in (1024, 4096):
            for ovl in (0.0, 0.5, 0.75, 0.875, 0.6):
                sp = fft(n=n, overlap=ovl, sub_mean=G.SUBMEAN_EXACT)
                three_ways("mtab h n %d overlap %g" % (n, ovl), sp, 300, 0, 31, batch=False)
                sp.close()
        sp = fft(n=1024, overlap=0.5, sub_mean=G.SUBMEAN_EXACT)
        x = streams(1, 300 * sp.hop, 0, 32)
        for env in produced:
            case("mtab h produced means %s" % sorted(env.items()), lambda: with_env(lambda: sp.run(x[0]), **env))
        sp.close()
        return
    # spectro16h, the periodogram: every hop of the ladders (16, 8, 4, 2 sixteenths) and one outside them, every sample format,
    # no mean removal / the means given (reference order) / summed in the kernel (fast); history zeroed in every frame
    for n in (512, 1024):
        for ovl in (0.0, 0.5, 0.75, 0.875, 0.6):
            for fmt in (0, 1, 2):
                for sub in SUB_MEANS:
                    for hm in ((0, 1) if sub == 0 and fmt == 0 else (0,)):
                        sp = fft(n=n, overlap=ovl, sub_mean=sub, sample_format=fmt, history_mode=hm)
                        three_ways("h n %d overlap %g %s sub_mean %d history %d" % (n, ovl, FMT_NAMES[fmt], sub, hm), sp, 40, fmt, 33)
                        sp.close()
        sys.stdout.flush()
    # ... the means produced inside the launch (GLFER_MEANS_PRODUCERS; the lock-stepped form with GLFER_FUSED_BLOCK_FRAMES)
    sp = fft(n=1024, overlap=0.5, sub_mean=G.SUBMEAN_EXACT)
    x = streams(1, 300 * sp.hop, 0, 32)
    for env in produced:
        case("h produced means %s" % sorted(env.items()), lambda: with_env(lambda: sp.run(x[0]), **env))
    sp.close()
    # ... the register-reuse forms: work >= 4 x resident workgroups (3 072 workgroups of 8, 2 and 1 frames at N = 1024, 4096, 16384)
    for n, ovl, frames in ((1024, 0.5, 24800), (1024, 0.75, 24800), (1024, 0.875, 24800), (4096, 0.75, 6400), (16384, 0.875, 1100)):
        for fmt in (0, 1):
            sp = fft(n=n, overlap=ovl, sample_format=fmt)
            x = streams(2, frames * sp.hop + 64, fmt, 34)
            tag = "h shifted n %d overlap %g %s" % (n, ovl, FMT_NAMES[fmt])
            case(tag + " rows", lambda: sp.run(x[1]))
            case(tag + " batch", lambda: sp.run_batch(x))
            case(tag + " ragged", lambda: ragged(sp, x, [frames, 100], [0, 5]))
            sp.close()
            del x
        sys.stdout.flush()
    # ... the average inside the launch (a launch of >= 256 frames with full windows), single and batch
    for n in (512, 1024, 4096):
        for ovl in (0.0, 0.5, 0.75, 0.875, 0.6):
            for sub in (0, G.SUBMEAN_EXACT):
                for fmt in ((0, 1) if ovl == 0.5 else (0,)):
                    sp = fft(n=n, overlap=ovl, sub_mean=sub, sample_format=fmt)
                    x = streams(2, 600 * sp.hop + 64, fmt, 35)
                    tag = "h average n %d overlap %g %s sub_mean %d" % (n, ovl, FMT_NAMES[fmt], sub)
                    for depth in (1, 4):
                        case("%s depth %d" % (tag, depth), lambda: sp.run_avg(x[0], G.AVG_PLAIN, depth, 3, sp.bins - 5, want_psd=True))
                        case("%s depth %d batch" % (tag, depth), lambda: sp.run_avg_batch(x, G.AVG_PLAIN, depth, 3, sp.bins - 5, want_psd=True))
                    sp.close()
        sys.stdout.flush()
    # spectro16 (and spectro_small below N = 256), the general path: RA9MB and the limiter, the spectrum output
    for n in (128, 256, 1024, 4096, 16384):
        for fmt in (0, 2):
            sp = G.Spectrogram(G.FftParams(n=n, window_type=0, overlap=0.5, a=0.5, limiter=1, sample_format=fmt))
            x = three_ways("packed general n %d %s" % (n, FMT_NAMES[fmt]), sp, 24, fmt, 36)
            sp.close()
            sp = fft(n=n, overlap=0.5, sample_format=fmt)
            case("packed spectrum n %d %s" % (n, FMT_NAMES[fmt]), lambda: sp.run(x[0], spectrum=True))
            sp.close()
    sys.stdout.flush()
    # the multitaper: even counts (spectro16), odd ones (spectro16xl's LDS tables; spectro16x with 23 tapers, whose tables do not
    # fit; spectro16y at N = 4096; packed at 2048 and from 8192), spectro16h's form at N = 8192 and spectro16w's at 16384; the
    # forms forced with GLFER_FORM, spectro16y's full tables and static stride
    hops = ((0.0, 0), (0.0, G.SUBMEAN_EXACT), (0.5, G.SUBMEAN_FAST), (0.75, G.SUBMEAN_FAST), (0.5, 0))
    shapes = [(n, 2.5, k) for n in (256, 512, 1024, 2048, 4096) for k in (3, 4, 6)] + [(1024, 12.0, 22), (8192, 2.5, 4), (16384, 2.5, 4)]
    for n, w, kmax in shapes:
        for ovl, sub in (hops if n <= 4096 else hops[:3]):
            for fmt in ((0, 2) if kmax == 4 else (0,)):
                for hm in ((0, 1) if (ovl, sub, fmt, kmax) == (0.5, 0, 0, 4) else (0,)):
                    sp = mtm(n=n, overlap=ovl, w=w, kmax=kmax, sub_mean=sub, sample_format=fmt, history_mode=hm)
                    tag = "mtm n %d tapers %d overlap %g %s sub_mean %d history %d" % (n, kmax + 1, ovl, FMT_NAMES[fmt], sub, hm)
                    x = three_ways(tag, sp, 40, fmt, 37)
                    forms = [dict(GLFER_FORM=f) for f in ("w", "h", "x") if n >= 2048 and kmax == 4]
                    if n == 4096:
                        forms += [dict(GLFER_Y_TAPERS="full"), dict(GLFER_Y_QUEUE="0"), dict(GLFER_Y_TAPERS="full", GLFER_Y_QUEUE="0")]
                    for env in forms:
                        etag = "%s %s" % (tag, " ".join("%s=%s" % kv for kv in sorted(env.items())))
                        case(etag + " rows", lambda: with_env(lambda: sp.run(x[1]), **env))
                        case(etag + " batch", lambda: with_env(lambda: sp.run_batch(x), **env))
                        case(etag + " ragged", lambda: with_env(lambda: ragged(sp, x, [40, 13, 34], [0, 5, 0]), **env))
                    sp.close()
        sys.stdout.flush()
    # the periodogram through spectro16w (GLFER_FORM=w)
    for n in (2048, 4096, 8192, 16384):
        for hm in (0, 1):
            sp = fft(n=n, overlap=0.5, history_mode=hm)
            with_env(lambda: three_ways("w periodogram n %d history %d" % (n, hm), sp, 24, 0, 38), GLFER_FORM="w")
            sp.close()
    # N = 32768 both ways (the two-kernel form; spectro16w's single kernel with GLFER_FORM=w and for the spectrum), N = 65536
    for make, name in ((lambda **kw: fft(**kw), "fft"), (lambda **kw: mtm(w=2.5, kmax=4, **kw), "mtm")):
        for fmt in (0, 1):
            for ovl in (0.0, 0.5):
                sp = make(n=32768, overlap=ovl, sample_format=fmt)
                tag = "n 32768 %s overlap %g %s" % (name, ovl, FMT_NAMES[fmt])
                x = three_ways(tag, sp, 6, fmt, 39, nb=2)
                with_env(lambda: three_ways(tag + " GLFER_FORM=w", sp, 6, fmt, 39, nb=2), GLFER_FORM="w")
                if name == "fft":
                    case(tag + " spectrum", lambda: sp.run(x[0], spectrum=True))
                sp.close()
    sp = fft(n=65536, overlap=0.5)
    three_ways("n 65536 fft", sp, 4, 0, 40, nb=2)
    sp.close()
    sys.stdout.flush()
    # complex I/Q rows (spectro16c) and the cross-spectrum (spectro16cx): single and batch over their size lists, every format
    for n in (256, 512, 1024, 2048, 4096, 8192, 16384):
        for fmt in (0, 1, 2):
            for name, sp in (("fft", fft(n=n, overlap=0.5, sample_format=fmt)), ("mtm", mtm(n=n, overlap=0.5, w=2.5, kmax=2, sample_format=fmt))):
                x = streams(3, 2 * (20 * sp.hop + 8), fmt, 41).reshape(3, -1, 2)
                tag = "n %d %s %s" % (n, name, FMT_NAMES[fmt])
                case("iq " + tag, lambda: sp.run_iq(x[1], centered=(fmt == 1), swap=(fmt == 2)))
                case("iq batch " + tag, lambda: sp.run_iq_batch(x))
                if name == "mtm":
                    case("cross " + tag, lambda: tuple(sp.cross(x[1], want=("sxx", "syy", "sxy", "coh"))))
                    case("cross batch " + tag, lambda: tuple(sp.cross_batch(x, want=("sxx", "syy", "sxy", "coh"))))
                sp.close()
        sys.stdout.flush()
    # the F statistic on integer samples (the float forms: main())
    for fmt in (1, 2):
        sp = mtm(n=512, overlap=0.5, w=2.5, kmax=4, sample_format=fmt)
        x = streams(3, 40 * sp.hop + 8, fmt, 42)
        tag = "F n 512 %s" % FMT_NAMES[fmt]
        case(tag, lambda: sp.ftest(x[1]))
        case(tag + " batch", lambda: sp.ftest_batch(x))
        case(tag + " rows-and-F", lambda: sp.rows_ftest(x[1]))
        case(tag + " rows-and-F batch", lambda: sp.rows_ftest_batch(x))
        sp.close()


def main():
    if sys.argv[1:] == ["columns"]:
        return column_cases()
    if sys.argv[1:] == ["lmp"]:
        return lmp_cases()
    if sys.argv[1:] == ["launchers"]:
        return launcher_cases()
    if sys.argv[1:] == ["mtab"]:
        os.environ["GLFER_MTAB_WPS"] = "2"              # (read once, at the first launch that asks)
        return launcher_cases(mtab=True)
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
    lmp_cases()
    column_cases()
    launcher_cases()


if __name__ == "__main__":
    main()
