"""Multi-channel recordings: what the de-interleave kernel and the channel entries cost (one MI355X).
    python tools/channels_rate.py --step kernel            GB/s (read + written bytes) of the stereo and the general form
                                                           beside hipMemcpyAsync device-to-device of the same total bytes
    python tools/channels_rate.py --step device --case C2|C3
                                                           run_channels against the composition a Python user had
                                                           (view(S, 2).t().contiguous() + run_batch) and against run_batch on
                                                           planes that were separate to begin with (the floor)
    python tools/channels_rate.py --step file              run_wav_channels on a stereo WAV against two run_wav calls on two
                                                           mono files that hold the same channels
All on one hour of 48 kHz samples; events on the launch stream, --reps alternating repetitions in ONE process, median (min max).
tools/channels_rate.sh runs the steps, each under its own time limit, and writes profiles/channels_rate.txt."""
import argparse
import ctypes as C
import os
import sys
import tempfile
import time
import wave

sys.path.insert(0, ".")
import numpy as np
import torch
import glfer_amd as G

FRAMES = 3600 * 48000                     # sample frames of a 1-hour 48 kHz recording


def once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


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


def samples(dtype, count, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    if dtype == torch.float32:
        return torch.rand(count, device="cuda", generator=g) - 0.5
    return torch.randint(-20000, 20000, (count,), device="cuda", generator=g, dtype=torch.int32).to(torch.int16)


def loaded_hip_runtime():
    """the HIP runtime this process already runs on (torch's own): the copy must go through the same one"""
    with open("/proc/self/maps") as f:
        paths = sorted({line.split()[-1] for line in f if "libamdhip64" in line})
    assert len(paths) == 1, paths
    return paths[0]


def step_kernel(reps):
    hip = C.CDLL(loaded_hip_runtime())
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    print("de-interleave kernel, %d samples (one hour of 48 kHz stereo), all channels selected; GB/s = (bytes read + bytes written) / time" % (2 * FRAMES))
    for name, dtype in (("s16", torch.int16), ("f32", torch.float32)):
        esz = 2 if dtype == torch.int16 else 4
        total = 2 * FRAMES
        x = samples(dtype, total + 8, 3)
        out = torch.empty(total + 8, dtype=dtype, device="cuda")
        cp = torch.empty(total, dtype=dtype, device="cuda")
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

        def deint(c, wide, off=0):
            def fn():
                os.environ["GLFER_CHANNELS_WIDE"] = "1" if wide else "0"
                G.deinterleave(x[off:off + total], c, out=out[off:off + total].view(c, total // c))
            return fn

        def copy():
            rc = hip.hipMemcpyAsync(cp.data_ptr(), x.data_ptr(), total * esz, 3, st)
            assert rc == 0, rc

        fns = [("stereo form, C = 2", deint(2, True)), ("general form, C = 2", deint(2, False)),
               ("general form, C = 2, bases one sample off", deint(2, True, 1)), ("general form, C = 8", deint(8, True)),
               ("hipMemcpyAsync device to device", copy)]
        res = alternate(fns, reps)
        os.environ.pop("GLFER_CHANNELS_WIDE", None)
        assert torch.equal(out[:total].view(8, total // 8), x[:total].view(total // 8, 8).t())      # (the last call's result)
        gb = 2.0 * total * esz / 1e9
        for fname, _ in fns:
            m, lo, hi = res[fname]
            print("  %s  %-44s %8.3f ms (min %.3f max %.3f)  %7.1f GB/s" % (name, fname, m, lo, hi, gb / (m * 1e-3)))
        base = res["hipMemcpyAsync device to device"][0]
        print("  %s  stereo form / copy: %.2f of the copy's rate; general C = 2: %.2f; general C = 8: %.2f" % (
            name, base / res["stereo form, C = 2"][0], base / res["general form, C = 2"][0], base / res["general form, C = 8"][0]))


def step_device(case, reps):
    if case == "C2":
        params, title = G.FftParams(n=4096, window_type=0, overlap=0.75, sample_format=G.SAMPLES_S16), "C2: N = 4096, Hanning, 75 % overlap"
    else:
        params, title = G.MtmParams(n=4096, overlap=0.0, w=2.5, kmax=4, sample_format=G.SAMPLES_S16), "C3: N = 4096, 5 tapers, no overlap"
    sp = G.Spectrogram(params)
    x = samples(torch.int16, 2 * FRAMES, 5)
    frames = sp.num_frames(FRAMES)
    out = torch.empty((2, frames, sp.pitch), device="cuda")
    planes = x.view(FRAMES, 2).t().contiguous()
    fns = [("run_channels", lambda: sp.run_channels(x, channels=2, out=out)),
           ("t().contiguous() + run_batch", lambda: sp.run_batch(x.view(FRAMES, 2).t().contiguous(), out=out)),
           ("run_batch on separate planes (floor)", lambda: sp.run_batch(planes, out=out))]
    fns[2][1]()
    ref = out.clone()
    for name, fn in fns[:2]:
        out.zero_()
        fn()
        assert torch.equal(out.view(torch.int32), ref.view(torch.int32)), name
    del ref
    res = alternate(fns, reps)
    print("%s; stereo s16, %d frames a channel, device-resident, %d alternating repetitions" % (title, frames, reps))
    for name, _ in fns:
        m, lo, hi = res[name]
        print("  %-40s %9.3f ms (min %.3f max %.3f)  %7.2f M frames/s" % (name, m, lo, hi, 2 * frames / m * 1e-3))
    floor = res["run_batch on separate planes (floor)"][0]
    print("  over the floor: run_channels %+.3f ms, t().contiguous() + run_batch %+.3f ms" % (
        res["run_channels"][0] - floor, res["t().contiguous() + run_batch"][0] - floor))


def write_wav(path, data, channels):
    with wave.open(path, "wb") as w:
        w.setnchannels(channels)
        w.setsampwidth(2)
        w.setframerate(48000)
        w.writeframes(data.tobytes())


def step_file(reps):
    sp = G.Spectrogram(G.FftParams(n=4096, window_type=0, overlap=0.75, sample_format=G.SAMPLES_S16))
    rng = np.random.default_rng(9)
    x = rng.integers(-20000, 20000, (FRAMES, 2), dtype=np.int16)
    with tempfile.TemporaryDirectory() as d:
        stereo, left, right = (os.path.join(d, n) for n in ("stereo.wav", "left.wav", "right.wav"))
        write_wav(stereo, x, 2)
        write_wav(left, np.ascontiguousarray(x[:, 0]), 1)
        write_wav(right, np.ascontiguousarray(x[:, 1]), 1)
        del x

        def one_pass():
            return sp.run_wav_channels(stereo)

        def two_passes():
            return sp.run_wav(left), sp.run_wav(right)

        ts = {"run_wav_channels (one pass, one file)": [], "two run_wav calls (two mono files)": []}
        same = None
        for r in range(reps + 1):
            for name, fn in (("run_wav_channels (one pass, one file)", one_pass), ("two run_wav calls (two mono files)", two_passes)):
                t0 = time.perf_counter()
                got = fn()
                ts[name].append((time.perf_counter() - t0) * 1e3)
                if r == 0:
                    if same is None:
                        same = got
                    else:
                        assert np.array_equal(same[0], got[0]) and np.array_equal(same[1], got[1])
                        same = None
                del got
        print("file entry, C2 plan (N = 4096, Hanning, 75 %% overlap), 1-hour 48 kHz stereo 16-bit WAV (%d frames a channel, rows to pageable "
              "host memory), wall clock, files in the page cache" % sp.num_frames(FRAMES))
        for name, v in ts.items():
            m, lo, hi = med(v[1:])
            print("  %-40s first call %9.1f ms; then %9.1f ms (min %.1f max %.1f, %d calls)" % (name, v[0], m, lo, hi, reps))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=["kernel", "device", "file"], required=True)
    ap.add_argument("--case", choices=["C2", "C3"], default="C2")
    ap.add_argument("--reps", type=int, default=6)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    if a.step == "kernel":
        step_kernel(a.reps)
    elif a.step == "device":
        step_device(a.case, a.reps)
    else:
        step_file(a.reps)
