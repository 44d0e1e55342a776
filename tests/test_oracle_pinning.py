"""CPU tests: the oracle is pinned (a) bit-exact against the reference's own objects (oracle/_ref:
fft_radix2.c, g-l_dpss.c, avg.c, util.c), through what they returned on the same seeded inputs
(tests/golden/ref_pins.json, made by tests/_refpins.py), (b) against independent known
answers (numpy rfft in float64, scipy DPSS, Parseval) for the parts restating fft.c/mtm.c, and
(c) against the committed golden vectors."""
import glob
import os

import numpy as np
import pytest

import _refpins as P
from _signals import rel_err, synth

GOLD = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def pins():
    return P.load()


@pytest.mark.parametrize("n", P.FFT_NS)
def test_fft_bitexact_vs_reference(oracle, pins, n):
    for x, want in zip(P.fft_inputs(n), pins["fft"][str(n)]):
        assert P.sha(x) == want["in"], "the seeded input is not the one the pins were made from"
        assert P.sha(oracle.rfft_halfcomplex(x)) == want["out"]


@pytest.mark.parametrize("n,kmax,nw", P.DPSS_CASES)
def test_dpss_bitexact_vs_reference(oracle, pins, n, kmax, nw):
    v, s = oracle.dpss(n, kmax, nw)
    want = pins["dpss"]["%d-%d-%s" % (n, kmax, nw)]
    assert want["err"] == 0
    assert P.sha(v) == want["v"] and P.sha(s) == want["s"]


def test_bessel_and_svd_bitexact_vs_reference(oracle, pins):
    assert [P.num(oracle.bessel_i0(x)) for x in P.bessel_inputs()] == pins["bessel_i0"]
    A = P.svd_input()
    want = pins["svd"]
    assert P.sha(A) == want["in"], "the seeded input is not the one the pins were made from"
    rc, U, S, Q = oracle.svd(A)
    assert rc == want["rc"] == 0
    assert P.sha(U) == want["u"] and P.sha(S) == want["s"] and P.sha(Q) == want["q"]


@pytest.mark.parametrize("mode", P.AVG_MODES)
def test_avg_bitexact_vs_reference(oracle, pins, mode):
    rows = P.avg_inputs()
    assert P.sha(np.stack(rows)) == pins["avg_in"], "the seeded input is not the one the pins were made from"
    a1 = oracle.Averager(1024, 4)
    for f, (psd, want) in enumerate(zip(rows, pins["avg"][mode])):
        assert P.avg_step(a1.update(mode, psd, 10, 400, max0=f % 2, n=513)) == want, f


def test_fft_known_answer_numpy(oracle):
    for n in (64, 1024, 4096):
        x = synth(n, seed=n)
        hc = oracle.rfft_halfcomplex(x).astype(np.float64)
        X = np.fft.rfft(x.astype(np.float64))
        want = np.concatenate([X.real, X.imag[1:-1][::-1]])
        assert np.abs(hc - want).max() / np.abs(want).max() < 4e-6    # the reference's own f32 error


def test_window_properties(oracle):
    for name, t in oracle.WINDOWS.items():
        w = oracle.window(t, 1024).astype(np.float64)
        assert abs((w * w).sum() - 1.0) < 1e-5, name                  # fft.c:352-359
        assert np.allclose(w, w[::-1], atol=1e-6), name               # all eight are symmetric
    h = oracle.window(0, 1024).astype(np.float64)
    hn = np.hanning(1024)
    assert np.allclose(h, hn / np.sqrt((hn * hn).sum()), atol=1e-7)
    k = oracle.window(7, 1024).astype(np.float64)
    kn = np.kaiser(1024, 6.0)                                         # alpha*t = 6
    assert np.allclose(k, kn / np.sqrt((kn * kn).sum()), atol=2e-6)   # polynomial I0


def test_dpss_known_answer_scipy(oracle):
    from scipy.signal.windows import dpss
    v, sig = oracle.dpss(4096, 4, 2.5)
    sv, lam = dpss(4096, 2.5, 5, return_ratios=True)
    for k in range(5):
        sgn = np.sign(np.dot(v[k], sv[k]))
        assert np.abs(v[k] * sgn - sv[k]).max() < 2e-7
        assert abs(1 + sig[k] - lam[k]) < 4e-6
    assert np.allclose((v * v).sum(axis=1), 1.0, atol=1e-12)


def test_periodogram_parseval(oracle):
    # unit-power window, one-sided PSD without doubling: sum(psd) ~= A^2/4 for a sine
    n = 1024
    x = (0.5 * np.sin(2 * np.pi * 100.0 * np.arange(n) / n)).astype(np.float32)
    psd = oracle.spectrogram_fft(x, n, 0.0, oracle.WINDOWS["hanning"])
    assert abs(psd[0].sum() - 0.0625) < 1e-4


def test_mtm_is_weighted_sum_of_eigenspectra(oracle):
    n, kmax, nw = 1024, 4, 2.5
    x = synth(n, fs=8000.0, seed=9)
    v, sig = oracle.dpss(n, kmax, nw)
    want = np.zeros(n // 2 + 1)
    for j in range(kmax + 1):
        X = np.fft.rfft(v[j] * x.astype(np.float64))
        want += (X.real ** 2 + X.imag ** 2) / n / (1.0 + sig[j])      # mtm.c:212-219: sum, not mean
    got = oracle.spectrogram_mtm(x, n, 0.0, nw, kmax)[0]
    assert np.abs(got - want).max() / want.max() < 2e-6


def test_history_and_submean_semantics(oracle):
    n, ovl = 1024, 0.5
    h = oracle.hop(n, ovl)
    x = synth(6 * h, fs=8000.0, seed=3) + np.float32(0.1)
    w = oracle.window(0, n).astype(np.float64)

    def frame_psd(fr):
        X = np.fft.rfft(w * fr)
        return (X.real ** 2 + X.imag ** 2) / n
    # ZERO_FIRST: frame f = samples [f*h-(n-h), f*h+h), zeros before the stream (fft.c:98-113)
    got = oracle.spectrogram_fft(x, n, ovl, 0)
    xx = np.concatenate([np.zeros(n - h), x.astype(np.float64)])
    for f in range(6):
        assert np.abs(got[f] - frame_psd(xx[f * h:f * h + n])).max() / got[f].max() < 2e-6
    # ZERO_ALWAYS: history zeroed in every frame
    got = oracle.spectrogram_fft(x, n, ovl, 0, history_mode=1)
    for f in range(6):
        fr = np.concatenate([np.zeros(n - h), x[f * h:(f + 1) * h].astype(np.float64)])
        assert np.abs(got[f] - frame_psd(fr)).max() / got[f].max() < 2e-6
    # sub_mean: each hop loses the mean of its own new samples (fft.c:86-96)
    got = oracle.spectrogram_fft(x, n, ovl, 0, sub_mean=1)
    hops = x.astype(np.float64).reshape(6, h)
    hops = hops - hops.mean(axis=1, keepdims=True)
    xx = np.concatenate([np.zeros(n - h), hops.ravel()])
    for f in range(6):
        assert np.abs(got[f] - frame_psd(xx[f * h:f * h + n])).max() / got[f].max() < 5e-6


def test_hop_truncation(oracle):
    assert oracle.hop(1024, 0.9) == 102        # (int)(1024*(1.0-0.9f)), SURVEY 8c
    assert oracle.hop(4096, 0.75) == 1024
    assert oracle.hop(1024, 0.0) == 1024


def test_pcm_conversion(oracle):
    assert np.array_equal(oracle.pcm_u8_to_float(np.array([0, 128, 255], np.uint8)),
                          np.array([-1.0, 0.0, 127 / 128], np.float32))
    assert np.array_equal(oracle.pcm_s16_to_float(np.array([-32768, 0, 32767], np.int16)),
                          np.array([-1.0, 0.0, 32767 / 32768], np.float32))


@pytest.mark.parametrize("path", sorted(p for p in glob.glob(os.path.join(GOLD, "*.npz"))
                                        if os.path.basename(p)[:2] not in ("l_", "f_", "w_")),     # round-2 rows: test_oracle_extras.py
                         ids=os.path.basename)
def test_oracle_reproduces_golden(oracle, path):
    g = np.load(path)
    name = os.path.basename(path)
    if name.startswith("spec_"):
        assert np.array_equal(oracle.rfft_halfcomplex(g["win"] * g["x"]), g["halfcomplex"])
    elif name.startswith("avg_floor"):
        psd = g["psd"]
        fl = np.array([oracle.floor_stats(p) for p in psd], np.float64)
        assert np.array_equal(fl, g["floor"])
        for mode in ("plain", "sumextreme", "sumavg"):
            for max0 in (0, 1):
                a = oracle.Averager(1024, int(g["depth"]))
                for f in range(psd.shape[0]):
                    r, avg, peak, var = a.update(mode, psd[f], int(g["minbin"]), int(g["maxbin"]), max0=max0, n=513)
                    assert np.array_equal(avg, g["%s_max%d_avg" % (mode, max0)][f])
                    assert np.array_equal(np.array([r, peak, var]), g["%s_max%d_ret" % (mode, max0)][f], equal_nan=True)
    elif name.startswith("display_"):
        cases = {"lin_fixed_thresh": dict(palette_id=1, scale_log=False, autoscale=False, max_level_db=-25.0,
                                          min_level_db=-70.0, thr_level=20.0),
                 "log_fixed_bone": dict(palette_id=5, scale_log=True, autoscale=False, max_level_db=-20.0,
                                        min_level_db=-80.0, thr_level=5.0)}
        for cname, kw in cases.items():
            rgb, lev, levels, _ = oracle.display(g["psd"], g["stats"], **kw)
            assert np.array_equal(rgb, g[cname + "_rgb"]) and np.array_equal(lev, g[cname + "_lev"])
            assert np.array_equal(levels, g[cname + "_levels"])
        rgb, lev, levels, _ = oracle.display(g["avg"], g["stats"], palette_id=7, scale_log=True, autoscale=True,
                                             overlap=0.5)
        assert np.array_equal(rgb, g["avg_log_auto_otd_rgb"]) and np.array_equal(lev, g["avg_log_auto_otd_lev"])
    elif str(g["mode"]) == "hparma":
        got = oracle.spectrogram_hparma(g["x"], int(g["n"]), float(g["overlap"]), int(g["t"]), int(g["p_e"]))
        assert np.array_equal(got, g["psd"])
        fr = oracle.hparma_frames(g["x"], int(g["n"]), float(g["overlap"]), int(g["t"]), int(g["p_e"]))
        assert all(np.array_equal(f[1], a) and f[2] == r for f, a, r in zip(fr, g["ar"], g["rank"]))
    elif str(g["mode"]) == "fft":
        got = oracle.spectrogram_fft(g["x"], int(g["n"]), float(g["overlap"]), int(g["window"]), float(g["a"]),
                                     int(g["limiter"]), int(g["sub_mean"]), int(g["history_mode"]))
        assert np.array_equal(got, g["psd"])
        assert np.array_equal(oracle.window(int(g["window"]), int(g["n"])), g["win"])
    else:
        got = oracle.spectrogram_mtm(g["x"], int(g["n"]), float(g["overlap"]), float(g["nw"]), int(g["kmax"]),
                                     int(g["sub_mean"]), int(g["history_mode"]))
        assert np.array_equal(got, g["psd"])


def test_hparma_row0_overflow_and_ar_spectrum(oracle):
    """hparma.c:89-102: lags 0..t-1 go into row 0 of a (t+1) x (p_e+1) contiguous matrix, so rows
    i > p_e are built from already rewritten cells ("row 33 col 0 holds r(1) not r(33)").
    The restatement is checked against an independent numpy construction of that aliasing and of
    the rest of hparma_do (numpy SVD for the subspace instead of the Jacobi sweeps)."""
    n, t, p_e = 4096, 128, 32
    ncol = p_e + 1
    x = synth(n, seed=12)
    (psd, a, rank), = oracle.hparma_frames(x, n, 0.0, t, p_e)
    xd = x.astype(np.float64)
    r = np.array([np.dot(xd[i:], xd[:n - i]) / (n - i) for i in range(t)]).astype(np.float32)
    flat = np.zeros((t + 1) * ncol, np.float32)
    flat[:t] = r
    for i in range(1, t):
        for j in range(ncol):
            flat[i * ncol + j] = flat[abs(j - i)]
    M = flat[:t * ncol].reshape(t, ncol).astype(np.float64)
    assert M[33, 0] == r[1] and M[33, 0] != r[33]                     # the aliasing itself
    U, S, Vt = np.linalg.svd(M, full_matrices=False)
    nu = np.sqrt(np.cumsum(S ** 2) / np.sum(S ** 2))
    assert rank == int(np.argmax(nu > 0.995))
    V = Vt.T
    noise = V[:, rank + 1:]
    a_np = noise @ noise[0] / (noise[0] @ noise[0])                   # hparma.c:125-138: projector row 0, normalised
    assert np.abs(a.astype(np.float64) - a_np).max() < 5e-4 * np.abs(a_np).max()
    A = np.polyval(a[::-1].astype(np.float64), np.exp(-2j * np.pi * np.arange(n // 2 + 1) / n))
    inv = np.abs(A) ** 2 / n
    got_inv = np.concatenate([1.0 / psd[:n // 2].astype(np.float64), psd[n // 2:].astype(np.float64)])
    assert np.abs(got_inv - inv).max() / inv.max() < 1e-5            # the float32 FFT of the padded AR vector


def test_hparma_is_conditioned_at_1e5(oracle):
    """Why HP-ARMA parity is stated at 1e-4: perturbing every input sample by at most one float
    ulp moves the REFERENCE algorithm's own |A(f)|^2 by up to ~1e-5 (peak-normalised)."""
    n, ovl, t, p_e = 1024, 0.5, 96, 16
    x = synth(10 * 512, seed=n + t)
    rng = np.random.default_rng(0)
    x2 = (x.view(np.int32) + rng.integers(-1, 2, x.size).astype(np.int32)).view(np.float32)
    a, b = oracle.hparma_frames(x, n, ovl, t, p_e), oracle.hparma_frames(x2, n, ovl, t, p_e)
    errs = [max(rel_err(1.0 / q[0][:n // 2].astype(np.float64), 1.0 / p[0][:n // 2].astype(np.float64))) for p, q in zip(a, b)]
    assert 1e-6 < max(errs) < 1e-4, errs


# ---- display mapping (g_main.c:651-762, 1099-1236): g_main.c needs GTK and cannot be built
# here, so the restatement is pinned by known answers worked out from the reference's formulas.

def test_palette_known_answers(oracle):
    P = oracle.PALETTES
    hsv = oracle.palette(P["hsv"])
    assert hsv[0].tolist() == [0, 0, 255] and hsv[63].tolist() == [0, 252, 255]
    assert hsv[64].tolist() == [0, 255, 254] and hsv[128].tolist() == [2, 255, 0]
    assert hsv[192].tolist() == [255, 252, 0] and hsv[255].tolist() == [255, 0, 0]
    th = oracle.palette(P["thresh"])
    assert not th[:16].any() and np.array_equal(th[16:], hsv[16:])
    c = np.arange(256)
    assert np.array_equal(oracle.palette(P["bw"]), np.stack([c, c, c], 1))
    assert np.array_equal(oracle.palette(P["cool"]), np.stack([c, 255 - c, np.full(256, 255)], 1))
    hot = oracle.palette(P["hot"])
    assert hot[95].tolist() == [253, 0, 0] and hot[96].tolist() == [255, 2, 0] and hot[255].tolist() == [255, 255, 254]
    # OTD runs below zero at both ends of its ramps: 2*0-1 = -1 -> 255, 2*(128-127)-1 = 1
    otd = oracle.palette(P["otd"])
    assert otd[0].tolist() == [0, 255, 255] and otd[1].tolist() == [0, 1, 253]
    assert otd[128].tolist() == [1, 255, 0] and otd[255].tolist() == [255, 1, 0]
    # BONE's red passes 255 at c = 263 -> never; copper's red 1.23*207 = 254.61 -> 254, then 255
    cop = oracle.palette(P["copper"])
    assert cop[207].tolist() == [254, 161, 103] and cop[208].tolist() == [255, 162, 104]
    bone = oracle.palette(P["bone"])
    assert bone[255].tolist() == [246, 255, 255] and bone[96].tolist() == [85, 86, 114]
    # an unknown id is the reference's final else branch: black and white
    assert np.array_equal(oracle.palette(42), oracle.palette(P["bw"]))


def test_display_linear_fixed_levels_known_answer(oracle):
    # linear scale, fixed levels 0 dB / -10 dB -> display range [0.1, 1.0]; BW palette = v itself
    n = 64
    psd = np.linspace(0.0, 1.2, n, dtype=np.float32)[None, :]
    stats = np.zeros((1, 4), np.float32)
    rgb, lev, levels, _ = oracle.display(psd, stats, palette_id=4, scale_log=False, autoscale=False,
                                         max_level_db=0.0, min_level_db=-10.0)
    assert levels[0].tolist() == [1.0, np.float32(0.1)]
    x = psd[0, ::-1].astype(np.float32)                       # pixel i shows bin n-1-i
    f = np.float32(255) * ((x - np.float32(0.1)) / (np.float32(1.0) - np.float32(0.1)))
    want = np.where(f < 0, 0, np.where(f > 255, 255, np.trunc(f))).astype(np.uint8)
    assert np.array_equal(rgb[0, :, 0], want) and np.array_equal(rgb[0, :, 1], want)
    assert rgb[0, 0, 0] == 255 and rgb[0, -1, 0] == 0


def test_display_log_truncates_to_whole_db(oracle):
    # sig_level takes the value of the SHORT levbuf cell (g_main.c:1195): -37.6 dB shows as -37
    db = np.array([[-37.6, -0.4, -99.9, -12.5, 3.7]])
    psd = (10.0 ** (db / 10.0)).astype(np.float32)
    rgb, lev, levels, _ = oracle.display(psd, np.zeros((1, 4), np.float32), palette_id=4, scale_log=True,
                                         autoscale=False, max_level_db=0.0, min_level_db=-100.0)
    assert lev[0].tolist() == [3, -12, -99, 0, -37]            # pixel i shows bin n-1-i, truncated toward 0
    assert levels[0].tolist() == [0.0, -100.0]
    want = [255, int(np.float32(255) * np.float32(88 / 100)), int(255 * np.float32(1 / 100)), 255, int(255 * np.float32(63 / 100))]
    assert rgb[0, :, 0].tolist() == want
    # a zero bin: log10(0) = -inf -> the x86 conversion gives INT_MIN, whose low 16 bits are 0
    rgb, lev, _, _ = oracle.display(np.zeros((1, 3), np.float32), np.zeros((1, 4), np.float32), palette_id=4,
                                    scale_log=True, autoscale=False, max_level_db=0.0, min_level_db=-100.0)
    assert lev[0].tolist() == [0, 0, 0] and rgb[0, :, 0].tolist() == [255, 255, 255]


def test_display_autoscale_recurrence(oracle):
    rng = np.random.default_rng(3)
    stats = np.abs(rng.standard_normal((50, 4))).astype(np.float32) + 0.1
    stats[:, 1] *= 0.01
    psd = np.abs(rng.standard_normal((50, 17))).astype(np.float32)
    _, _, levels, st = oracle.display(psd, stats, scale_log=False, autoscale=True, overlap=0.5)
    mx = np.float32(stats[0, 0] / np.float32(0.5))             # first buffer: /= overlap
    mn = np.float32(stats[0, 1] / np.float32(0.5))
    assert levels[0].tolist() == [mx, mn]
    for f in range(1, 50):
        mx = np.float32((1.0 - 0.99) * float(stats[f, 0]) + 0.99 * float(mx))
        mn = np.float32((1.0 - 0.99) * float(stats[f, 1]) + 0.99 * float(mn))
        assert levels[f].tolist() == [mx, mn]
    assert st == (0, mx, mn)
    # state carried across calls == one long call
    _, _, l1, s1 = oracle.display(psd[:20], stats[:20], scale_log=False, autoscale=True, overlap=0.5)
    _, _, l2, s2 = oracle.display(psd[20:], stats[20:], scale_log=False, autoscale=True, overlap=0.5,
                                  first_buffer=bool(s1[0]), state=s1[1:])
    assert np.array_equal(np.vstack([l1, l2]), levels) and s2 == st


def test_display_golden(oracle):
    g = np.load(os.path.join(GOLD, "display_fft1024.npz"))
    assert np.array_equal(np.array([oracle.palette(i) for i in range(8)]), g["palettes"])
    rgb, lev, levels, _ = oracle.display(g["psd"], g["stats"], palette_id=0, scale_log=True, autoscale=True,
                                         overlap=0.5)
    assert np.array_equal(rgb, g["log_auto_hsv_rgb"]) and np.array_equal(lev, g["log_auto_hsv_lev"])
    assert np.array_equal(levels, g["log_auto_hsv_levels"])
