"""Float64 'exact-arithmetic' adaptively weighted multitaper rows of one real stream, their float32 stand-in, and the inputs the
adaptive tests share (tests only): tests/_exact.py / _iq_exact.py for Spectrogram.adaptive.

A stream is float32 values (the sample format's conversion is input preparation and exact).  Frame f holds samples
[f H - (N - H), f H + H) with the history rules of real streams.  With the plan's unit-energy tapers v_j and the float32 weights
lambda_j, beta_j the kernel gets (glfer_hip_adaptive_weights), taken as the doubles they are:

    E_j = |rfft(v_j x_f)|^2 / N          sigma2 = sum_n x_f[n]^2 / N          B_j = beta_j sigma2 / N
    S = (E_0 + E_1) / 2, then per sweep   u_j = (lambda_0 S + B_0) / (lambda_j S + B_j), u_0 = 1, 0-denominator -> 1
                                          w_j = lambda_j u_j^2      S' = sum w_j E_j / sum w_j      nu = 2 (sum w)^2 / sum w^2

The stand-in keeps the same frames and goes float32: one float32 transform per taper, torch.fft.rfft on CPU tensors row by row (as
_cross_exact._rfft32), sigma2, the weights and the sums in float32.  Its keyword arguments are the criterion test's mutations.
"""
import numpy as np

from _cross_exact import _rfft32, quantise, to_float32  # noqa: F401  (re-exported for the tests)
from _iq_exact import frames64


def frames_real(x32, n, overlap, history_mode=0):
    """The assembled frames as float64 rows of the float32 samples."""
    return frames64(np.asarray(x32, np.float32).astype(np.complex64), n, overlap, history_mode).real


def eigen64(x32, n, overlap, tapers, history_mode=0):
    """(E [frames][K][n/2+1], sigma2 [frames]) in float64."""
    fr = frames_real(x32, n, overlap, history_mode)
    E = np.empty((fr.shape[0], len(tapers), n // 2 + 1))
    for j in range(len(tapers)):
        X = np.fft.rfft(fr * tapers[j], axis=1)
        E[:, j, :] = (X.real ** 2 + X.imag ** 2) / n
    return E, np.sum(fr * fr, axis=1) / n


def start64(E):
    return 0.5 * (E[:, 0, :] + E[:, 1, :])


def sweep64(S, E, lam, beta, sigma2, n):
    """One sweep from S [frames][bins] in float64: (S', nu)."""
    lam = np.asarray(lam, np.float64)
    B = np.asarray(beta, np.float64)[None, :] * np.asarray(sigma2, np.float64)[:, None] / n      # [frames][K]
    num = lam[0] * S + B[:, 0, None]
    den = lam[None, :, None] * S[:, None, :] + B[:, :, None]
    u = np.where(den == 0.0, 1.0, num[:, None, :] / np.where(den == 0.0, 1.0, den))
    u[:, 0, :] = 1.0
    w = lam[None, :, None] * u * u
    sw = w.sum(axis=1)
    return (w * E).sum(axis=1) / sw, 2.0 * sw * sw / (w * w).sum(axis=1)


def adaptive64(E, lam, beta, sigma2, n, iters):
    S, nu = start64(E), None
    for _ in range(iters):
        S, nu = sweep64(S, E, lam, beta, sigma2, n)
    return S, nu


def fixed64(E, sig):
    """The fixed-weight row of Spectrogram.run from the eigenspectra: sum_j E_j / (1 + sig_j)."""
    return (E / (1.0 + np.asarray(sig, np.float64))[None, :, None]).sum(axis=1)


def eigen32(x32, n, overlap, tapers, history_mode=0, sig=None):
    """The stand-in's (E, sigma2) in float32.  sig: the mutation that leaves 1 / (1 + sig_j) in the eigenspectra."""
    fr = frames_real(x32, n, overlap, history_mode).astype(np.float32)            # (exact: the values are float32)
    E = np.empty((fr.shape[0], len(tapers), n // 2 + 1), np.float32)
    for j in range(len(tapers)):
        X = _rfft32(fr * np.asarray(tapers[j], np.float32))
        E[:, j, :] = (X.real * X.real + X.imag * X.imag) / np.float32(n)
        if sig is not None:
            E[:, j, :] *= np.float32(1.0 / (1.0 + sig[j]))
    s2 = np.zeros(fr.shape[0], np.float32)
    for i in range(n):                                                            # a float32 sum in a fixed order
        s2 += fr[:, i] * fr[:, i]
    return E, s2 / np.float32(n)


def sweep32(S, E, lam, beta, sigma2, n, no_over_n=False, drop_lambda=False):
    f = np.float32
    lam, beta = np.asarray(lam, f), np.asarray(beta, f)
    K = E.shape[1]
    B = [(beta[j] * sigma2) if no_over_n else (beta[j] * sigma2 / f(n)) for j in range(K)]   # [frames] each
    num = lam[0] * S + B[0][:, None]
    sw = np.full(S.shape, f(1.0) if drop_lambda else lam[0], f)
    sw2 = sw * sw
    acc = sw * E[:, 0, :]
    for j in range(1, K):
        den = lam[j] * S + B[j][:, None]
        with np.errstate(divide="ignore", invalid="ignore"):
            u = np.where(den == 0, f(1.0), num / den).astype(f)
        w = (u * u) if drop_lambda else (lam[j] * u) * u
        sw = sw + w
        sw2 = sw2 + w * w
        acc = acc + w * E[:, j, :]
    return (acc / sw).astype(f), (f(2.0) * sw * sw / sw2).astype(f)


def adaptive32(x32, n, overlap, tapers, lam, beta, iters, history_mode=0, mutate=None, sig=None, s2_stride=None):
    """The float32 stand-in after `iters` sweeps: (psd, dof, E32).  mutate: one of MUTATIONS (the criterion test).  s2_stride:
    sigma2 of the frame that many frames earlier (one_pass_earlier: the criterion test's stale carried state)."""
    f = np.float32
    E, s2 = eigen32(x32, n, overlap, tapers, history_mode, sig=sig if mutate == "sig_in_eigen" else None)
    if s2_stride is not None:
        s2 = one_pass_earlier(s2, s2_stride)
    lam, beta = np.asarray(lam, f), np.asarray(beta, f)
    if mutate == "beta_from_float_lambda":
        beta = (f(1.0) - lam).astype(f)
    if mutate == "sigma2_fresh_only":              # the mean square of the samples that are not zeroed history
        cnt = n - _zeroed(E.shape[0], n, overlap, history_mode)
        s2 = (s2 * f(n) / cnt.astype(f)).astype(f)
    S = (E[:, 0, :] if mutate == "start_e0" else f(0.5) * (E[:, 0, :] + E[:, 1, :])).astype(f)
    nsweeps = max(iters - 1, 1) if mutate == "one_sweep_short" else iters
    dofs = []
    for _ in range(nsweeps):
        S, dof = sweep32(S, E, lam, beta, s2, n, no_over_n=mutate == "b_without_n", drop_lambda=mutate == "weights_without_lambda")
        dofs.append(dof)
    return S, dofs[-2] if mutate == "dof_previous_sweep" and len(dofs) > 1 else dofs[-1], E


def _zeroed(nframes, n, overlap, history_mode):
    """Zeroed history samples per frame."""
    from _exact import hop_len
    h = hop_len(n, overlap)
    z = np.zeros(nframes)
    for fi in range(nframes):
        z[fi] = (n - h) if history_mode else max(0, (n - h) - fi * h)
    return z


MUTATIONS = ("sig_in_eigen", "b_without_n", "beta_from_float_lambda", "dof_previous_sweep", "weights_without_lambda", "start_e0",
             "one_sweep_short", "sigma2_fresh_only")

# ---- the inputs: float32 [S] in [-1, 1)
NOISE_LIKE = ("noise", "dither", "two_level")
INPUTS = NOISE_LIKE + ("line", "line_on_bin", "edge_tones", "impulses", "alternating", "dc", "silence", "silent_frame")
CARRIER_AMP = 0.7
# the weak line under the carrier, by sample format.  u8: 45 dB, not 30 -- the fixed-weight row's skirt with eight tapers stands
# 28 - 36 dB under the carrier, so a line 30 dB down is one the fixed-weight row finds too (tests/test_adaptive_criterion.py)
LINE_DB = {"f32": -80.0, "s16": -60.0, "u8": -45.0}


def carrier_bin(n):
    return n // 8 + 0.5                                   # off-bin: the worst leakage


def line_bin(n, w):
    """The weak line's bin: well outside the carrier's +-2 ceil(w) bins."""
    return n // 8 + 10 * int(np.ceil(w)) + 3


def make_input(name, n, nsamples, seed, fmt_name="f32", w=2.5, line_db=None):
    """line_db: another level for the weak line than LINE_DB's (the criterion test's record of why u8 is not at 30 dB)."""
    x = _values(name, n, nsamples, seed, fmt_name, w, line_db)
    return to_float32(quantise(np.clip(x, -0.999, 0.999).astype(np.float32), fmt_name), fmt_name)


# ---- inputs keyed to the passes of a persistent grid (tests/_grid_passes.py): `noise` or `line` times a level that changes where
# a block goes from one frame group to its next, so that sigma2 -- the state a block's lanes carry through a frame -- differs by
# 60 dB or by everything between the frame a block handles and the one it handled a pass earlier.  A sample belongs to the frame
# whose fresh hop it lies in, a frame to pass frame // stride; the pass's level is LEVEL_ORDERS[order][pass % 3].  With two
# passes: down 1 -> 1e-3, up 0 -> 1e-3, gap 1 -> 0; with three, gap has digital silence between sound and `up` / `down` end / begin
# with it.  u8 holds neither base at 1e-3 (0.2e-3 and 0.7e-3 of full scale round to the zero code): there that level IS silence.
LEVEL_ORDERS = {"down": (1.0, 1e-3, 0.0), "up": (0.0, 1e-3, 1.0), "gap": (1.0, 0.0, 1e-3)}
PASS_INPUTS = tuple("%s_%s" % (b, o) for b in ("noise", "line") for o in ("down", "up", "gap"))


def level_by_pass(name, n, hop, nsamples, seed, stride, fmt_name="f32", w=2.5, levels=None):
    """name: one of PASS_INPUTS.  levels: another level triple than LEVEL_ORDERS' (a case that drops the 1e-3 level)."""
    base, order = name.split("_")
    lv = np.asarray(LEVEL_ORDERS[order] if levels is None else levels)
    x = _values(base, n, nsamples, seed, fmt_name, w, None) * lv[((np.arange(nsamples) // hop) // stride) % 3]
    return to_float32(quantise(np.clip(x, -0.999, 0.999).astype(np.float32), fmt_name), fmt_name)


def one_pass_earlier(a, stride):
    """Per-frame state as a block that never renewed it would hold it: that of the frame stride earlier."""
    a = np.asarray(a)
    return np.concatenate([a[:stride], a[:len(a) - stride]]) if len(a) > stride else a


def _values(name, n, nsamples, seed, fmt_name, w, line_db):
    line_db = LINE_DB[fmt_name] if line_db is None else line_db
    rng = np.random.default_rng([seed, n, INPUTS.index(name)])
    t = np.arange(nsamples, dtype=np.float64)
    if name == "noise":
        x = 0.2 * rng.standard_normal(nsamples)
    elif name == "dither":                                # a few quantisation steps of an 8-bit format
        x = rng.integers(-2, 3, nsamples) / 128.0
    elif name == "two_level":                             # noise whose level steps by 40 dB in the middle of the stream
        x = 0.3 * rng.standard_normal(nsamples)
        x[nsamples // 2:] *= 0.01
    elif name == "line":                                  # an off-bin carrier and a weak line LINE_DB under it
        x = CARRIER_AMP * np.sin(2 * np.pi * carrier_bin(n) * t / n + 0.4) \
            + CARRIER_AMP * 10.0 ** (line_db / 20.0) * np.sin(2 * np.pi * line_bin(n, w) * t / n + 1.3)
    elif name == "line_on_bin":                           # both tones on their bins
        x = CARRIER_AMP * np.sin(2 * np.pi * (n // 8) * t / n + 0.4) \
            + CARRIER_AMP * 10.0 ** (line_db / 20.0) * np.sin(2 * np.pi * line_bin(n, w) * t / n + 1.3)
    elif name == "edge_tones":                            # a tone in bin 1 and one in bin N/2 - 1
        x = 0.5 * np.sin(2 * np.pi * 1 * t / n + 0.2) + 0.4 * np.sin(2 * np.pi * (n // 2 - 1) * t / n + 0.5)
    elif name == "impulses":
        x = np.zeros(nsamples)
        x[rng.integers(0, nsamples, 9)] = 0.9
        x[5] = -0.6
    elif name == "alternating":
        x = 0.5 * (1.0 - 2.0 * (np.arange(nsamples) & 1))
    elif name == "dc":
        x = np.full(nsamples, 0.375)
    elif name == "silence":
        x = np.zeros(nsamples)
    elif name == "silent_frame":                          # silence between loud stretches, longer than a frame
        x = 0.3 * rng.standard_normal(nsamples)
        x[nsamples // 3:nsamples // 3 + 2 * n + 17] = 0.0
    else:
        raise ValueError(name)
    return x
