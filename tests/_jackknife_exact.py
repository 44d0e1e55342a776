"""The delete-one jackknife over tapers in float64, the weights it is taken over, and its float32 stand-in (tests only):
tests/_adaptive_exact.py for Spectrogram.jackknife.

For a frame and a bin, with E_j the eigenspectra (j = 0 .. K-1), w_j the final weights and S = sum w_j E_j / sum w_j:

    S_(i)  = sum_{j != i} w_j E_j / sum_{j != i} w_j        weights held fixed, summed in the order j = 0, 1, ... without i
    l_i    = ln(S_(i) / S)          lbar = mean_i l_i          logvar = ((K-1)/K) sum_i (l_i - lbar)^2

S == 0 gives 0; S > 0 with some S_(i) == 0 gives +inf; no value is NaN.  The weights: the adaptive ones of the sweep from a given S
(weights64: _adaptive_exact.sweep64's, returned), or the float32 lambda_j taken as doubles (iters = 0).

The stand-in keeps _adaptive_exact's float32 eigenspectra and sweeps (eigen32, sweep32) and forms the weights of the last sweep and
the statistic in float32, operation for operation as the kernel does.  Its `mutate` argument is the criterion test's mutations.
"""
import numpy as np

from _adaptive_exact import eigen32, one_pass_earlier, sweep32

MUTATIONS = ("factor_dropped", "factor_one_over_k", "about_ln_s", "weights_recomputed", "previous_sweep_weights", "equal_weights",
             "zero_partner_counted", "total_minus_term")


def weights64(S, E, lam, beta, sigma2, n):
    """The weights of one sweep from S [frames][bins] in float64, [frames][K][bins]: what sweep64 forms its mean with."""
    lam = np.asarray(lam, np.float64)
    B = np.asarray(beta, np.float64)[None, :] * np.asarray(sigma2, np.float64)[:, None] / n
    S = np.asarray(S, np.float64)
    num = lam[0] * S + B[:, 0, None]
    den = lam[None, :, None] * S[:, None, :] + B[:, :, None]
    u = np.where(den == 0.0, 1.0, num[:, None, :] / np.where(den == 0.0, 1.0, den))
    u[:, 0, :] = 1.0
    return lam[None, :, None] * u * u


def lambda_weights(lam, shape):
    """iters = 0: w_j = lambda_j, the float32 values as doubles, broadcast to [frames][K][bins]."""
    return np.broadcast_to(np.asarray(lam, np.float32).astype(np.float64)[None, :, None], shape)


def delete_one64(E, w):
    """(S, S_(i) [frames][K][bins]) in float64; a delete-one estimate whose terms are all 0 is 0."""
    E = np.asarray(E, np.float64)
    w = np.broadcast_to(np.asarray(w, np.float64), E.shape)
    K = E.shape[1]
    S = (w * E).sum(axis=1) / w.sum(axis=1)
    Si = np.empty_like(E)
    for i in range(K):
        keep = [j for j in range(K) if j != i]
        num, den = (w[:, keep] * E[:, keep]).sum(axis=1), w[:, keep].sum(axis=1)
        Si[:, i] = np.where(num == 0.0, 0.0, num / np.where(num == 0.0, 1.0, den))
    return S, Si


def jackknife64(E, w):
    """(S, logvar, min_i S_(i)) in float64, the degenerate cases decided as the kernel decides them."""
    S, Si = delete_one64(E, w)
    K = Si.shape[1]
    ok = (S > 0)[:, None, :] & (Si > 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        l = np.where(ok, np.log(np.where(ok, Si, 1.0) / np.where(S > 0, S, 1.0)[:, None, :]), 0.0)
    d = l - l.mean(axis=1, keepdims=True)
    lv = (K - 1.0) / K * (d * d).sum(axis=1)
    lv = np.where((Si == 0).any(axis=1) | ~np.isfinite(lv), np.inf, lv)
    lv = np.where(S == 0, 0.0, lv)
    return S, lv, Si.min(axis=1)


def _weights32(S, E, lam, beta, sigma2, n):
    """The weights of the sweep from S in float32, a list of K arrays [frames][bins]: sweep32's arithmetic."""
    f = np.float32
    K = E.shape[1]
    B = [(beta[j] * sigma2 / f(n)) for j in range(K)]
    num = lam[0] * S + B[0][:, None]
    w = [np.full(S.shape, lam[0], f)]
    for j in range(1, K):
        den = lam[j] * S + B[j][:, None]
        with np.errstate(divide="ignore", invalid="ignore"):
            u = np.where(den == 0, f(1.0), num / den).astype(f)
        w.append(((lam[j] * u) * u).astype(f))
    return w


def _mean32(w, E):
    f = np.float32
    sw, sw2, acc = w[0].copy(), w[0] * w[0], w[0] * E[:, 0, :]
    for j in range(1, len(w)):
        sw = sw + w[j]
        sw2 = sw2 + w[j] * w[j]
        acc = acc + w[j] * E[:, j, :]
    with np.errstate(divide="ignore", invalid="ignore"):
        return (acc / sw).astype(f), (f(2.0) * sw * sw / sw2).astype(f), acc, sw


def jackknife32(x32, n, overlap, tapers, lam, beta, iters, history_mode=0, mutate=None, s2_stride=None):
    """The float32 stand-in: (psd, dof, logvar, E32).  iters = 0: w_j = lambda_j.  mutate: one of MUTATIONS.  s2_stride: sigma2
    of the frame that many frames earlier (_adaptive_exact.one_pass_earlier)."""
    f = np.float32
    E, s2 = eigen32(x32, n, overlap, tapers, history_mode)
    if s2_stride is not None:
        s2 = one_pass_earlier(s2, s2_stride)
    lam, beta = np.asarray(lam, f), np.asarray(beta, f)
    K = E.shape[1]
    S = (f(0.5) * (E[:, 0, :] + E[:, 1, :])).astype(f)
    prev = S
    for _ in range(max(iters - 1, 0)):
        prev = S
        S, _ = sweep32(S, E, lam, beta, s2, n)
    if iters == 0:
        w = [np.full(S.shape, lam[j], f) for j in range(K)]
    else:
        w = _weights32(S, E, lam, beta, s2, n)
    psd, dof, acc, sw = _mean32(w, E)
    wj = list(w)                                     # the weights the statistic is taken over
    if mutate == "previous_sweep_weights" and iters >= 2:
        wj = _weights32(prev, E, lam, beta, s2, n)
    if mutate == "equal_weights":
        wj = [np.ones(S.shape, f) for _ in range(K)]
    Ej = [E[:, j, :] for j in range(K)]
    if mutate == "zero_partner_counted" and K % 2:   # the zero row behind an odd K's lone taper, as a taper of its own
        Ej.append(np.zeros(S.shape, f))
        wj.append(wj[-1])
    recompute = None
    if mutate == "weights_recomputed" and iters >= 1:
        # the weights formed again from the delete-one estimate, taper i left out of them
        recompute = lambda si: _weights32(si, E, lam, beta, s2, n)  # noqa: E731
    return psd, dof, statistic32(Ej, wj, psd, mutate, recompute), E


def statistic32(Ej, wj, psd, mutate=None, recompute=None):
    """logvar in float32 from the eigenspectra Ej and the weights wj (lists of float32 arrays of one shape) and the row psd, the
    kernel's operations in its order.  mutate: the mutations of the statistic itself; recompute: weights_recomputed's hook."""
    f = np.float32
    S = psd
    Kj = len(Ej)
    ls = []
    unbounded = np.zeros(S.shape, bool)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for i in range(Kj):
            if mutate == "total_minus_term":
                tot, den = np.zeros(S.shape, f), np.zeros(S.shape, f)
                for j in range(Kj):
                    tot, den = tot + wj[j] * Ej[j], den + wj[j]
                ni, di = tot - wj[i] * Ej[i], den - wj[i]
            else:
                ni, di = np.zeros(S.shape, f), np.zeros(S.shape, f)
                for j in range(Kj):
                    if j != i:
                        ni, di = ni + wj[j] * Ej[j], di + wj[j]
            if recompute is not None:
                si = np.where(ni == 0, f(0), ni / di).astype(f)
                w2 = recompute(si)
                ni, di = np.zeros(S.shape, f), np.zeros(S.shape, f)
                for j in range(Kj):
                    if j != i:
                        ni, di = ni + w2[j] * Ej[j], di + w2[j]
            li = np.where(ni == 0, f(-np.inf), np.log(((ni / di).astype(f) / psd).astype(f))).astype(f)
            unbounded |= ~(np.abs(li) < np.inf)
            ls.append(li)
        lsum = np.zeros(S.shape, f)
        for li in ls:
            lsum = lsum + li
        lbar = np.zeros(S.shape, f) if mutate == "about_ln_s" else (lsum / f(Kj)).astype(f)
        ss = np.zeros(S.shape, f)
        for li in ls:
            ss = ss + (li - lbar) * (li - lbar)
        factor = f(1.0) if mutate == "factor_dropped" else (f(1.0) / f(Kj) if mutate == "factor_one_over_k" else (f(Kj) - f(1.0)) / f(Kj))
        lv = (factor * ss).astype(f)
    lv = np.where(unbounded | ~(lv >= 0), f(np.inf), lv)
    lv = np.where(psd == 0, f(0), lv).astype(f)
    return lv
