"""The drift search restated in numpy (include/glfer_hip.h, "Drift search"): the offsets, the sums in float32 in the fixed order,
the sums in float64, and best / drift by the scan 0, +1, -1, +2, -2, ... that replaces on strict >.

Rows are a 2-D array [F][pitch], pitch >= bins; only a row's first `bins` values are data.  Everything here is the definition;
`drift_sums` takes the pieces a wrong kernel would get wrong as arguments (tests/test_drift_criterion.py passes mutated ones to
show that the bit-for-bit comparison tells them apart)."""
import numpy as np


def offset(T, d, t, rounding="away"):
    """o(d, t) = sgn(d) ((2 |d| t + (T - 1)) div (2 (T - 1))): d t / (T - 1) rounded half away from zero.
    rounding "up" / "even": the same quotient rounded half up / half to even (mutations; equal to "away" off the ties)."""
    den = 2 * (T - 1)
    if rounding == "away":
        o = (2 * abs(d) * t + (T - 1)) // den
        return -o if d < 0 else o
    num = 2 * d * t                                    # d t / (T - 1) = num / den
    if rounding == "up":
        return (num + (T - 1)) // den                  # floor(x + 1/2)
    assert rounding == "even"
    q, r = divmod(num, den)
    if 2 * r > den or (2 * r == den and q % 2 == 1):
        q += 1
    return q


def offsets(T, dmin, dmax, rounding="away"):
    """[D][T] ints"""
    return np.array([[offset(T, d, t, rounding) for t in range(T)] for d in range(dmin, dmax + 1)], dtype=np.int64).reshape(dmax - dmin + 1, T)


def blocks(F, T, step):
    return 0 if F < T else (F - T) // step + 1


def drift_sums(rows, bins, T, step, dmin, dmax, dtype=np.float32, offs=None, downward=False, late=0, terms=None, outside="zero"):
    """sums[b][d - dmin][k] = sum over t = 0 .. T - 1, in that order, in `dtype` from +0.0, of rows[b step + t][k + o(d, t)]; a bin
    outside [0, bins) contributes nothing.
    The mutations: offs (another [D][T] table), downward (t from T - 1 to 0), late (the block starts that many rows later, where
    the rows reach), terms (only the first `terms` frames), outside="flat" (a bin outside the row reads what lies there in
    memory, the padding or the neighbouring row, where that is inside the array)."""
    rows = np.asarray(rows)
    F, pitch = rows.shape
    D = dmax - dmin + 1
    offs = offsets(T, dmin, dmax) if offs is None else offs
    nb = blocks(F, T, step)
    out = np.zeros((nb, D, bins), dtype=dtype)
    flat = rows.reshape(-1)
    k = np.arange(bins)
    order = range(T if terms is None else terms)
    order = list(reversed(order)) if downward else list(order)
    for b in range(nb):
        r0 = b * step + late
        if r0 + T > F:
            r0 = b * step
        acc = np.zeros((D, bins), dtype=dtype)
        for t in order:
            col = k[None, :] + offs[:, t][:, None]                         # [D][bins]
            inside = (col >= 0) & (col < bins)
            if outside == "zero":
                vals = np.where(inside, rows[r0 + t][np.clip(col, 0, bins - 1)], 0)
            else:
                at = (r0 + t) * pitch + col
                ok = (at >= 0) & (at < flat.size)
                vals = np.where(ok, flat[np.clip(at, 0, flat.size - 1)], 0)
            with np.errstate(invalid="ignore", over="ignore"):
                acc = acc + vals.astype(dtype)
        out[b] = acc
    return out


def scan_order(dmin, dmax, neg_first=False):
    """0, +1, -1, +2, -2, ... inside [dmin, dmax] (neg_first: the mutation -1, +1, -2, +2)"""
    order = [0]
    for a in range(1, max(-dmin, dmax) + 1):
        pair = (-a, a) if neg_first else (a, -a)
        order += [d for d in pair if dmin <= d <= dmax]
    return order


def best_drift(sums, dmin, order=None):
    """(best [nb][bins] of sums' dtype, drift [nb][bins] int16): a scan in `order` (default: scan_order) that replaces on strict >.
    order = range(dmin, dmax + 1) is the mutation "ties to the lowest index"."""
    nb, D, bins = sums.shape
    order = scan_order(dmin, dmin + D - 1) if order is None else list(order)
    best = sums[:, order[0] - dmin, :].copy()
    drift = np.full((nb, bins), order[0], dtype=np.int16)
    with np.errstate(invalid="ignore"):
        for d in order[1:]:
            s = sums[:, d - dmin, :]
            m = s > best
            best = np.where(m, s, best)
            drift = np.where(m, np.int16(d), drift)
    return best, drift


def drift_all(rows, bins, T, step, dmin, dmax, dtype=np.float32):
    s = drift_sums(rows, bins, T, step, dmin, dmax, dtype)
    return (s,) + best_drift(s, dmin)


def same_bits(a, b):
    """equal bit for bit, NaN results compared as NaN"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != "f":
        return bool(np.array_equal(a, b))
    na, nb = np.isnan(a), np.isnan(b)
    ui = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(ui)[~na], b.view(ui)[~nb]))
