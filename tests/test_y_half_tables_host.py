"""The register-resident half tables of the five-taper N = 4096 multitaper kernel (spectro16y.hip), on the host:
the lane -> residue map, and that half table + mirror rule give back the plan's full tables bit for bit."""
import numpy as np
import pytest

N, T, HALF_FLOATS = 4096, 256, 40


def residue(t):
    j, p = t >> 4, t & 15
    return 8 * j + p if p < 8 else 240 - 8 * j + p


def tables(lib, nw):
    L = lib.api.lib()
    half = np.full((T, HALF_FLOATS), np.nan, np.float32)
    pairs = np.zeros((2, 8, T, 4), np.float32)
    last = np.zeros((4, T, 4), np.float32)
    rc = L.glfer_hip_y_half_tables(N, 4, nw, half.ctypes.data, pairs.ctypes.data, last.ctypes.data)
    assert rc in (0, 1), rc
    # full[k][i]: taper k at sample i of the frame, as the full-table form reads it (sample t + 256 m: lane t, register m)
    full = np.zeros((5, N), np.float32)
    for m in range(16):
        for k in range(4):
            full[k, T * m:T * (m + 1)] = pairs[k // 2, m // 2, :, 2 * (m & 1) + (k & 1)]
        full[4, T * m:T * (m + 1)] = last[m // 4, :, m & 3]
    return rc, half, full


def test_lane_map_pairs_mirrored_residues_in_one_dpp_row():
    r = np.array([residue(t) for t in range(T)])
    assert sorted(r) == list(range(T))                      # a permutation of the residues
    for t in range(T):
        assert residue(t ^ 15) == 255 - residue(t)          # the row_mirror partner (same 16-lane row) holds the mirror residue
        assert (t ^ 15) >> 4 == t >> 4
    # a wavefront's sample load covers two ascending runs of 32 residues
    for w in range(4):
        rw = r[64 * w:64 * (w + 1)]
        assert sorted(rw) == list(range(32 * w, 32 * w + 32)) + list(range(224 - 32 * w, 256 - 32 * w))
    # exchange 0, row layout: a 16-lane ds_write_b64 group's columns fall on 16 distinct bank pairs (of 32)
    for j in range(16):
        assert len({int(c) % 32 for c in r[16 * j:16 * j + 16]}) == 16


def test_half_table_and_mirror_rule_rebuild_the_full_tables_bit_for_bit(lib):
    rc, half, full = tables(lib, 2.5)                       # C3's tapers
    assert rc == 1
    assert not np.isnan(half).any()
    bits = lambda a: np.asarray(a, np.float32).view(np.uint32)
    for k in range(5):
        sign = np.float32(-1.0 if k & 1 else 1.0)
        col = lambda m: 32 + m if k == 4 else 16 * (k // 2) + 2 * m + (k & 1)
        for t in range(T):
            r, partner = residue(t), t ^ 15
            for m in range(16):
                want = full[k, r + T * m]
                got = half[t, col(m)] if m < 8 else sign * half[partner, col(15 - m)]
                # the sign is applied as the kernel does: a negation, exact; +-0 excepted (x * +-0 is a zero either way)
                assert bits(got) == bits(want) or (got == 0.0 and want == 0.0), (k, t, m)


@pytest.mark.parametrize("nw,built", [(2.5, 1), (2.0, 1), (3.0, 1), (3.5, 0), (4.0, 0)])
def test_half_table_is_built_only_for_exactly_symmetric_float_tables(lib, nw, built):
    rc, half, full = tables(lib, nw)
    exact = all(np.array_equal(full[k, ::-1], -full[k] if k & 1 else full[k]) for k in range(5))
    assert rc == int(exact) == built
    if not rc:
        assert np.isnan(half).all()                         # left alone
    assert lib.api.lib().glfer_hip_y_half_tables(2048, 4, 2.5, half.ctypes.data, None, None) < 0
    assert lib.api.lib().glfer_hip_y_half_tables(N, 6, 2.5, half.ctypes.data, None, None) < 0
