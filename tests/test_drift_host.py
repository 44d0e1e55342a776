"""The drift search without a GPU: the symbols are exported and declared, the block count and the offsets of the C entries against
the restatement (tests/_drift_exact.py), the piece cut of the spectrogram-level entry (glfer_amd/csrc/drift_cuts.h, walked by
tests/c_drift_cuts.c as a C99 caller), the C argument rules that need no device, and the Python wrappers' refusals."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import _drift_exact as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"glfer_hip_drift_blocks": "size_t", "glfer_hip_drift_offsets": "int", "glfer_hip_drift_device": "int",
           "glfer_hip_drift_batch_device": "int", "glfer_hip_spectrogram_drift_device": "int"}
OK, E_ARG = 0, -1
ALIGN = 32                                                       # GLFER_FRAME_ALIGN


def test_drift_entries_exported(lib):
    L = lib.api.lib()
    header = open(os.path.join(ROOT, "include", "glfer_hip.h")).read()
    for name, ret in ENTRIES.items():
        assert hasattr(L, name), name
        assert name in lib.api.EXPORTS, name
        assert "%s %s(" % (ret, name) in header, name
    for name in ("drift_blocks", "drift_offsets", "drift_sums", "drift_sums_batch"):
        assert callable(getattr(lib, name, None)), name
    assert callable(lib.Spectrogram.run_drift)
    assert lib.Drift._fields == ("sums", "best", "drift")
    assert L.glfer_hip_abi_version() == 5                        # entries added: the ABI number stays
    assert "#define GLFER_HIP_ABI 5\n" in header


def test_drift_blocks(lib):
    f = lib.api.lib().glfer_hip_drift_blocks
    for T in (2, 3, 16, 17, 4096):
        for step in (1, T - 1 or 1, T, T + 3):
            assert f(0, T, step) == 0 and f(T - 1, T, step) == 0             # F < T
            assert f(T, T, step) == 1                                        # F = T
            assert f(T + step - 1, T, step) == 1 and f(T + step, T, step) == 2   # one row short of a further block, and that block
            for F in (T + 1, 3 * T, 3 * T + 5, 10 * T + step - 1):
                assert f(F, T, step) == X.blocks(F, T, step) == lib.drift_blocks(F, T, step), (F, T, step)
    assert f(100, 1, 1) == 0 and f(100, 4097, 1) == 0 and f(100, 16, 0) == 0   # outside the entries' ranges: no block
    assert lib.drift_blocks(64, 16) == 4                                     # step defaults to frames
    for bad in ((-1, 16, 1), (10, 1, 1), (10, 4097, 1), (10, 16, 0)):
        with pytest.raises(ValueError):
            lib.drift_blocks(*bad)


def _admissible(T):
    """the widest ranges T admits under the 255 cap: symmetric, and the two one-sided ones"""
    r = T - 1
    return [(-min(r, 127), min(r, 127)), (-min(r, 254), 0), (0, min(r, 254))]


@pytest.mark.parametrize("T", [2, 3, 5, 16, 17, 64, 4096])
def test_drift_offsets_equal_the_restatement(lib, T):
    f = lib.api.lib().glfer_hip_drift_offsets
    for dmin, dmax in _admissible(T):
        D = dmax - dmin + 1
        got = np.full((D, T), 12345, np.int32)
        assert f(T, dmin, dmax, got.ctypes.data) == OK
        assert f(T, dmin, dmax, None) == OK                      # the check alone
        assert np.array_equal(got, X.offsets(T, dmin, dmax)), (T, dmin, dmax)
        assert np.array_equal(got, lib.drift_offsets(T, dmin, dmax))
        # the four properties of the definition
        d = np.arange(dmin, dmax + 1)
        assert np.all(got[:, 0] == 0) and np.array_equal(got[:, T - 1], d)
        assert np.all(np.abs(np.diff(got, axis=1)) <= 1)
        if dmin == -dmax:
            assert np.array_equal(got, -got[::-1])               # o(-d, t) = -o(d, t)
    if T == 3:
        assert lib.drift_offsets(3, -1, 1).tolist() == [[0, -1, -1], [0, 0, 0], [0, 1, 1]]
    # rounded half away from zero: the nearest integer to d t / (T - 1), the larger magnitude at a tie
    for dmin, dmax in _admissible(T)[:1]:
        got = lib.drift_offsets(T, dmin, dmax).astype(np.int64)
        d, t = np.arange(dmin, dmax + 1)[:, None], np.arange(T)[None, :]
        assert np.all(np.abs(got * (T - 1) - d * t) * 2 <= T - 1)
        tie = np.abs(got * (T - 1) - d * t) * 2 == T - 1
        assert np.all(np.abs(got[tie]) * (T - 1) > np.abs(d * t)[tie])


def test_drift_offsets_refuse_what_the_definition_excludes(lib):
    f = lib.api.lib().glfer_hip_drift_offsets
    for T, dmin, dmax in ((1, 0, 0), (0, 0, 0), (4097, 0, 0), (16, -16, 0), (16, 0, 16), (16, 1, 5), (16, -5, -1), (4096, -127, 128),
                          (4096, -255, 0), (4096, 0, 255)):
        assert f(T, dmin, dmax, None) == E_ARG, (T, dmin, dmax)
    assert f(4096, -254, 0, None) == OK and f(4096, 0, 254, None) == OK and f(2, -1, 1, None) == OK


# ---- drift_cuts.h through its C99 caller
@pytest.fixture(scope="module")
def walked(tmp_path_factory):
    exe = tmp_path_factory.mktemp("drift_cuts") / "c_drift_cuts"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "glfer_amd", "csrc"),
                    os.path.join(ROOT, "tests", "c_drift_cuts.c"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-2000:])
    out = {}
    for line in r.stdout.splitlines():
        kind, *nums = line.split()
        out.setdefault(kind, []).append(tuple(int(v) for v in nums))
    return out


def test_header_arithmetic_against_the_restatement(walked):
    assert len(walked["off"]) == sum(T * (2 * T - 1) for T in (2, 3, 5, 16, 17))
    for T, d, t, o in walked["off"]:
        assert o == X.offset(T, d, t), (T, d, t)
    assert len(walked["blocks"]) > 100
    for F, T, step, n in walked["blocks"]:
        assert n == X.blocks(F, T, step), (F, T, step)
    for T, step, dmin, dmax, ok in walked["args"]:
        want = 2 <= T <= 4096 and step >= 1 and -(T - 1) <= dmin <= 0 <= dmax <= T - 1 and dmax - dmin + 1 <= 255
        assert ok == int(want), (T, step, dmin, dmax)
    assert {ok for *_, ok in walked["args"]} == {0, 1}


def test_pieces_are_whole_blocks_cover_every_block_once_and_fit_the_budget(walked):
    row_bytes = 4 * 129
    calls = {}
    for T, step, nblocks, first, budget, b0, nb, rows, lo, hi in walked["piece"]:
        calls.setdefault((T, step, nblocks, first, budget), []).append((b0, nb, rows, lo, hi))
    assert len(calls) > 60
    many = lone = 0
    for (T, step, nblocks, first, budget), pieces in calls.items():
        end = first + (nblocks - 1) * step + T
        at = 0
        for b0, nb, rows, lo, hi in pieces:
            assert b0 == at and nb >= 1                          # whole blocks, in order, none twice
            at += nb
            a, e = first + b0 * step, first + (b0 + nb - 1) * step + T
            # the rows computed for the piece: from the frame grid at or below its first frame to the grid at or above its last,
            # inside the call's frames -- its own rows are among them, and they are what was counted against the budget
            assert lo == max(first, a // ALIGN * ALIGN) and hi == min(end, -(-e // ALIGN) * ALIGN)
            assert lo <= a and e <= hi and hi - lo <= rows == (nb - 1) * step + T + 2 * (ALIGN - 1)
            if nb > 1:
                assert rows * row_bytes <= budget, (T, step, nblocks, budget, nb)
            else:
                lone += rows * row_bytes > budget
            # as large as the budget allows: one more block would not fit (or there is none left)
            if b0 + nb < nblocks:
                assert (rows + step) * row_bytes > budget
        assert at == nblocks                                      # every block once
        many += len(pieces) >= 3
    assert many >= 20 and lone >= 6                               # budgets below one block's rows: lone blocks go all the same


# ---- the C argument rules that need no device
def test_drift_argument_rules_without_a_device(lib):
    L = lib.api.lib()
    one, batch, spec = L.glfer_hip_drift_device, L.glfer_hip_drift_batch_device, L.glfer_hip_spectrogram_drift_device
    p = 4096                                                     # any non-NULL value: nothing below reaches a device

    def one_(rows, nrows, bins, pitch, T, step, nb, dmin, dmax, s, b, d):
        return one(rows, nrows, bins, pitch, T, step, nb, dmin, dmax, s, b, d, None)

    def batch_(rows, ns, stride, nrows, bins, pitch, T, step, nb, dmin, dmax, s, ss, b, bs, d, ds):
        return batch(rows, ns, stride, nrows, bins, pitch, T, step, nb, dmin, dmax, s, ss, b, bs, d, ds, None)

    # (1) frames, step, dmin, dmax, bins, pitch come first, before "nothing to do"
    shapes = [(1, 1, 0, 0, 65, 65), (4097, 1, 0, 0, 65, 65), (16, 0, -15, 15, 65, 65), (16, 16, -16, 15, 65, 65), (16, 16, -15, 16, 65, 65),
              (16, 16, 1, 15, 65, 65), (16, 16, -15, -1, 65, 65), (4096, 1, -128, 127, 65, 65), (16, 16, -15, 15, 0, 65),
              (16, 16, -15, 15, -3, 65), (16, 16, -15, 15, 65, 64), (16, 16, -15, 15, (1 << 31) - 1023, 1 << 31)]   # (bins past what the kernel's int indices hold)
    for T, step, dmin, dmax, bins, pitch in shapes:
        assert one_(None, 0, bins, pitch, T, step, 0, dmin, dmax, None, None, None) == E_ARG, (T, step, dmin, dmax, bins, pitch)
        assert one_(p, 64, bins, pitch, T, step, 1, dmin, dmax, p, p, p) == E_ARG
        assert batch_(None, 0, 0, 0, bins, pitch, T, step, 0, dmin, dmax, None, 0, None, 0, None, 0) == E_ARG
        assert batch_(p, 2, 1 << 20, 64, bins, pitch, T, step, 1, dmin, dmax, p, 1 << 20, p, 1 << 20, p, 1 << 20) == E_ARG
    assert spec(None, None, 0, 0, 16, 16, 0, -15, 15, None, None, None, None) == E_ARG       # no plan: no row shape
    # (2) no block, no stream: OK whatever the pointers
    assert one_(None, 0, 65, 65, 16, 16, 0, -15, 15, None, None, None) == OK
    assert one_(None, 15, 65, 70, 16, 1, 0, 0, 0, None, None, None) == OK
    assert batch_(None, 0, 0, 64, 65, 65, 16, 16, 4, -15, 15, None, 0, None, 0, None, 0) == OK
    assert batch_(None, 3, 0, 64, 65, 65, 16, 16, 0, -15, 15, None, 0, None, 0, None, 0) == OK
    # (3) NULL rows, all outputs NULL
    assert one_(None, 64, 65, 65, 16, 16, 4, -15, 15, p, p, p) == E_ARG
    assert one_(p, 64, 65, 65, 16, 16, 4, -15, 15, None, None, None) == E_ARG
    assert batch_(None, 2, 64 * 65, 64, 65, 65, 16, 16, 4, -15, 15, p, 4 * 31 * 65, p, 4 * 65, p, 4 * 65) == E_ARG
    assert batch_(p, 2, 64 * 65, 64, 65, 65, 16, 16, 4, -15, 15, None, 4 * 31 * 65, None, 4 * 65, None, 4 * 65) == E_ARG
    # more blocks than the rows hold
    assert one_(p, 64, 65, 65, 16, 16, 5, -15, 15, p, p, p) == E_ARG
    assert one_(p, 15, 65, 65, 16, 16, 1, -15, 15, p, p, p) == E_ARG
    assert one_(p, 16 + 18, 65, 65, 16, 19, 2, -15, 15, p, p, p) == E_ARG                     # one row short of the second block
    assert batch_(p, 2, 1 << 20, 64, 65, 65, 16, 1, 50, -15, 15, p, 1 << 20, p, 1 << 20, p, 1 << 20) == E_ARG
    # strides shorter than a stream's rows or outputs (pitched rows: the last row ends with its bins)
    held = 63 * 70 + 65
    good = (4 * 31 * 65, 4 * 65, 4 * 65)
    for stride, ss, bs, ds in ((held - 1, *good), (held, good[0] - 1, good[1], good[2]), (held, good[0], good[1] - 1, good[2]),
                               (held, good[0], good[1], good[2] - 1)):
        assert batch_(p, 2, stride, 64, 65, 70, 16, 16, 4, -15, 15, p, ss, p, bs, p, ds) == E_ARG, (stride, ss, bs, ds)
    assert batch_(p, 2, held, 64, 65, 70, 16, 16, 4, -15, 15, None, 0, p, 4 * 65 - 1, None, 0) == E_ARG
    # sizes that overflow size_t
    assert batch_(p, 2, 1 << 62, 64, 65, 65, 16, 16, 4, -15, 15, p, 1 << 20, p, 1 << 20, p, 1 << 20) == E_ARG
    assert batch_(p, 2, 1 << 20, 64, 65, 65, 16, 16, 4, -15, 15, p, 1 << 62, p, 1 << 20, p, 1 << 20) == E_ARG
    assert one_(p, 1 << 62, 65, 65, 16, 16, 4, -15, 15, p, p, p) == E_ARG                     # the rows' bytes
    assert one_(p, 1 << 40, 1 << 20, 1 << 20, 16, 1, 1 << 39, -15, 15, p, p, p) == E_ARG      # the sums' bytes
    assert one_(p, 64, 65, 1 << 62, 16, 16, 1, -15, 15, p, p, p) == E_ARG                     # a pitch no row stride holds


def test_drift_wrappers_refuse_bad_arguments(lib):
    import torch
    cpu = torch.zeros((64, 65), dtype=torch.float32)
    for fn, rows in ((lib.drift_sums, cpu), (lib.drift_sums_batch, cpu.view(2, 32, 65))):
        with pytest.raises(ValueError, match="GPU"):
            fn(rows, 16)
        with pytest.raises(ValueError, match="float32"):
            fn(rows.double(), 16)
        with pytest.raises(ValueError, match="-D"):
            fn(rows.reshape(-1), 16)
    with pytest.raises(ValueError, match="adjacent"):
        lib.drift_sums(torch.zeros((65, 64), dtype=torch.float32).t(), 16)
    with pytest.raises(ValueError, match="apart"):
        lib.drift_sums(torch.zeros((1, 65), dtype=torch.float32).expand(64, 65), 16)
    # frames, step and the drift range
    A = lib.api._drift_args
    assert A(16, None, None, None) == (16, 16, -15, 15) and A(4096, 7, None, None) == (4096, 7, -127, 127)
    assert A(16, 1, 0, None) == (16, 1, 0, 15) and A(300, 300, -254, 0) == (300, 300, -254, 0)
    for T in (1, 0, 4097):
        with pytest.raises(ValueError, match="frames"):
            A(T, None, None, None)
    with pytest.raises(ValueError, match="step"):
        A(16, 0, None, None)
    for dmin, dmax in ((-16, 0), (0, 16), (1, 5), (-5, -1)):
        with pytest.raises(ValueError, match="dmin"):
            A(16, 16, dmin, dmax)
    with pytest.raises(ValueError, match="255"):
        A(4096, 1, -128, 127)
    with pytest.raises(ValueError, match="want"):
        lib.api._drift_outs((), None, (), 1, 3, 5, "cpu")
    with pytest.raises(ValueError, match="want"):
        lib.api._drift_outs(("best", "psd"), None, (), 1, 3, 5, "cpu")
    with pytest.raises(ValueError, match="out"):
        lib.api._drift_outs(("best",), {"best": cpu}, (), 1, 3, 5, "cpu")
    with pytest.raises(ValueError):
        lib.drift_offsets(16, -16, 0)
