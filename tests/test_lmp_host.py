"""The LMP statistic's three per-column entries without a GPU: the symbols are exported, the C argument rules that need no
device, the Python wrappers' refusals, and the ragged launcher's block table (glfer_amd/csrc/lmp_groups.h, walked by
tests/c_lmp_groups.c as a C99 caller) against a restatement of its definition."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("glfer_hip_lmp_device", "glfer_hip_lmp_batch_device", "glfer_hip_lmp_ragged_device")
OK, E_ARG = 0, -1


def test_lmp_entries_exported(lib):
    L = lib.api.lib()
    for name in ENTRIES:
        assert hasattr(L, name), name
        assert name in lib.api.EXPORTS, name
    for name in ("lmp_statistic", "lmp_statistic_batch", "lmp_statistic_ragged"):
        assert callable(getattr(lib, name, None)), name
    assert L.glfer_hip_abi_version() == 5                        # entries added: the ABI number stays
    header = open(os.path.join(ROOT, "include", "glfer_hip.h")).read()
    for name in ENTRIES:
        assert "int %s(" % name in header, name


def test_lmp_argument_rules_without_a_device(lib):
    L = lib.api.lib()
    one, batch, ragged = L.glfer_hip_lmp_device, L.glfer_hip_lmp_batch_device, L.glfer_hip_lmp_ragged_device
    p = 4096                                                     # any non-NULL value: nothing below reaches a device
    # the ring size and the row length come first, before "nothing to do"
    for av in (0, -1, 4097):
        assert one(p, 0, 0, 0, 129, av, p, None) == E_ARG
        assert batch(p, 0, 0, 0, 0, 0, 129, av, p, 0, None) == E_ARG
        assert ragged(p, 0, None, 129, av, p, None) == E_ARG
    for bins in (0, -5):
        assert one(p, 0, 0, 0, bins, 4, p, None) == E_ARG
        assert batch(p, 0, 0, 0, 0, 0, bins, 4, p, 0, None) == E_ARG
        assert ragged(p, 0, None, bins, 4, p, None) == E_ARG
    # zero frames, zero streams: OK, whatever the pointers
    assert one(None, 0, 0, 0, 129, 4, None, None) == OK
    assert one(None, 0, 0, 0, 129, 1, None, None) == OK and one(None, 0, 0, 0, 129, 4096, None, None) == OK
    assert batch(None, 0, 0, 0, 0, 7, 129, 4, None, 0, None) == OK
    assert batch(None, 3, 0, 0, 0, 0, 129, 4, None, 0, None) == OK
    assert ragged(None, 0, None, 129, 4, None, None) == OK
    none = np.zeros(4, np.uint64)
    assert ragged(None, 3, none.ctypes.data, 129, 4, None, None) == OK          # three streams without rows
    flat = np.full(4, 17, np.uint64)
    assert ragged(None, 3, flat.ctypes.data, 129, 4, None, None) == OK
    # NULL pointers with work to do
    assert one(None, 0, 0, 5, 129, 4, p, None) == E_ARG and one(p, 0, 0, 5, 129, 4, None, None) == E_ARG
    assert batch(None, 2, 5 * 129, 0, 0, 5, 129, 4, p, 5 * 129, None) == E_ARG
    assert batch(p, 2, 5 * 129, 0, 0, 5, 129, 4, None, 5 * 129, None) == E_ARG
    good = np.array([0, 3, 3, 8], np.uint64)
    assert ragged(p, 3, None, 129, 4, p, None) == E_ARG
    assert ragged(None, 3, good.ctypes.data, 129, 4, p, None) == E_ARG and ragged(p, 3, good.ctypes.data, 129, 4, None, None) == E_ARG
    # rows that do not reach back min(lmp_av - 1, first) frames
    for av, first, row_first in ((4, 10, 8), (4, 2, 1), (8, 7, 1), (2, 1, 1), (4, 3, 4), (3, 100, 99)):
        assert one(p, row_first, first, 5, 129, av, p, None) == E_ARG, (av, first, row_first)
        assert batch(p, 2, 1 << 20, row_first, first, 5, 129, av, p, 1 << 20, None) == E_ARG, (av, first, row_first)
    # strides shorter than a stream's rows or outputs; too many frames
    assert batch(p, 2, 7 * 129, 7, 10, 5, 129, 4, p, 5 * 129, None) == E_ARG    # holds 8 rows a stream
    assert batch(p, 2, 8 * 129, 7, 10, 5, 129, 4, p, 5 * 129 - 1, None) == E_ARG
    assert one(p, 0, 0, 1 << 31, 129, 4, p, None) == E_ARG
    assert batch(p, 2, 1 << 62, 0, 0, 5, 129, 4, p, 1 << 62, None) == E_ARG     # overflows
    # the ragged table: decreasing, a stream over 2^31 - 1 rows, rows that overflow
    down = np.array([0, 5, 3, 8], np.uint64)
    assert ragged(p, 3, down.ctypes.data, 129, 4, p, None) == E_ARG
    long_ = np.array([0, 1 << 31], np.uint64)
    assert ragged(p, 1, long_.ctypes.data, 129, 4, p, None) == E_ARG
    most = np.array([5, 5 + (1 << 31) - 1], np.uint64)
    assert ragged(None, 1, most.ctypes.data, 129, 4, None, None) == E_ARG       # 2^31 - 1 rows pass the table and meet the NULL rows
    huge = np.array([0, 1 << 62], np.uint64)
    assert ragged(p, 1, huge.ctypes.data, 129, 4, p, None) == E_ARG


def test_lmp_wrappers_refuse_bad_arguments(lib):
    import torch
    cpu = torch.zeros((8, 65), dtype=torch.float32)
    for fn, rows in ((lib.lmp_statistic, cpu), (lib.lmp_statistic_batch, cpu.view(2, 4, 65))):
        with pytest.raises(ValueError, match="GPU"):
            fn(rows, 4)
        with pytest.raises(ValueError, match="float32"):
            fn(rows.double(), 4)
        with pytest.raises(ValueError, match="-D"):
            fn(rows.reshape(-1), 4)
        for av in (0, 4097):
            with pytest.raises(ValueError, match="avg"):
                fn(rows, av)
        with pytest.raises(ValueError, match="lead"):
            fn(rows, 4, first_frame=5, lead=2)                   # the ring reaches back three frames
        with pytest.raises(ValueError, match="lead"):
            fn(rows, 4, first_frame=2, lead=1)
        with pytest.raises(ValueError, match="first_frame"):
            fn(rows, 4, first_frame=2, lead=3)
        with pytest.raises(ValueError, match="at least"):
            fn(rows[..., :2, :], 4, first_frame=9, lead=3)       # fewer rows than the lead
    with pytest.raises(ValueError, match="GPU"):
        lib.lmp_statistic_ragged(cpu, [0, 3, 8], 4)
    with pytest.raises(ValueError, match="row_starts"):
        lib.lmp_statistic_ragged(cpu, [0, 5, 3, 8], 4)
    with pytest.raises(ValueError, match="row_starts"):
        lib.lmp_statistic_ragged(cpu, [0, 3, 9], 4)
    with pytest.raises(ValueError, match="avg"):
        lib.lmp_statistic_ragged(cpu, [0, 3, 8], 0)
    with pytest.raises(ValueError, match="float32"):
        lib.lmp_statistic_ragged(cpu.double(), [0, 3, 8], 4)


# ---- the block table of the ragged launcher
def _form_and_group(nl):
    """glfer_launch_lmp's rule by ring size: registers for 2, 3, 4, 8 (groups of whole turns of the ring), LDS for the other
    sizes up to 64 (groups of 64), else frame by frame"""
    if nl in (2, 3, 4, 8):
        return 1, 15 if nl == 3 else 16
    return (2, 64) if 1 < nl <= 64 else (0, 1)


def _table(lengths, G, piece_blocks):
    """the definition: a stream with frames owns ceil(frames / G) consecutive blocks of the flat list, in stream order; a piece
    is closed when the next stream would take it past piece_blocks; blk0 counts from the piece's first block"""
    entries, piece, used, row = [], -1, 0, 0
    for b, n in enumerate(lengths):
        if n > 0:
            blocks = -(-n // G)
            if piece < 0 or used + blocks > piece_blocks:
                piece, used = piece + 1, 0
            entries.append((b, row, n, used, piece))
            used += blocks
        row += n
    return entries, piece + 1


def _cases():
    cases = []
    rng = np.random.default_rng(5)
    for nl in (1, 2, 3, 4, 7, 8, 16, 64, 65, 4096):
        G = _form_and_group(nl)[1]
        pool = [0, 1, max(nl - 1, 0), max(G - 1, 0), G, G + 1, 3 * G + 2]
        cases.append((nl, 0x7fffffff, pool))                                       # every length once, in order
        cases.append((nl, 0x7fffffff, [0, 0] + pool[1:] + [0, 0]))                 # empty streams first, last and adjacent
        cases.append((nl, 0x7fffffff, [0, 5, 0, 0, G, 0, 1, 0]))
        cases.append((nl, 0x7fffffff, [0, 0, 0]))                                  # nothing but empty streams
        for _ in range(4):
            cases.append((nl, 0x7fffffff, [int(v) for v in rng.choice(pool, size=int(rng.integers(1, 12)))]))
        # a piece limit small enough to be crossed: seven blocks a piece
        cases.append((nl, 7, [3 * G + 2, 0, G, G + 1, 3 * G + 2, 1, 0, 2 * G, 4 * G, 1]))
    # the real limit, crossed by streams of the most frames a stream may have (frame by frame: a block a frame)
    cases.append((1, 0x7fffffff, [0x7fffffff, 1, 0, 0x7ffffffe, 1, 1]))
    cases.append((4, 0x7fffffff, [0x7fffffff] * 17 + [5]))                         # 2^27 blocks each: fifteen to a piece, the sixteenth would pass the limit by one block
    return cases


@pytest.fixture(scope="module")
def walked(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("lmp_groups")
    exe = tmp / "c_lmp_groups"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "glfer_amd", "csrc"),
                    os.path.join(ROOT, "tests", "c_lmp_groups.c"), "-o", str(exe)], check=True)
    cases = _cases()
    text = "".join("%d %d %d %s\n" % (nl, limit, len(lens), " ".join(str(v) for v in np.concatenate([[0], np.cumsum(lens, dtype=np.int64)])))
                   for nl, limit, lens in cases)
    r = subprocess.run([str(exe)], input=text, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-2000:])
    out, cur = [], None
    for line in r.stdout.splitlines():
        kind, *nums = line.split()
        if kind == "case":
            cur = (tuple(int(v) for v in nums), [])
            out.append(cur)
        else:
            cur[1].append(tuple(int(v) for v in nums))
    assert len(out) == len(cases)
    return list(zip(cases, out))


def test_ragged_table_against_its_definition(walked):
    crossed = 0
    for (nl, limit, lens), ((G, form, n, pieces), entries) in walked:
        assert (form, G) == _form_and_group(nl), nl
        want, want_pieces = _table(lens, G, limit)
        assert n == len(want) == len(entries) == sum(1 for v in lens if v > 0), (nl, lens)   # streams without frames get no entry
        assert pieces == want_pieces, (nl, limit, lens)
        assert entries == want, (nl, limit, lens)
        crossed += pieces > 1
        # what the kernels rely on: within a piece blk0 starts at 0 and is strictly increasing, an entry's blocks end where the
        # next one's begin, and no piece holds more blocks than the limit
        for pc in range(pieces):
            mine = [e for e in entries if e[4] == pc]
            assert mine and mine[0][3] == 0
            for a, b in zip(mine, mine[1:]):
                assert b[3] == a[3] + -(-a[2] // G) > a[3]
            assert mine[-1][3] + -(-mine[-1][2] // G) <= limit
    assert crossed >= 10                                        # the synthetic limit per ring size, and the real one twice


def test_a_stream_shorter_than_a_group_or_the_ring_is_one_short_group(walked):
    for (nl, limit, lens), ((G, form, n, pieces), entries) in walked:
        for stream, row0, nframes, blk0, piece in entries:
            assert row0 == sum(lens[:stream]) and nframes == lens[stream]
            if nframes <= G:
                nxt = [e for e in entries if e[4] == piece and e[3] > blk0]
                assert not nxt or min(e[3] for e in nxt) == blk0 + 1
