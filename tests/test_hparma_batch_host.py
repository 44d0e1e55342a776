"""HP-ARMA rows for many streams, the part that needs no GPU: glfer_amd/csrc/hparma_frames.h -- a frame's LDS bytes, the frames a
launch keeps in flight and the flat frame list of a batch or a ragged call -- walked by tests/c_hparma_frames.c as a C99 caller
and compared with a restatement of its definition; and the psd_pitch keyword of HparmaParams."""
import bisect
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "glfer_amd", "csrc")
LIMIT = 0x7fffffff                                                # frames of one launch: the queue's ticket is 32 bits


def _lds_bytes(n, t, ncol):
    """hparma_kernel's LDS layout: the frame (with a zero tail of 128 when t <= 128) overlaid by the t x ncol matrix, then Q
    (ncol x ncol), the t lags, the ncol singular values and the ncol AR coefficients, in floats"""
    xlen = n + (128 if t <= 128 else 0)
    return 4 * (max(xlen, t * ncol) + ncol * ncol + t + 2 * ncol)


def _resident(lds):
    """a wavefront per frame, as many per CU as 160 KiB of LDS hold, 256 CUs"""
    return 256 * ((160 * 1024) // lds)


def _table(counts, piece_frames):
    """the definition: a stream with frames owns that many consecutive flat frames, in stream order; a piece is closed when the
    next stream would take it past piece_frames; g0 counts from the piece's first frame"""
    entries, piece, used = [], -1, 0
    for b, n in enumerate(counts):
        if n > 0:
            if piece < 0 or used + n > piece_frames:
                piece, used = piece + 1, 0
            entries.append((b, used, n, piece))
            used += n
    return entries, piece + 1


SHAPES = [(4096, 128, 33), (32768, 128, 33), (1024, 96, 17), (512, 64, 21), (2048, 160, 13), (32, 8, 4), (256, 128, 33), (16384, 128, 33)]


def _table_cases():
    cases = [(LIMIT, [0, 1, 5, 0, 0, 7, 1, 0]),
             (LIMIT, [0, 0, 0]),                                  # only empty streams
             (LIMIT, [0]),
             (LIMIT, [9]),                                        # one stream alone
             (LIMIT, [1])]
    rng = np.random.default_rng(11)
    pool = [0, 1, 2, 7, 1792, 1793]
    for _ in range(40):
        cases.append((LIMIT, [int(v) for v in rng.choice(pool, size=int(rng.integers(1, 13)))]))
    # a synthetic limit of ten frames a piece, crossed several times (a stream of ten fills a piece; seven and four do not share one)
    cases.append((10, [3, 0, 7, 1, 10, 0, 0, 4, 4, 4, 9, 1, 1, 0, 10, 2]))
    cases.append((10, [10] * 5))
    cases.append((10, [5, 5, 5, 5, 1]))
    for _ in range(10):
        cases.append((10, [int(v) for v in rng.integers(0, 11, size=int(rng.integers(1, 13)))]))
    # the real limit, crossed by streams of the most frames a stream may have
    cases.append((LIMIT, [LIMIT, 1, 0, LIMIT - 1, 1, 1]))
    cases.append((LIMIT, [LIMIT] * 5 + [5]))
    cases.append((LIMIT, [1 << 30, 1 << 30, 1 << 30, 0, (1 << 30) - 1, 1, 1]))
    return cases


@pytest.fixture(scope="module")
def walked(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("hparma_frames")
    exe = tmp / "c_hparma_frames"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "c_hparma_frames.c"), "-o", str(exe)],
                   check=True)
    cases = _table_cases()
    text = "".join("lds %d %d %d\n" % s for s in SHAPES)
    text += "".join("table %d %d %s\n" % (limit, len(counts), " ".join(str(v) for v in counts)) for limit, counts in cases)
    r = subprocess.run([str(exe)], input=text, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-2000:])
    lds, out, cur = [], [], None
    for line in r.stdout.splitlines():
        kind, *nums = line.split()
        nums = tuple(int(v) for v in nums)
        if kind == "lds":
            lds.append(nums)
        elif kind == "case":
            cur = (nums, [])
            out.append(cur)
        else:
            cur[1].append(nums)
    assert len(lds) == len(SHAPES) and len(out) == len(cases)
    return dict(zip(SHAPES, lds)), list(zip(cases, out))


def test_lds_bytes_and_resident_frames(walked):
    lds, _ = walked
    assert lds[(4096, 128, 33)] == (22028, 1792)                  # BASELINE config 5: seven frames a CU
    assert lds[(32768, 128, 33)][1] == 256                        # one frame a CU
    assert lds[(32768, 128, 33)][0] <= 160 * 1024
    assert lds[(1024, 96, 17)][0] == 8204                         # glfer's defaults
    for shape, (nbytes, resident) in lds.items():
        assert nbytes == _lds_bytes(*shape), shape
        assert resident == _resident(nbytes), shape


def test_frame_table_against_its_definition(walked):
    _, tables = walked
    crossed = 0
    for (limit, counts), ((n, pieces), entries) in tables:
        want, want_pieces = _table(counts, limit)
        assert n == len(entries) == len(want) == sum(1 for v in counts if v > 0), counts   # streams without frames get no entry
        assert pieces == want_pieces and entries == want, (limit, counts)
        assert pieces == (max(e[3] for e in entries) + 1 if entries else 0)
        crossed += pieces > 1
        assert [e[0] for e in entries] == sorted(e[0] for e in entries)                   # stream order
        for stream, g0, nframes, piece in entries:
            assert nframes == counts[stream]                                              # a stream is never split
        for pc in range(pieces):
            mine = [e for e in entries if e[3] == pc]
            # what the kernel relies on: g0 starts at 0 and is strictly increasing, an entry ends where the next begins, and no
            # piece goes over the limit
            assert mine and mine[0][1] == 0
            for a, b in zip(mine, mine[1:]):
                assert b[1] == a[1] + a[2] > a[1]
            total = mine[-1][1] + mine[-1][2]
            assert total <= limit
            # a piece is closed only when the next stream would not fit
            nxt = [e for e in entries if e[3] == pc + 1]
            if nxt:
                assert total + nxt[0][2] > limit
            # every flat index maps back by bisection (the kernel's: the last entry with g0 <= g) to its stream and frame
            starts = [e[1] for e in mine]
            if total <= 20000:
                probe = range(total)
                back = []
                for stream, g0, nframes, _ in mine:
                    back += [(stream, f) for f in range(nframes)]
            else:                                                # the ends of every entry, where a bisection goes wrong first
                probe, back = [], []
                for stream, g0, nframes, _ in mine:
                    for f in sorted(f for f in {0, 1, nframes // 2, nframes - 2, nframes - 1} if 0 <= f < nframes):
                        probe.append(g0 + f)
                        back.append((stream, f))
            for g, (stream, f) in zip(probe, back):
                k = bisect.bisect_right(starts, g) - 1
                assert (mine[k][0], g - mine[k][1]) == (stream, f), (counts, g)
    assert crossed >= 8                                            # the synthetic limit and the real one


def test_the_launcher_and_the_c_abi_share_the_header():
    """the LDS rule exists once: the kernel's launcher sizes its launch with the header, and plan creation refuses with it"""
    hip = open(os.path.join(CSRC, "hparma.hip")).read()
    cabi = open(os.path.join(CSRC, "plan_tables.cpp")).read()        # (plan_config_ok: plan creation's refusals)
    for text in (hip, cabi):
        assert '#include "hparma_frames.h"' in text and "glfer_hparma_lds_bytes(" in text
    assert "glfer_hparma_resident(" in hip and "glfer_hparma_frame_table(" in hip


def test_hparma_params_take_psd_pitch(lib):
    assert lib.HparmaParams().psd_pitch == 0
    assert lib.HparmaParams(n=1024, t=96, p_e=16, psd_pitch=520).psd_pitch == 520
