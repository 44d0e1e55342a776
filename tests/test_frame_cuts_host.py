"""glfer_amd/csrc/frame_cuts.h, the one statement of the launchers' frame and hop arithmetic, walked without a GPU:
tests/c_frame_cuts.c includes it as a C99 caller and prints every cut and hop span for lo in 0..40, hi in lo..lo+40,
first_inside in {0, 1, 3, 7}, G in {1, 2, 8, 16}; each line is checked here against the DEFINITION (the frame groups
enumerated one by one, the hops a frame reads listed one by one), not against the rounding formula typed a second time."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(tmp_path, name, *flags):
    exe = tmp_path / name
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", *flags, "-I", os.path.join(ROOT, "glfer_amd", "csrc"),
                    os.path.join(ROOT, "tests", "c_frame_cuts.c"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-2000:])
    return r.stdout


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    out = _run(tmp_path_factory.mktemp("frame_cuts"), "c_frame_cuts")
    rows = {}
    for line in out.splitlines():
        kind, *nums = line.split()
        rows.setdefault(kind, []).append(tuple(int(v) for v in nums))
    return rows


def test_sizes_first_inside_and_groups(lines):
    assert lines["size"] == [(0, 4), (1, 2), (2, 1)]                       # f32, s16, u8
    for keep, hop, fi in lines["inside"]:
        assert fi == min(f for f in range(keep + 1) if f * hop >= keep)     # the first frame whose history is in the stream
    # the shared-odd kernels: two sets of 256 lanes' worth of frames at 16 points a lane; every other route one frame
    assert lines["group"] == [(256, 32, 1), (512, 16, 1), (1024, 8, 1), (2048, 4, 1), (4096, 2, 1), (8192, 2, 1), (16384, 2, 1)]


def test_cuts_partition_and_the_body_is_the_union_of_whole_groups(lines):
    cuts = lines["cut"]
    assert len(cuts) == 41 * 41 * 4 * 4
    assert {c[:2] for c in cuts} == {(lo, hi) for lo in range(41) for hi in range(lo, lo + 41)}
    assert {c[2] for c in cuts} == {0, 1, 3, 7} and {c[3] for c in cuts} == {1, 2, 8, 16}
    for lo, hi, fi, G, b0, b1 in cuts:
        inside = range(max(lo, fi), hi)
        union = set()
        for k in range(hi // G + 1):
            group = range(k * G, (k + 1) * G)
            if all(f in inside for f in group):
                union |= set(group)
        # head [lo, b0), body [b0, b1), tail [b1, hi) partition [lo, hi)
        assert lo <= b0 <= b1 <= hi, (lo, hi, fi, G, b0, b1)
        assert set(range(b0, b1)) == union, (lo, hi, fi, G, b0, b1)
        if not union:
            assert b0 == b1 == hi
        # ... so the clamps the by-copy calls used to carry are identities
        assert min(b0, hi) == b0 and max(b1, min(b0, hi)) == b1


def test_copy_spans_hold_every_hop_the_frames_read(lines):
    seen = set()
    for first, nframes, back, fresh, lo, n in lines["copy"]:
        seen.add((back > 0, fresh))
        span = range(lo, lo + n)
        if nframes == 0:
            assert n == 0
            continue
        need = {h for f in range(first, first + nframes) for h in range(f - back, f + 1) if h >= 0}
        assert need <= set(span), (first, nframes, back, fresh, lo, n)
        assert lo + n == first + nframes                                    # nothing past the last frame's own hop
        last = first + nframes - 1
        if fresh and last > 0:
            assert last - 1 in span, (first, nframes, back, lo, n)          # the stale part of a trailing partial block
            need.add(last - 1)
        assert lo == min(need)                                              # and nothing below what is needed
    assert seen == {(False, 0), (False, 1), (True, 0), (True, 1)}


def test_means_spans_hold_the_body_and_its_history(lines):
    leads = set()
    for b0, b1, lead, fi, lo, n in lines["means"]:
        leads.add(lead)
        if b1 <= b0:
            assert n == 0
            continue
        need = {h for f in range(b0 - lead, b1) for h in range(f - fi, f + 1)}
        assert min(need) >= 0                                               # (the body lies inside the stream)
        assert set(range(lo, lo + n)) == need, (b0, b1, lead, fi, lo, n)
    assert leads == {0, 3}


def test_the_program_under_address_and_undefined_sanitizers(lines, tmp_path):
    """The same program, its own main, built with gcc's address and undefined-behaviour sanitizers: same output, no report.
    This needs gcc's libasan and libubsan; on a machine without them the test SKIPS and the header has then been walked by the
    plain build only -- a sanitizer run is claimed only where this test is reported as passed."""
    for lib in ("libasan.so", "libubsan.so"):
        path = subprocess.run(["gcc", "-print-file-name=" + lib], check=True, capture_output=True, text=True).stdout.strip()
        if not os.path.isabs(path):
            pytest.skip("gcc's sanitizer runtime is not installed")
    out = _run(tmp_path, "c_frame_cuts_san", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
    assert sum(len(v) for v in lines.values()) == len(out.splitlines())
    plain = _run(tmp_path, "c_frame_cuts_plain")
    assert out == plain
