"""tests/_grid_passes.py held to the launchers' rule and to the facts the suite already writes down (no GPU): the cases past one
grid pass make the passes their tests are named for, their last frame group is partly filled and is not its block's first, and the
batch cases' grids are a multiple of 8 (xcd_block_index's remap applies) in one and not in the other."""
import numpy as np
import pytest

import _grid_passes as G

SINGLE = [(k, n) for k in ("spectro16cx", "spectro16a") for n in G.KERNELS[k].sizes] + [("spectro16c", 256), ("spectro16c", 1024)]
# the batch tests' sizes: one with FPB = 16, one with T = 128 lanes a frame, the largest built size
BATCH_SIZES = {"spectro16cx": (256, 2048, 8192), "spectro16a": (256, 2048, 4096)}


def test_the_restated_functions():
    assert G.resident_workgroups(2, 256) == 512 and G.resident_workgroups(3, 256) == 768 and G.resident_workgroups(2, 512) == 256
    assert G.resident_workgroups(2, 1024) == 256                      # (never less than one workgroup a CU)
    assert [G.xcd_slices(g) for g in (1, 63, 64, 71, 72, 683)] == [1, 63, 64, 64, 72, 680]
    assert G.glfer_batch_cap(2048, 1) == 2048 and G.glfer_batch_cap(2048, 3) == 683 and G.glfer_batch_cap(2048, 64) == 32
    assert [G.fpb_of(n) for n in (256, 512, 1024, 2048, 4096, 8192)] == [16, 8, 4, 2, 1, 1]
    assert [G.block_of(n) for n in (256, 2048, 4096, 8192, 16384)] == [256, 256, 256, 512, 1024]
    for g in (8, 32, 64, 680):                                        # a multiple of 8: XCD w mod 8 takes a contiguous slice
        idx = [G.xcd_block_index(w, g) for w in range(g)]
        assert sorted(idx) == list(range(g))
        for x in range(8):
            mine = [idx[w] for w in range(x, g, 8)]
            assert mine == list(range(x * (g // 8), (x + 1) * (g // 8)))
    assert [G.xcd_block_index(w, 52) for w in range(52)] == list(range(52))


def test_facts_the_suite_already_writes_down():
    # tests/_iq_cases.py: "more workgroups than one XCD slice rule keeps (67 -> a grid of 64)", N = 4096
    assert G.grid_of("spectro16c", 4096, 67) == 64
    p = G.passes("spectro16c", 4096, 67)
    assert p.npasses == 2 and (p.pass_of == 1).sum() == 3
    # tests/test_gpu_ftest_batch.py::test_more_work_than_the_shared_grid: "4 x 512 of 2 frames at N = 2048 ... with 3 streams
    # ... 683 (cut to a multiple of 8: the XCD order)", and 56 workgroups per stream with 37
    cap = G.glfer_batch_cap(4 * G.resident_workgroups(2, G.block_of(2048)), 3)
    assert cap == 683 and G.persistent_grid(10 ** 6, cap) == 680
    assert G.glfer_batch_cap(4 * G.resident_workgroups(2, G.block_of(2048)), 37) == 56
    assert G.glfer_batch_cap(4 * G.resident_workgroups(3, G.block_of(256)), 3) == 1024
    # tests/test_gpu_iq.py::test_batch_sharing_the_grid_equals_single_calls: "N = 16384: a launch keeps 1024 workgroups for all
    # its streams ... five streams of 300 frames (200 workgroups each)" -- 205 by the rule, cut to 200
    assert G.cap_of("spectro16c", 16384) == 1024 and G.grid_of("spectro16c", 16384, 300, 5) == 200


def _last_group_checks(p, n, frames):
    last = frames - 1
    if p.fpb > 1:
        assert frames % p.fpb != 0                                    # partly filled
    assert p.pass_of[last] >= 1                                       # not the first group of its block
    assert p.prev[last] == last - p.stride and p.block_of[p.prev[last]] == p.block_of[last]


@pytest.mark.parametrize("kernel,n", SINGLE)
def test_single_stream_cases_make_two_passes(kernel, n):
    frames = G.TWO_PASS_FRAMES[n]
    p = G.passes(kernel, n, frames)
    assert p.work == 71 and p.grid == 64 and p.stride == 64 * G.fpb_of(n) and p.npasses == 2
    assert len(set(p.block_of[p.pass_of == 1])) == 7                  # seven blocks run a second group
    _last_group_checks(p, n, frames)
    # a block's consecutive groups lie stride frames apart, and every frame has one block and one pass
    for f in range(frames):
        if p.prev[f] >= 0:
            assert p.pass_of[p.prev[f]] == p.pass_of[f] - 1 and p.block_of[p.prev[f]] == p.block_of[f]
    assert G.pass_bounds(p, frames) == [(0, p.stride), (p.stride, frames)]
    # the range calls of section 4: at most 60 work units make a single pass
    assert G.passes(kernel, n, 60 * G.fpb_of(n)).npasses == 1


@pytest.mark.parametrize("kernel", sorted(BATCH_SIZES))
def test_batch_cases(kernel):
    for n in BATCH_SIZES[kernel]:
        frames = G.TWO_PASS_FRAMES[n]
        a = G.passes(kernel, n, frames, G.BATCH_MULTIPLE_OF_8)
        b = G.passes(kernel, n, frames, G.BATCH_OTHER)
        assert a.grid == (16 if n == 8192 else 32) and a.grid % 8 == 0 and a.npasses >= 3, (n, a.grid, a.npasses)
        assert b.grid == (26 if n == 8192 else 52) and b.grid % 8 != 0 and b.npasses >= 2, (n, b.grid, b.npasses)
        for p in (a, b):
            _last_group_checks(p, n, frames)
        # with the remap a block's second group is NOT the one `grid` blockIdx.x further on would suggest by identity
        assert (a.block_of[:a.stride:a.fpb] != np.arange(a.grid)).any()
        assert (b.block_of[:b.stride:b.fpb] == np.arange(b.grid)).all()
    assert G.fpb_of(BATCH_SIZES[kernel][0]) == 16 and BATCH_SIZES[kernel][1] // 16 == 128
    assert BATCH_SIZES[kernel][2] == max(G.KERNELS[kernel].sizes)


# ---- the single-stream route, spectro16h.hip's register-walk forms and the second units of work (tests/_walk_cases.py) ------------
def test_the_restated_kernels():
    import _walk_cases as W
    h, w = G.KERNELS["spectro16h"], G.KERNELS["spectro16w"]
    sizes = (512, 1024, 2048, 4096, 8192, 16384)
    assert [h.fpb(n) for n in sizes] == [16, 8, 4, 2, 1, 1] and [h.block(n) for n in sizes] == [256] * 5 + [512]
    assert [G.walk_resident(n) for n in sizes] == [768] * 5 + [256]
    assert [G.walk_threshold_frames(n) for n in sizes] == [49152, 24576, 12288, 6144, 3072, 1024]
    assert [w.fpb(n) for n in w.sizes] == [4, 2, 1, 1, 1] and [w.block(n) for n in w.sizes] == [256, 256, 256, 512, 1024]
    assert [G.KERNELS["spectro16xl"].fpb(n) for n in (256, 512, 1024, 2048)] == [32, 16, 8, 4]
    assert G.KERNELS["spectro16x"].fpb(1024) == 8 and G.cap_of("spectro16xl", 512) == 2048
    # tests/_rows_cases.py (f): "launch16_fmt (spectro16.hip) starts at most 4 x resident blocks: 2048 x 2 = 4 096 frames at
    # N = 2048 ..., 3072 x 16 = 49 152 at N = 256"; tests/_pairs_cases.py xl_second_pass_from: "grid of at most 2 048 workgroups"
    assert G.cap_of("spectro16", 2048) == 2048 and G.cap_of("spectro16", 256) == 3072
    for kernel in ("spectro16", "spectro16x", "spectro16xl"):
        assert G.KERNELS[kernel].walk == "strided"
    for kernel in ("spectro16h", "spectro16h_mt", "spectro16w"):
        assert G.KERNELS[kernel].walk == "contiguous"
    # the cut: frame_cuts.h's own examples of tests/c_frame_cuts.c's kind
    assert G.first_inside(4096, 1024) == 3 and G.first_inside(4096, 512) == 7 and G.first_inside(4096, 4096) == 0
    assert G.cut_frames(0, 100, 3) == (3, 100) and G.cut_frames(5, 100, 3) == (5, 100) and G.cut_frames(0, 3, 3) == (3, 3)
    assert G.cut_frames(0, 21, 3, 8) == (8, 16) and G.cut_frames(0, 15, 3, 8) == (15, 15) and G.cut_frames(0, 9, 7, 8) == (9, 9)
    assert G.hop_sixteenths(4096, 1024) == 4 and G.hop_sixteenths(4096, 409) == 0
    # tests/_rows_cases.py LONG_CASES: fft(2048, 0.5, ..., 4096 + 1009) stays in the plain form (1 277 units)
    lw = G.walk(2048, 1024, 4096 + 1009 - 1)
    assert lw.shift == 0 and lw.work == 1276 and W.head_of(W.WALK_CASES[0]) == 3


def test_walk_cases_are_above_the_threshold_and_the_just_below_cases_below():
    import _walk_cases as W
    assert len(W.WALK_CASES) == 14
    seen, pers = set(), set()
    for c in W.WALK_CASES:
        b0, w = W.walk_of(c)
        k16 = G.hop_sixteenths(c.n, W.X.hop_len(c.n, c.ovl))
        assert b0 == W.head_of(c) and w.shift == k16 and k16 in G.WALK_SHIFTS, W.case_id(c)
        assert w.work >= 4 * G.walk_resident(c.n) and w.grid == G.walk_resident(c.n) and w.per in (4, 5)
        assert 0 < w.last_slot_frames < w.per                         # a partly filled last slot
        assert w.slot[-1] + 1 < w.grid * w.fpb or w.per == 4          # per = 5: whole slots (and workgroups) past the end
        assert (np.bincount(w.slot)[:-1] == w.per).all() and (np.diff(w.it)[np.diff(w.slot) == 0] == 1).all()
        assert 8e6 <= c.frames * (c.n // 2 + 1) <= 13e6
        seen.add((c.n, w.shift, c.fmt))
        pers.add(w.per)
    assert pers == {4, 5}                                             # an even and an odd per
    assert {n for n, _, _ in seen} == {512, 1024, 2048, 4096, 8192, 16384}
    assert {s for n, s, _ in seen if n == 4096} == {2, 4, 8} and {s for n, s, _ in seen if n <= 1024} == {2, 4, 8}
    assert {f for _, _, f in seen} == {"f32", "s16", "u8"} and {(4, "s16"), (4, "u8")} <= {(s, f) for _, s, f in seen}
    assert (4096, 4, "f32") in seen and W.WALK_CASES[6].window == "hanning"   # C2's own shape
    for c in W.BELOW_CASES:
        _, w = W.walk_of(c)
        assert w.shift == 0 and w.work == 4 * G.walk_resident(c.n) - 1, W.case_id(c)
    # the range calls: still above the threshold, the start off the whole-stream call's slot grid, the end inside a slot of their own
    assert {G.hop_sixteenths(c.n, W.X.hop_len(c.n, c.ovl)) for c in W.RANGE_CASES} == {2, 4, 8}
    for c in W.RANGE_CASES:
        lo, hi = W.range_of(c)
        b0w, whole = W.walk_of(c)
        b0, w = W.walk_of(c, lo, hi)
        assert b0 == lo and w.shift == whole.shift and whole.it[lo - b0w] != 0
        assert 0 < w.last_slot_frames < w.per
    # the batch and the ragged call: every stream's body above the threshold on the grid the streams share
    _, w = W.walk_of(W.BATCH_CASE, nbatch=2)
    assert w.shift == 8 and w.grid == G.walk_resident(W.BATCH_CASE.n)
    for more in (0, W.RAGGED_MORE):
        c = W.RAGGED_CASE._replace(frames=W.RAGGED_CASE.frames + more)
        _, w = W.walk_of(c, nbatch=2)
        assert w.shift == 4 and 0 < w.last_slot_frames < w.per


def test_second_unit_cases_have_65_to_71_units_on_64_workgroups():
    import _walk_cases as W
    kernels = set()
    for s in W.SECOND_CASES:
        b0, b1, p = W.second_passes(s)
        assert 65 <= p.work <= 71 and p.grid == 64 and p.npasses == 2, W.second_id(s)
        late = p.pass_of >= 1
        assert late.any() and (p.block_of[p.prev[late]] == p.block_of[late]).all() and (p.pass_of[p.prev[late]] == 0).all()
        if p.fpb > 1 and not W._shared_odd(s):
            assert (b1 - b0) % p.fpb != 0                             # the last unit is partly filled
        if W._shared_odd(s):
            assert s.c.kmax % 2 == 0 and b1 < s.c.frames and len(W.second_pairs(s)) >= p.fpb // 2
        if s.key == "pass":                                           # a workgroup's two units differ in level, each level in each pass
            lv = W.second_levels(s)[b0:b1]
            assert (lv[late] != lv[p.prev[late]]).all()
            assert set(lv[~late]) == set(W.LEVELS) and len(set(lv[late])) == min(3, -(-int(late.sum()) // p.fpb))
        kernels.add((s.kernel, s.c.est, s.c.n, s.form))
    assert {(k, n) for k, _, n, _ in kernels if k == "spectro16xl"} == {("spectro16xl", 512), ("spectro16xl", 1024), ("spectro16xl", 2048)}
    assert ("spectro16x", "mtm", 1024, "default") in kernels
    for est in ("fft", "mtm"):
        assert {n for k, e, n, f in kernels if k == "spectro16" and e == est and f == "x"} == {512, 1024, 4096, 8192}
        assert {n for k, e, n, f in kernels if k == "spectro16w" and e == est and f == "w"} == {2048, 4096, 8192}
    assert len([s for s in W.SECOND_CASES if s.kernel == "spectro16h_mt"]) == 3
    assert ("spectro16w", "mtm", 16384, "default") in kernels and any(s.spectrum and s.c.n == 32768 for s in W.SECOND_CASES)
    assert any(s.c.fmt != "f32" and s.offset and s.offset % 2 == 0 for s in W.SECOND_CASES)
    # spectro_big.hip: the frame at which subfft_kernel's workgroups start over, and the launcher's scratch group
    assert W.big_wrap_frame(32768) == 1024 < W.BIG_CAP[0].frames and W.big_group_frames(32768) == 4096
    assert W.big_group_frames(1 << 20) == 128 < W.BIG_GROUP[0].frames == 131
