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
