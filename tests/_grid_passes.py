"""Which frame a persistent block handles in which pass of its round loop (tests only): the launchers' grid rule restated once,
for the kernels whose blocks walk `while (nfblk < nframes) nfblk += gridDim.x * FPB` -- spectro16cx.hip (cross, Welch),
spectro16a.hip (adaptive, jackknife) and spectro16c.hip (I/Q).  tests/test_grid_passes_host.py holds the restatement to the facts
the suite already writes down; the case modules build their pass-keyed inputs from passes().

What is restated, and from where:
    resident_workgroups, xcd_slices, persistent_grid      glfer_amd/csrc/launch16.hpp:38-43
    glfer_batch_cap                                       glfer_amd/csrc/spectro_params.h:172-174
    xcd_block_index                                       glfer_amd/csrc/stockham16.hpp:101-104
    Launch16<LOGN>::FPB, BLOCK (T = N / 16 lanes a frame) glfer_amd/csrc/stockham16.hpp:38, 122-125
    the waves per SIMD and the multiple of the resident workgroups each launcher passes: KERNELS below
The Makefile overrides none of these with a -D flag (its only -D flags are GLFER_LOGN, GLFER_RAGGED and GLFER_JACKKNIFE).

A unit of WORK is a group of FPB frames (Welch: FPB rows).  Logical group i of a pass belongs to the block whose
xcd_block_index() is i; that block's next group lies `grid` groups, stride = grid * FPB frames, further on.
"""
import collections

import numpy as np

CUS = 256                                                  # launch16.hpp:35 "what the chip (256 CUs) holds"


def resident_workgroups(wps, block):
    per_cu = (wps * 256) // block
    return CUS * (per_cu if per_cu > 0 else 1)


def xcd_slices(grid):
    return grid & ~7 if grid >= 64 else grid


def persistent_grid(work, cap):
    return xcd_slices(min(work, cap))


def glfer_batch_cap(cap, nbatch):
    return (cap + nbatch - 1) // nbatch if nbatch > 1 else cap


def xcd_block_index(w, g):
    """The logical block index of workgroup w in a grid of g."""
    return w if g & 7 else (w & 7) * (g >> 3) + (w >> 3)


def fpb_of(n):
    t = n // 16
    return 1 if t >= 256 else 256 // t


def block_of(n):
    return (n // 16) * fpb_of(n)


def _iq_wps(n):                                            # spectro16c.hip:24-31: spectro16.hip's choice per size
    return 2 if n in (1024, 2048) else 3


# kernel: (waves per SIMD of size n, the multiple of the resident workgroups, the built sizes)
Kernel = collections.namedtuple("Kernel", "wps mult sizes")
KERNELS = {
    "spectro16cx": Kernel(lambda n: 2, 4, (256, 512, 1024, 2048, 4096, 8192)),      # spectro16cx.hip:47-49, 407-408; CXLOGNS
    "spectro16a": Kernel(lambda n: 2, 4, (256, 512, 1024, 2048, 4096)),             # spectro16a.hip:49-51, 481-482; ALOGNS
    "spectro16c": Kernel(_iq_wps, 4, (256, 512, 1024, 2048, 4096, 8192, 16384)),    # spectro16c.hip:24-31, 279-280; LOGNS
}


def cap_of(kernel, n, nbatch=1):
    k = KERNELS[kernel]
    assert n in k.sizes, (kernel, n)
    return glfer_batch_cap(k.mult * resident_workgroups(k.wps(n), block_of(n)), nbatch)


def grid_of(kernel, n, frames, nbatch=1):
    """gridDim.x of a call over `frames` frames (rows) of every stream."""
    work = -(-frames // fpb_of(n))
    return persistent_grid(work, cap_of(kernel, n, nbatch))


Passes = collections.namedtuple("Passes", "grid fpb stride work npasses pass_of block_of prev")


def passes(kernel, n, frames, nbatch=1):
    """Of a call over frames 0 .. frames - 1 (counted from the call's first frame) of one stream of a batch of nbatch:
    grid, fpb, stride = grid * fpb, work, npasses, and per frame pass_of (the round-loop iteration that handles it), block_of
    (blockIdx.x of its block) and prev (the frame the same lanes of that block handled one pass earlier, -1 in pass 0)."""
    fpb = fpb_of(n)
    grid = grid_of(kernel, n, frames, nbatch)
    stride = grid * fpb
    work = -(-frames // fpb)
    f = np.arange(frames)
    logical = (f // fpb) % grid
    inverse = np.empty(grid, np.int64)
    for w in range(grid):
        inverse[xcd_block_index(w, grid)] = w
    return Passes(grid, fpb, stride, work, -(-work // grid), f // stride, inverse[logical], np.where(f >= stride, f - stride, -1))


def pass_bounds(p, frames):
    """[(first frame, end frame)] of every pass."""
    return [(k * p.stride, min((k + 1) * p.stride, frames)) for k in range(p.npasses)]


# ---- the cases past one pass: frames (rows) per size, work = 71 units -> a grid of 64, seven blocks run a second group
TWO_PASS_FRAMES = {256: 1125, 512: 563, 1024: 281, 2048: 141, 4096: 71, 8192: 71}
BATCH_MULTIPLE_OF_8 = 64                                   # streams: every stream's grid a multiple of 8, three passes and more
BATCH_OTHER = 40                                           # streams: a grid that is no multiple of 8, two passes and more
