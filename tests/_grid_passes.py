"""Which frame a persistent block handles in which pass of its round loop (tests only): the launchers' grid rule restated once,
for the kernels whose blocks walk `while (nfblk < nframes) nfblk += gridDim.x * FPB` -- spectro16cx.hip (cross, Welch),
spectro16a.hip (adaptive, jackknife) and spectro16c.hip (I/Q).  tests/test_grid_passes_host.py holds the restatement to the facts
the suite already writes down; the case modules build their pass-keyed inputs from passes().
Further down, for tests/_walk_cases.py: the same for spectro16.hip, spectro16x.hip, spectro16xl.hip (strided), spectro16h.hip and
spectro16w.hip (a contiguous range per workgroup); how a single-stream call is cut into head, body and tail; and launch16h_fmt's
choice of the register-walk forms (SHIFT, g, per, every slot's frames).

What is restated, and from where:
    resident_workgroups, xcd_slices, persistent_grid      glfer_amd/csrc/launch16.hpp:38-43
    glfer_batch_cap                                       glfer_amd/csrc/spectro_params.h:172-174
    xcd_block_index                                       glfer_amd/csrc/stockham16.hpp:101-104
    Launch16<LOGN>::FPB, BLOCK (T = N / 16 lanes a frame) glfer_amd/csrc/stockham16.hpp:38, 122-125
    LaunchH / LaunchXL / LaunchW (FPB, BLOCK of the other kernels)  spectro16h.hip:109-118, spectro16xl.hip:39-45, spectro16w.hip:81-87
    the waves per SIMD and the multiple of the resident workgroups each launcher passes: KERNELS below
The Makefile overrides none of these with a -D flag (its only -D flags are GLFER_LOGN, GLFER_RAGGED and GLFER_JACKKNIFE).
xcd_block_index() is spelled out inside spectro16h.hip (:495, over the consumer part of the grid): the same map.

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


def _packed_wps(n):                                        # spectro16.hip:31-39 (rows only; 2 with spectrum / RA9MB: :644)
    return 2 if n in (1024, 2048) else 3


def _h_fpb(n):                                             # spectro16h.hip:109-118: T = (N / 2) / 16 lanes a frame
    return max(1, 256 // (n // 32))


def _h_block(n):
    return (n // 32) * _h_fpb(n)


def _w_fpb(n):                                             # spectro16w.hip:81-87: W = N / 2048 wavefronts a frame
    return max(1, 4 // (n // 2048))


def _w_block(n):
    return 64 * (n // 2048) * _w_fpb(n)


def _w_wps(n):                                             # spectro16w.hip:35-37
    return 3 if n == 4096 else 4 if n == 32768 else 2


# kernel: waves per SIMD of size n, the multiple of the resident workgroups, the built sizes, the frames of a unit of work, the
# workgroup's threads, and how a workgroup takes its units: 'strided' (unit i, i + grid, ... of the logical block index) or
# 'contiguous' (units [i per, (i + 1) per), per = ceil(work / grid))
Kernel = collections.namedtuple("Kernel", "wps mult sizes fpb block walk", defaults=(fpb_of, block_of, "strided"))
KERNELS = {
    "spectro16cx": Kernel(lambda n: 2, 4, (256, 512, 1024, 2048, 4096, 8192)),      # spectro16cx.hip:47-49, 407-408; CXLOGNS
    "spectro16a": Kernel(lambda n: 2, 4, (256, 512, 1024, 2048, 4096)),             # spectro16a.hip:49-51, 481-482; ALOGNS
    "spectro16c": Kernel(_iq_wps, 4, (256, 512, 1024, 2048, 4096, 8192, 16384)),    # spectro16c.hip:24-31, 279-280; LOGNS
    # spectro16.hip:152, 210 (fblk = xcd_block_index() * FPB, += gridDim.x * FPB), 640-646; LOGNS
    "spectro16": Kernel(_packed_wps, 4, (256, 512, 1024, 2048, 4096, 8192, 16384)),
    # spectro16h.hip:30-32 (3 waves, 2 at N = 16384), 493-497, 538 (a contiguous range per workgroup), 1041-1043 (8 x); HLOGNS.
    # Plain: the periodogram (SHIFT = 0 below the walk threshold); MT: the multitaper form, built from N = 8192 (:1055)
    "spectro16h": Kernel(lambda n: 2 if n == 16384 else 3, 8, (512, 1024, 2048, 4096, 8192, 16384), _h_fpb, _h_block, "contiguous"),
    "spectro16h_mt": Kernel(lambda n: 2 if n == 16384 else 3, 8, (8192, 16384), _h_fpb, _h_block, "contiguous"),
    # spectro16x.hip:25-26, 105, 137 (fblk = xcd_block_index() * 2 FPB, += gridDim.x * 2 FPB), 263-269; XLOGNS
    "spectro16x": Kernel(lambda n: 3, 4, (256, 512, 1024), lambda n: 2 * fpb_of(n)),
    # spectro16xl.hip:44-45, 102, 109, 268-271 ("resident = 256 * 2": two waves a SIMD at 256 lanes); XLLOGNS
    "spectro16xl": Kernel(lambda n: 2, 4, (256, 512, 1024, 2048), lambda n: 2 * (256 // (n // 16)), lambda n: 256),
    # spectro16w.hip:35-37, 81-87, 312-315 (fblk = xcd_block_index() * per * FPB ... fend), 665-675 (8 x); WLOGNS
    "spectro16w": Kernel(_w_wps, 8, (2048, 4096, 8192, 16384, 32768), _w_fpb, _w_block, "contiguous"),
}


def cap_of(kernel, n, nbatch=1):
    k = KERNELS[kernel]
    assert n in k.sizes, (kernel, n)
    return glfer_batch_cap(k.mult * resident_workgroups(k.wps(n), k.block(n)), nbatch)


def grid_of(kernel, n, frames, nbatch=1):
    """gridDim.x of a call over `frames` frames (rows) of every stream."""
    work = -(-frames // KERNELS[kernel].fpb(n))
    return persistent_grid(work, cap_of(kernel, n, nbatch))


Passes = collections.namedtuple("Passes", "grid fpb stride work npasses pass_of block_of prev logical")


def passes(kernel, n, frames, nbatch=1):
    """Of a call over frames 0 .. frames - 1 (counted from the call's first frame) of one stream of a batch of nbatch:
    grid, fpb (the frames of a unit of work), work, npasses, and per frame pass_of (the round-loop iteration that handles it),
    block_of (blockIdx.x of its block), prev (the frame the same lanes of that block handled one pass earlier, -1 in pass 0) and
    logical (the block's xcd_block_index()).  A 'strided' kernel's block takes units logical, logical + grid, ...: stride =
    grid * fpb frames lie between its passes.  A 'contiguous' kernel's block takes the units [logical * per, (logical + 1) * per),
    per = npasses = ceil(work / grid): stride = fpb, its passes are adjacent units."""
    k = KERNELS[kernel]
    fpb = k.fpb(n)
    grid = grid_of(kernel, n, frames, nbatch)
    work = -(-frames // fpb)
    npasses = -(-work // grid)
    f = np.arange(frames)
    if k.walk == "strided":
        stride = grid * fpb
        logical, pass_of = (f // fpb) % grid, f // stride
    else:
        assert k.walk == "contiguous"
        stride = fpb
        logical, pass_of = (f // fpb) // npasses, (f // fpb) % npasses
    inverse = np.empty(grid, np.int64)
    for w in range(grid):
        inverse[xcd_block_index(w, grid)] = w
    return Passes(grid, fpb, stride, work, npasses, pass_of, inverse[logical], np.where(pass_of >= 1, f - stride, -1), logical)


def pass_bounds(p, frames):
    """[(first frame, end frame)] of every pass of a 'strided' kernel."""
    assert p.stride == p.grid * p.fpb
    return [(k * p.stride, min((k + 1) * p.stride, frames)) for k in range(p.npasses)]


# ---- how a single-stream rows call reaches spectro16h.hip's periodogram forms ---------------------------------------------
# glfer_hip.cpp:934-973 (launch_by_n): frames [lo, hi) are cut by glfer_cut_frames (frame_cuts.h:31-38) with G = 1 for every
# route but the shared-odd one (frame_cuts.h:21-24): head [lo, b0) and tail [b1, hi) go to the packed kernel, the body [b0, b1)
# to the route's kernel, b0 = max(lo, first_inside) rounded up to G, b1 = hi rounded down, first_inside = ceil(R / H)
# (frame_cuts.h:17: the first frame whose history lies inside the stream).  GLFER_FRAME_ALIGN (include/glfer_hip.h:154) = 32 is
# what shards and chunks cut on; the cut itself depends on G alone.
FRAME_ALIGN = 32


def first_inside(n, hop):
    return -(-(n - hop) // hop)


def frame_group(shared_odd, n):
    return 2 * fpb_of(n) if shared_odd else 1


def cut_frames(lo, hi, inside, group=1):
    """(b0, b1) of frames [lo, hi): frame_cuts.h:31-38."""
    b0 = -(-max(lo, inside) // group) * group
    b1 = hi // group * group
    return (hi, hi) if b0 >= b1 else (b0, b1)


# launch16h_fmt (spectro16h.hip:1032-1157) for the periodogram without mean removal, history from the stream, one stream or a
# batch: work = ceil(body / FPB), resident = resident_workgroups(WPS, BLOCK), cap = glfer_batch_cap(8 resident, nbatch).  The hop
# in sixteenths of the frame k16 in {2, 4, 8} and work >= 4 resident: SHIFT = k16 on g = persistent_grid(work / 4, cap)
# (:1146-1155); else SHIFT = 0 on persistent_grid(work, cap) (:1043, 1157).  In the kernel (:493-497, 538) per =
# ceil(body / (g FPB)) frames a slot; workgroup w starts at xcd_block_index(w) * per * FPB, and with SHIFT its slot fl walks the
# frames start + fl * per + it, it = 0 .. per - 1 -- consecutive, 16 - SHIFT register pairs kept from frame to frame; a slot past
# the body's end is clamped and stores nothing.  GLFER16H_PREFETCH2 is 0 in this build (:55-57; the Makefile defines no
# GLFER16H_* macro), so the PF2 landing sets are compiled out: the SHIFT 4 / 8 frame loop is unrolled over the 16 / SHIFT
# rotations (:438, 1004-1010) and loads a frame's SHIFT new pairs straight into the rotating registers.
WALK_SHIFTS = (2, 4, 8)


def hop_sixteenths(n, hop):
    return 16 * hop // n if (16 * hop) % n == 0 else 0


def walk_resident(n):
    k = KERNELS["spectro16h"]
    return resident_workgroups(k.wps(n), k.block(n))


def walk_threshold_frames(n):
    """The fewest body frames whose work is 4 x resident; FPB frames fewer still round up to the same work."""
    return 4 * walk_resident(n) * _h_fpb(n)


Walk = collections.namedtuple("Walk", "shift grid fpb per work slot it nphase last_slot_frames")


def walk(n, hop, body, nbatch=1):
    """launch16h_fmt's choice for a body of `body` frames: shift (0: the plain strided-slot form), grid, fpb, per, work, and per
    body frame (counted from the body's first) slot (logical workgroup * FPB + fl) and it (the frame's place in its slot's walk)."""
    k = KERNELS["spectro16h"]
    fpb = k.fpb(n)
    work = -(-body // fpb)
    resident = walk_resident(n)
    cap = glfer_batch_cap(k.mult * resident, nbatch)
    k16 = hop_sixteenths(n, hop)
    shift = k16 if k16 in WALK_SHIFTS and work >= 4 * resident else 0
    grid = persistent_grid(work // 4, cap) if shift else persistent_grid(work, cap)
    per = -(-body // (grid * fpb))
    f = np.arange(body)
    if shift:
        slot, it = f // per, f % per
    else:                                                   # rel_of(i) = i * FPB + fl from the workgroup's start
        wg, r = f // (per * fpb), f % (per * fpb)
        slot, it = wg * fpb + r % fpb, r // fpb
    last = body - (body - 1) // per * per if shift else 0
    return Walk(shift, grid, fpb, per, work, slot, it, 16 // shift if shift else 1, last)


# ---- the register-walk cases: body frames per size = the threshold and a remainder that leaves a partly filled last slot.  At the
# threshold work / 4 = resident, so g = resident and per = 4 up to g * FPB * 4 body frames, 5 above.  REM_EVEN = -1 keeps per = 4
# and leaves the last slot three frames (FPB >= 2 only: with FPB = 1 one frame fewer is below the threshold); REM_ODD = 10 makes
# per = 5, and no threshold is a multiple of 5, so the last slot holds 1 ... 4 frames and the slots behind it are clamped away
# (test_grid_passes_host.py asserts both)
WALK_REM_EVEN, WALK_REM_ODD = -1, 10


def walk_frames(n, hop, rem):
    """The frames of a whole-stream case: the head, the threshold, the remainder."""
    return first_inside(n, hop) + walk_threshold_frames(n) + rem


# ---- second units of work: 65 ... 71 units on 64 workgroups.  (kernel, n) -> the body frames of `units` units and a partly
# filled last one
def second_unit_frames(kernel, n, units=71, short=1):
    fpb = KERNELS[kernel].fpb(n)
    return units * fpb - (short if fpb > 1 else 0)


# ---- the cases past one pass: frames (rows) per size, work = 71 units -> a grid of 64, seven blocks run a second group
TWO_PASS_FRAMES = {256: 1125, 512: 563, 1024: 281, 2048: 141, 4096: 71, 8192: 71}
BATCH_MULTIPLE_OF_8 = 64                                   # streams: every stream's grid a multiple of 8, three passes and more
BATCH_OTHER = 40                                           # streams: a grid that is no multiple of 8, two passes and more
