"""The two halves of a waterfall whose columns live on several GPUs (-m gpu): glfer_hip_levels_host, then
glfer_hip_waterfall_map_device over two slices of the rows, against glfer_hip_waterfall_device over all of them -- rgb and levbuf
with torch.equal, the carried state with ==.  700 rows cross the 256-column chunk of the level walk twice; the second slice's
moving sums reach back across the cut.  The walk's half is one of the four places that take the fixed levels from the shared
display options, and nothing else calls the halves directly."""
import ctypes as C
import itertools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
STATE = ("first_buffer", "display_max_lvl", "display_min_lvl")
NFRAMES, BINS, CUT = 700, 129, 300
LEVELS = {"auto": dict(autoscale=1, overlap=0.5), "fixed": dict(autoscale=0, max_level_db=-20.0, min_level_db=-80.0)}
AV = {"none": dict(avg_mode=0), "plain4": dict(avg_mode=2, depth=4, minbin=0, maxbin=BINS),
      "mode3_7": dict(avg_mode=3, depth=7, minbin=3, maxbin=BINS - 2)}
CASES = list(itertools.product((0, 2), sorted(LEVELS), ("first", "carried"), sorted(AV)))


@pytest.fixture(scope="module")
def rows():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    g = torch.Generator(device="cuda:0").manual_seed(41)
    x = torch.rand((NFRAMES, BINS), generator=g, device="cuda:0", dtype=torch.float32)
    return (x * x * x * x * 0.1 + 2e-4).contiguous()             # PSD-like: non-negative, a floor, a few strong bins


def _state(d):
    return tuple(getattr(d, k) for k in STATE)


@pytest.mark.parametrize("scale_type,levels,incoming,av", CASES, ids=["-".join(map(str, c)) for c in CASES])
def test_levels_host_and_map_halves_equal_the_whole_call(lib, rows, scale_type, levels, incoming, av):
    import torch
    L = lib.api.lib()
    d_in = lib.Display(scale_type=scale_type, palette=3, first_buffer=1 if incoming == "first" else 0, **LEVELS[levels])
    if incoming == "carried":
        d_in.display_max_lvl, d_in.display_min_lvl = 0.06, 0.003
    a = AV[av]
    whole_d = lib.Display.from_buffer_copy(d_in)
    want_rgb, want_lev, stats = lib.waterfall(whole_d, rows, want_stats=True, **a)
    torch.cuda.synchronize()

    # the walk: the statistics meet on the host, one call gives every column its levels and carries the state
    h_stats = np.ascontiguousarray(stats.cpu().numpy())
    h_levels = np.empty((NFRAMES, 4), np.float32)
    walk_d = lib.Display.from_buffer_copy(d_in)
    assert L.glfer_hip_levels_host(C.byref(walk_d), h_stats.ctypes.data, NFRAMES, h_levels.ctypes.data, 0) == 0
    assert _state(walk_d) == _state(whole_d)

    # the map: two slices of the rows, each with its slice of the levels; the Display is read only
    d_levels = torch.from_numpy(h_levels).to("cuda:0")
    rgb = torch.zeros((NFRAMES, BINS, 3), dtype=torch.uint8, device="cuda:0")
    lev = torch.zeros((NFRAMES, BINS), dtype=torch.int16, device="cuda:0")
    map_d = lib.Display.from_buffer_copy(d_in)
    before = bytes(map_d)
    st = C.c_void_p(torch.cuda.current_stream(rows.device).cuda_stream)
    for first, n in ((0, CUT), (CUT, NFRAMES - CUT)):
        rc = L.glfer_hip_waterfall_map_device(C.byref(map_d), a["avg_mode"], a.get("depth", 1), a.get("minbin", 0), a.get("maxbin", 1), 0,
                                              rows.data_ptr(), first, n, BINS, d_levels[first:].data_ptr(), rgb[first:].data_ptr(),
                                              lev[first:].data_ptr(), st)
        assert rc == 0, (first, n)
    torch.cuda.synchronize()
    assert torch.equal(rgb, want_rgb)
    assert torch.equal(lev, want_lev)
    assert bytes(map_d) == before
