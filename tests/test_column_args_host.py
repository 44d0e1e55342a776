"""The averaging-argument rule without a GPU: one table of bad arguments, applied through ctypes to every entry that takes them.
Every bad call has non-NULL buffers and rows to work on, so the rule itself is what refuses it: GLFER_E_ARG, and a Display's
carried state is left as it was.  The entries that need a plan are skipped where no device exists."""
import ctypes as C

import numpy as np
import pytest

E_ARG = -1
BINS, NFRAMES, N = 129, 10, 256                                 # N / 2 + 1 = BINS: the plan's rows are the table's
GOOD = dict(mode=2, depth=4, minbin=0, maxbin=BINS, n_out=BINS)
# (what is wrong, the arguments that differ from GOOD, update_avg family only)
BAD = [("mode 0 - 1", dict(mode=-1), False), ("mode 5", dict(mode=5), False), ("depth 0", dict(depth=0), False),
       ("minbin -1", dict(minbin=-1), False), ("maxbin == minbin", dict(minbin=40, maxbin=40), False),
       ("maxbin == bins + 1", dict(maxbin=BINS + 1, n_out=BINS + 1), False),
       ("n_out 0", dict(n_out=0), True), ("maxbin > n_out", dict(n_out=BINS - 1), True)]
P = [C.c_void_p(4096 * (i + 1)) for i in range(6)]              # never dereferenced: the rule comes before any device work
STARTS = np.array([0, 4, NFRAMES], np.uint64)
OFFSETS = np.array([0, 8 * N], np.uint64)
LENGTHS = np.array([4 * N, 6 * N], np.uint64)
STATE = (0, 1.5, 0.5)


def _displays(lib, n):
    arr = (lib.Display * n)(*[lib.Display() for _ in range(n)])
    for d in arr:
        d.first_buffer, d.display_max_lvl, d.display_min_lvl = STATE
    return arr


def _waterfall(L, d, a):
    return L.glfer_hip_waterfall_device(d, a["mode"], a["depth"], a["minbin"], a["maxbin"], 0, P[0], NFRAMES, BINS, P[1], P[2], None, None)


def _waterfall_map(L, d, a):
    return L.glfer_hip_waterfall_map_device(d, a["mode"], a["depth"], a["minbin"], a["maxbin"], 0, P[0], 0, NFRAMES, BINS, P[3], P[1], P[2],
                                            None)


def _waterfall_batch(L, d, a):
    return L.glfer_hip_waterfall_batch_device(d, 2, a["mode"], a["depth"], a["minbin"], a["maxbin"], 0, P[0], NFRAMES, BINS, P[1], P[2], None,
                                              None)


def _waterfall_ragged(L, d, a):
    return L.glfer_hip_waterfall_ragged_device(d, 2, a["mode"], a["depth"], a["minbin"], a["maxbin"], 0, P[0], STARTS.ctypes.data, BINS, P[1],
                                               P[2], None, None)


def _avg(L, a):
    return L.glfer_hip_avg_device(a["mode"], P[0], NFRAMES, BINS, a["n_out"], a["depth"], a["minbin"], a["maxbin"], 0, P[1], P[2], None)


def _avg_batch(L, a):
    return L.glfer_hip_avg_batch_device(a["mode"], P[0], 2, NFRAMES, BINS, a["n_out"], a["depth"], a["minbin"], a["maxbin"], 0, P[1], P[2],
                                        None)


def _avg_ragged(L, a):
    return L.glfer_hip_avg_ragged_device(a["mode"], P[0], 2, STARTS.ctypes.data, BINS, a["n_out"], a["depth"], a["minbin"], a["maxbin"], 0,
                                         P[1], P[2], None)


def _avg_cum(L, a):
    return L.glfer_hip_avg_cum_device(P[0], NFRAMES, BINS, a["n_out"], a["depth"], a["minbin"], a["maxbin"], P[1], None)


def _rows_avg(L, plan, a):
    return L.glfer_hip_spectrogram_avg_device(plan, P[0], 20 * N, 0, NFRAMES, a["mode"], a["depth"], a["minbin"], a["maxbin"], 0, a["n_out"],
                                              P[1], P[2], P[3], None)


def _rows_avg_batch(L, plan, a):
    return L.glfer_hip_spectrogram_avg_batch_device(plan, P[0], 2, 20 * N, 20 * N, 0, NFRAMES, a["mode"], a["depth"], a["minbin"], a["maxbin"],
                                                    0, a["n_out"], P[1], P[2], P[3], None)


def _rows_avg_ragged(L, plan, a):
    return L.glfer_hip_spectrogram_avg_ragged_device(plan, P[0], 2, OFFSETS.ctypes.data, LENGTHS.ctypes.data, a["mode"], a["depth"],
                                                     a["minbin"], a["maxbin"], 0, a["n_out"], P[1], P[2], P[3], None, None)


WATERFALLS = [(_waterfall, 1), (_waterfall_map, 1), (_waterfall_batch, 2), (_waterfall_ragged, 2)]
AVERAGES = [_avg, _avg_batch, _avg_ragged, _avg_cum]
WITH_PLAN = [_rows_avg, _rows_avg_batch, _rows_avg_ragged]


@pytest.fixture(scope="module")
def plan(lib):
    """a periodogram plan of BINS bins, or None where no device exists; with a device, a plan that cannot be made is a failure"""
    import torch
    L = lib.api.lib()
    cfg = lib.api.make_config(lib.FftParams(n=N, window_type=0, overlap=0.0))
    h = C.c_void_p()
    rc = L.glfer_hip_plan_create(C.byref(cfg), C.byref(h))
    made = rc == 0
    assert made or not torch.cuda.is_available(), "glfer_hip_plan_create returned %d on a machine with a device" % rc
    yield h if made else None
    if made:
        L.glfer_hip_plan_destroy(h)


@pytest.mark.parametrize("what,change", [b[:2] for b in BAD if not b[2]], ids=[b[0] for b in BAD if not b[2]])
def test_bad_averaging_arguments_waterfalls(lib, what, change):
    L = lib.api.lib()                                           # (the waterfall entries take no n_out)
    args = dict(GOOD, **change)
    for call, n in WATERFALLS:
        d = _displays(lib, n)
        assert call(L, d, args) == E_ARG, (call.__name__, what)
        assert [(x.first_buffer, x.display_max_lvl, x.display_min_lvl) for x in d] == [STATE] * n, (call.__name__, what)


@pytest.mark.parametrize("what,change", [b[:2] for b in BAD], ids=[b[0] for b in BAD])
def test_bad_averaging_arguments_update_avg(lib, what, change):
    L = lib.api.lib()
    args = dict(GOOD, **change)
    for call in AVERAGES:
        if call is _avg_cum and "mode" in change:
            continue                                            # (the sliding sums have no mode)
        assert call(L, args) == E_ARG, (call.__name__, what)


@pytest.mark.parametrize("what,change", [b[:2] for b in BAD], ids=[b[0] for b in BAD])
def test_bad_averaging_arguments_rows_and_average(lib, plan, what, change):
    if plan is None:
        pytest.skip("no device: no plan can be made")
    L = lib.api.lib()
    args = dict(GOOD, **change)
    for call in WITH_PLAN:
        assert call(L, plan, args) == E_ARG, (call.__name__, what)
