"""The ragged moving average and waterfall without a GPU: the entries are exported, the C argument rules that need no device,
the Python wrappers' shape and dtype refusals, and the numpy restatement of the chunked sliding sum that the GPU test's
inexact-sum input relies on."""
import numpy as np
import pytest

from _ragged_cols import avg_chunk, chunked_sums, row_starts, swinging_rows

ENTRIES = ("glfer_hip_avg_ragged_device", "glfer_hip_spectrogram_avg_ragged_device", "glfer_hip_waterfall_ragged_device")


def test_ragged_columns_entries_exported(lib):
    L = lib.api.lib()
    for name in ENTRIES:
        assert hasattr(L, name), name
        assert name in lib.api.EXPORTS, name
    assert callable(getattr(lib.Spectrogram, "run_avg_ragged", None))
    assert callable(getattr(lib, "update_avg_ragged", None)) and callable(getattr(lib, "waterfall_ragged", None))


def test_ragged_columns_argument_rules_without_a_device(lib):
    L = lib.api.lib()
    good = np.array([0, 3, 3, 8], np.uint64)
    down = np.array([0, 5, 3, 8], np.uint64)
    none = np.zeros(4, np.uint64)
    # the average: nothing to do comes first, then the table, then the buffers
    assert L.glfer_hip_avg_ragged_device(2, None, 0, None, 65, 65, 4, 0, 65, 0, None, None, None) == 0
    assert L.glfer_hip_avg_ragged_device(2, None, 3, none.ctypes.data, 65, 65, 4, 0, 65, 0, None, None, None) == 0
    assert L.glfer_hip_avg_ragged_device(2, None, 3, None, 65, 65, 4, 0, 65, 0, None, None, None) == -1
    assert L.glfer_hip_avg_ragged_device(2, None, 3, down.ctypes.data, 65, 65, 4, 0, 65, 0, None, None, None) == -1
    assert L.glfer_hip_avg_ragged_device(2, None, 3, good.ctypes.data, 65, 65, 4, 0, 65, 0, None, None, None) == -1   # no buffers
    assert L.glfer_hip_avg_ragged_device(0, None, 3, none.ctypes.data, 65, 65, 4, 0, 65, 0, None, None, None) == -1   # the mode
    assert L.glfer_hip_avg_ragged_device(2, None, 3, none.ctypes.data, 65, 65, 4, 0, 66, 0, None, None, None) == -1   # the band
    huge = np.array([0, 2 ** 62], np.uint64)
    assert L.glfer_hip_avg_ragged_device(2, None, 1, huge.ctypes.data, 65, 65, 4, 0, 65, 0, None, None, None) == -1   # overflows
    # the rows and the average: no plan
    assert L.glfer_hip_spectrogram_avg_ragged_device(None, None, 2, None, None, 2, 4, 0, 65, 0, 65, None, None, None, None, None) == -1
    # the waterfall
    disps = (lib.Display * 3)(*[lib.Display() for _ in range(3)])
    assert L.glfer_hip_waterfall_ragged_device(disps, 0, 0, 1, 0, 1, 0, None, None, 129, None, None, None, None) == 0
    assert L.glfer_hip_waterfall_ragged_device(disps, 3, 0, 1, 0, 1, 0, None, none.ctypes.data, 129, None, None, None, None) == 0
    assert L.glfer_hip_waterfall_ragged_device(None, 3, 0, 1, 0, 1, 0, None, good.ctypes.data, 129, None, None, None, None) == -1
    assert L.glfer_hip_waterfall_ragged_device(disps, 3, 0, 1, 0, 1, 0, None, None, 129, None, None, None, None) == -1
    assert L.glfer_hip_waterfall_ragged_device(disps, 3, 0, 1, 0, 1, 0, None, down.ctypes.data, 129, None, None, None, None) == -1
    assert L.glfer_hip_waterfall_ragged_device(disps, 3, 0, 1, 0, 1, 0, None, good.ctypes.data, 129, None, None, None, None) == -1
    before = [bytes(d) for d in disps]
    disps[1].palette = 3                                                       # options that differ
    assert L.glfer_hip_waterfall_ragged_device(disps, 3, 0, 1, 0, 1, 0, None, none.ctypes.data, 129, None, None, None, None) == -1
    disps[1].palette = disps[0].palette
    assert [bytes(d) for d in disps] == before


def test_ragged_wrappers_refuse_bad_shapes_and_dtypes(lib):
    import torch
    cpu = torch.zeros((8, 65), dtype=torch.float32)
    with pytest.raises(ValueError):
        lib.update_avg_ragged(2, cpu, [0, 3, 8], 4, 0, 65)                     # not on the GPU
    with pytest.raises(ValueError):
        lib.waterfall_ragged([lib.Display(), lib.Display()], cpu, [0, 3, 8])
    two = [lib.Display(), lib.Display()]
    for bad_psd, match in ((torch.zeros((8, 65), dtype=torch.float64), "float32"), (torch.zeros(8 * 65), "2-D"),
                           (torch.zeros((2, 4, 65)), "2-D"), (torch.zeros((8, 65), dtype=torch.int32), "float32")):
        with pytest.raises(ValueError, match=match):
            lib.update_avg_ragged(2, bad_psd, [0, 3, 8], 4, 0, 65)             # the dtype and the rank, before any device is asked for
        with pytest.raises(ValueError, match=match):
            lib.waterfall_ragged(two, bad_psd, [0, 3, 8])
    with pytest.raises(ValueError, match="one Display per stream"):
        lib.waterfall_ragged(two + [lib.Display()], cpu, [0, 3, 8])
    with pytest.raises(ValueError, match="one Display per stream"):
        lib.waterfall_ragged(two[:1], cpu, [0, 3, 8])
    with pytest.raises(ValueError, match="row_starts"):
        lib.update_avg_ragged(2, cpu, [0, 5, 3, 8], 4, 0, 65)
    with pytest.raises(ValueError, match="row_starts"):
        lib.waterfall_ragged(two, cpu, [0, 3, 9])                              # past the rows given
    for bad in ([[0, 3], [3, 8]], [0.0, 3.0, 8.0], [], [0, 5, 3, 8], [0, 3, 9]):
        with pytest.raises(ValueError):
            lib.api._row_starts(bad, 8)
    assert list(lib.api._row_starts([0, 3, 3, 8], 8)) == [0, 3, 3, 8]
    assert lib.api._row_starts(np.array([0, 8], np.int32), 8).dtype == np.uint64


def test_chunk_lengths_of_the_single_stream_launchers():
    assert [avg_chunk(n) for n in (1, 40, 8191, 8192, 16383, 16384, 16400, 32768, 40000, 65536, 131071, 131072, 10 ** 7)] == \
        [8, 8, 8, 8, 8, 16, 16, 32, 32, 64, 64, 128, 128]


@pytest.mark.parametrize("depth", [4, 6])
def test_inexact_window_sums_carry_their_chunk_length(depth):
    """the GPU test's input (swinging_rows) really yields different doubles for two chunk lengths, and well-scaled rows do not"""
    x = swinging_rows(200, 65, seed=21)
    by_chunk = {c: chunked_sums(x, depth, c) for c in (8, 16, 32)}
    for a, b in ((8, 16), (16, 32), (8, 32)):
        differ = by_chunk[a].view(np.int64) != by_chunk[b].view(np.int64)
        assert differ.any(), (a, b)
        # ... in frames of chunks that restart in one and not in the other only, and never by more than rounding
        assert np.allclose(by_chunk[a], by_chunk[b], rtol=1e-6, atol=1e-2)
    assert not (by_chunk[8][:8].view(np.int64) != by_chunk[32][:8].view(np.int64)).any()   # the first chunk has no restart
    tame = (np.random.default_rng(3).random((200, 65)).astype(np.float32) * 16).astype(np.float32)
    tame = np.round(tame * 1024) / 1024                                        # few mantissa bits: every addition exact
    assert np.array_equal(chunked_sums(tame, depth, 8), chunked_sums(tame, depth, 32))
    assert list(row_starts([0, 3, 5])) == [0, 0, 3, 8]
