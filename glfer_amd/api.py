"""Host-side binding of the C-ABI in include/glfer_hip.h (glfer_amd/lib/libglfer_hip.so).

Everything computed here runs in the HIP library; torch is used only to own device
memory and streams.  There is no CPU fallback: if the library is missing, or HIP cannot
run, the calls raise.

Names follow the reference's estimator interface (fft.h:77-83, mtm.h:47-49, avg.h:38-43):
`FftParams` / `MtmParams` carry what change_params() copies out of `opt`
(source.c:320-325, 343-350) and `Spectrogram` is the per-hop loop of source.c:130-158
run over a whole stream.
"""
import collections
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# GLFER_LIB_PATH: another build of the library (same-box A/B runs of kernel variants, tools/)
LIB_PATH = os.environ.get("GLFER_LIB_PATH") or os.path.join(_HERE, "lib", "libglfer_hip.so")

MODE_FFT, MODE_MTM, MODE_HPARMA, MODE_LMP = 0, 1, 2, 3
WAV_PARTIAL_TAIL = 1
IQ_CENTERED, IQ_SWAP = 1, 2                            # flags of the complex I/Q entries
CROSS_FIELDS = ("sxx", "syy", "sxy", "coh")
Cross = collections.namedtuple("Cross", CROSS_FIELDS)  # what Spectrogram.cross returns: None for what was not asked
ADAPTIVE_FIELDS = ("psd", "dof")
Adaptive = collections.namedtuple("Adaptive", ADAPTIVE_FIELDS)  # what Spectrogram.adaptive returns: None for what was not asked
JACKKNIFE_FIELDS = ("psd", "dof", "logvar")
Jackknife = collections.namedtuple("Jackknife", JACKKNIFE_FIELDS)  # what Spectrogram.jackknife returns: None for what was not asked
DRIFT_FIELDS = ("sums", "best", "drift")
Drift = collections.namedtuple("Drift", "sums best drift")  # what drift_sums and Spectrogram.run_drift return: None for what was not asked
WINDOWS = {"hanning": 0, "blackman": 1, "gaussian": 2, "welch": 3,
           "bartlett": 4, "rectangular": 5, "hamming": 6, "kaiser": 7}
SAMPLES_F32, SAMPLES_S16, SAMPLES_U8 = 0, 1, 2
HISTORY_ZERO_FIRST, HISTORY_ZERO_ALWAYS = 0, 1
SUBMEAN_OFF, SUBMEAN_EXACT, SUBMEAN_FAST = 0, 1, 2     # cfg.sub_mean: 1 = the reference's rows (fft.c:86-96 in its own summation order)
AVG_SUMAVG, AVG_PLAIN, AVG_SUMEXTREME = 1, 2, 3

# every symbol include/glfer_hip.h declares
EXPORTS = [
    "glfer_hip_plan_create", "glfer_hip_plan_destroy", "glfer_hip_hop", "glfer_hip_bins",
    "glfer_hip_num_tapers", "glfer_hip_num_frames", "glfer_hip_get_window", "glfer_hip_get_tapers",
    "glfer_hip_make_window", "glfer_hip_make_dpss", "glfer_hip_y_half_tables", "glfer_hip_y_queue_shape", "glfer_hip_spectrogram_device",
    "glfer_hip_spectrum_device", "glfer_hip_spectrogram_host", "glfer_hip_wav_probe",
    "glfer_hip_spectrogram_wav", "glfer_hip_submean_device",
    "glfer_hip_floor_device",
    "glfer_hip_avg_device", "glfer_hip_palette", "glfer_hip_display_device", "glfer_hip_strerror", "glfer_hip_last_hip_error", "glfer_hip_version",
    "glfer_hip_frame_range", "glfer_hip_prepare_device", "glfer_hip_mtm_ftest_device", "glfer_hip_host_alloc",
    "glfer_hip_host_free", "glfer_hip_spectrogram_host_multi", "glfer_hip_spectrogram_wav_ex",
    "glfer_hip_avg_cum_device", "glfer_hip_waterfall_host", "glfer_hip_waterfall_device",
    "glfer_hip_spectrogram_host_workers",
    # round 3
    "glfer_hip_scratch_trim", "glfer_hip_scratch_held", "glfer_hip_scratch_limit", "glfer_hip_spectrogram_wav_range",
    "glfer_hip_spectrogram_wav_multi", "glfer_hip_spectrogram_wav_workers", "glfer_hip_levels_host",
    "glfer_hip_waterfall_map_device", "glfer_hip_waterfall_host_workers", "glfer_hip_waterfall_wav_workers",
    "glfer_hip_waterfall_wav_multi", "glfer_hip_submean_exact_device",
    # round 4
    "glfer_hip_numa_node_of_bus_id", "glfer_hip_numa_node_cpus", "glfer_hip_floor_device_pitched",
    # round 5
    "glfer_hip_abi_version", "glfer_hip_spectrogram_avg_device", "glfer_hip_workers_create", "glfer_hip_workers_destroy",
    "glfer_hip_workers_spectrogram_wav", "glfer_hip_workers_spectrogram_host",
    # many streams per call
    "glfer_hip_spectrogram_batch_device", "glfer_hip_avg_batch_device", "glfer_hip_spectrogram_avg_batch_device",
    "glfer_hip_waterfall_batch_device", "glfer_hip_mtm_ftest_batch_device",
    # the multitaper rows and F from one pass over the samples
    "glfer_hip_mtm_rows_ftest_device", "glfer_hip_mtm_rows_ftest_batch_device",
    # streams of unequal length in one call
    "glfer_hip_spectrogram_ragged_device", "glfer_hip_ragged_frames",
    # their moving average and waterfall
    "glfer_hip_avg_ragged_device", "glfer_hip_spectrogram_avg_ragged_device", "glfer_hip_waterfall_ragged_device",
    # their harmonic F-test, alone and beside the multitaper rows
    "glfer_hip_mtm_ftest_ragged_device", "glfer_hip_mtm_rows_ftest_ragged_device",
    # the LMP statistic over rows already on the device: one stream, a batch, ragged
    "glfer_hip_lmp_device", "glfer_hip_lmp_batch_device", "glfer_hip_lmp_ragged_device",
    # multi-channel recordings: every interleaved channel as a stream of its own
    "glfer_hip_deinterleave_device", "glfer_hip_spectrogram_channels_device", "glfer_hip_spectrogram_host_channels",
    "glfer_hip_spectrogram_wav_channels",
    # complex I/Q input: two-sided rows
    "glfer_hip_iq_supported", "glfer_hip_iq_tables", "glfer_hip_spectrogram_iq_device", "glfer_hip_spectrogram_iq_batch_device",
    # zoom: the digital down-converter and the I/Q rows of its output
    "glfer_hip_ddc_phase_word", "glfer_hip_ddc_design", "glfer_hip_ddc_supported", "glfer_hip_ddc_tables", "glfer_hip_ddc_create",
    "glfer_hip_ddc_destroy", "glfer_hip_ddc_device", "glfer_hip_ddc_batch_device", "glfer_hip_spectrogram_zoom_device",
    # two channels: multitaper auto- and cross-spectra and coherence in one pass
    "glfer_hip_cross_supported", "glfer_hip_mtm_cross_device", "glfer_hip_mtm_cross_batch_device",
    # the same averaged over L consecutive segments (Welch): FFT plans too
    "glfer_hip_welch_cross_supported", "glfer_hip_welch_rows", "glfer_hip_welch_cross_device", "glfer_hip_welch_cross_batch_device",
    # adaptive multitaper weights: leakage-resistant rows and their degrees of freedom in one pass
    "glfer_hip_adaptive_supported", "glfer_hip_adaptive_weights", "glfer_hip_mtm_adaptive_device", "glfer_hip_mtm_adaptive_batch_device",
    # jackknife confidence intervals for multitaper rows in the same pass
    "glfer_hip_jackknife_supported", "glfer_hip_jackknife_factor", "glfer_hip_mtm_jackknife_device",
    "glfer_hip_mtm_jackknife_batch_device",
    # the drift search: rows summed along straight lines of frequency drift
    "glfer_hip_drift_blocks", "glfer_hip_drift_offsets", "glfer_hip_drift_device", "glfer_hip_drift_batch_device",
    "glfer_hip_spectrogram_drift_device",
]


class GlferHipError(RuntimeError):
    pass


class Config(C.Structure):
    """glfer_hip_config (include/glfer_hip.h)."""
    _fields_ = [("mode", C.c_int), ("n", C.c_int), ("overlap", C.c_float),
                ("window_type", C.c_int), ("limiter_a", C.c_float), ("enable_limiter", C.c_int),
                ("sub_mean", C.c_int), ("history_mode", C.c_int), ("mtm_w", C.c_float),
                ("mtm_k", C.c_int), ("sample_format", C.c_int), ("device", C.c_int),
                ("hparma_t", C.c_int), ("hparma_p_e", C.c_int), ("lmp_av", C.c_int), ("psd_pitch", C.c_int)]


class DdcConfig(C.Structure):
    """glfer_hip_ddc_config (include/glfer_hip.h)."""
    _fields_ = [("decim", C.c_int), ("ntaps", C.c_int), ("freq", C.c_double), ("complex_in", C.c_int),
                ("sample_format", C.c_int), ("device", C.c_int)]


class Display(C.Structure):
    """glfer_hip_display (include/glfer_hip.h): the options and the carried state of
    main_window_draw's level tracking and pixel mapping (g_main.c:1099-1236)."""
    _fields_ = [("scale_type", C.c_int), ("autoscale", C.c_int), ("overlap", C.c_float),
                ("max_level_db", C.c_float), ("min_level_db", C.c_float), ("thr_level", C.c_float),
                ("palette", C.c_int), ("first_buffer", C.c_int), ("display_max_lvl", C.c_float),
                ("display_min_lvl", C.c_float), ("psd_pitch", C.c_int)]

    def __init__(self, scale_type=2, autoscale=1, overlap=0.0, max_level_db=-10.0, min_level_db=-60.0,
                 thr_level=0.0, palette=0, first_buffer=1, psd_pitch=0):
        super().__init__(scale_type, autoscale, overlap, max_level_db, min_level_db, thr_level,
                         palette, first_buffer, 0.0, 0.0, psd_pitch)


SCALE_LIN, SCALE_LIN_MAX0, SCALE_LOG, SCALE_LOG_MAX0 = range(4)          # glfer.h:43
PALETTES = {"hsv": 0, "thresh": 1, "cool": 2, "hot": 3, "bw": 4, "bone": 5, "copper": 6, "otd": 7}


class Phases(C.Structure):
    """glfer_hip_phases: where a call through a workers handle spent its time (seconds; the largest value over the workers)."""
    _fields_ = [("setup_s", C.c_double), ("read_s", C.c_double), ("h2d_s", C.c_double), ("kernel_s", C.c_double),
                ("d2h_s", C.c_double), ("wall_s", C.c_double), ("chunks", C.c_uint)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class WavInfo(C.Structure):
    """glfer_wav_info (include/glfer_hip.h): the header fields of wav_fmt.h:34-52 that are used."""
    _fields_ = [("format", C.c_int), ("channels", C.c_int), ("sample_rate", C.c_int),
                ("bits_per_sample", C.c_int), ("data_offset", C.c_size_t), ("nsamples", C.c_size_t),
                ("data_bytes", C.c_size_t)]


_lib = None


def lib():
    """Load libglfer_hip.so (built by __graft_entry__.build()); fail loudly if absent."""
    global _lib
    if _lib is not None:
        return _lib
    # torch bundles its own HIP runtime (same soname as /opt/rocm's); load it first so that
    # this process ends up with ONE runtime shared by torch tensors/streams and our kernels
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    if not os.path.exists(LIB_PATH):
        raise GlferHipError(
            "HIP extension not built: %s is missing (run `python -c 'import __graft_entry__ as g; "
            "g.build()'` or `make -C glfer_amd/csrc`). There is no CPU fallback." % LIB_PATH)
    L = C.CDLL(LIB_PATH)
    vp, sz = C.c_void_p, C.c_size_t
    L.glfer_hip_plan_create.argtypes = [C.POINTER(Config), C.POINTER(vp)]
    L.glfer_hip_plan_destroy.argtypes = [vp]
    L.glfer_hip_plan_destroy.restype = None
    for f in ("glfer_hip_hop", "glfer_hip_bins", "glfer_hip_num_tapers"):
        getattr(L, f).argtypes = [vp]
    L.glfer_hip_num_frames.argtypes = [vp, sz]
    L.glfer_hip_num_frames.restype = sz
    L.glfer_hip_get_window.argtypes = [vp, vp]
    L.glfer_hip_get_tapers.argtypes = [vp, vp, vp]
    L.glfer_hip_make_window.argtypes = [C.c_int, C.c_int, vp]
    L.glfer_hip_make_dpss.argtypes = [C.c_int, C.c_int, C.c_double, vp, vp]
    if hasattr(L, "glfer_hip_y_half_tables"):          # (absent from older builds loaded through GLFER_LIB_PATH for A/B runs)
        L.glfer_hip_y_half_tables.argtypes = [C.c_int, C.c_int, C.c_double, vp, vp, vp]
    if hasattr(L, "glfer_hip_y_queue_shape"):
        L.glfer_hip_y_queue_shape.argtypes = [vp, vp]
        L.glfer_hip_y_queue_shape.restype = None
    L.glfer_hip_spectrogram_device.argtypes = [vp, vp, sz, sz, sz, vp, vp]
    L.glfer_hip_spectrogram_batch_device.argtypes = [vp, vp, sz, sz, sz, sz, sz, vp, vp]
    L.glfer_hip_spectrum_device.argtypes = [vp, vp, sz, sz, sz, vp, vp, vp]
    L.glfer_hip_spectrogram_host.argtypes = [vp, vp, sz, vp, C.POINTER(sz)]
    L.glfer_hip_wav_probe.argtypes = [C.c_char_p, C.POINTER(WavInfo)]
    L.glfer_hip_spectrogram_wav.argtypes = [vp, C.c_char_p, vp, sz, C.POINTER(sz), sz]
    L.glfer_hip_submean_device.argtypes = [vp, vp, C.c_int, sz, C.c_int, vp]
    L.glfer_hip_submean_exact_device.argtypes = [vp, vp, C.c_int, sz, C.c_int, vp]
    L.glfer_hip_floor_device.argtypes = [vp, sz, C.c_int, vp, vp]
    L.glfer_hip_floor_device_pitched.argtypes = [vp, sz, C.c_int, C.c_int, vp, vp]
    L.glfer_hip_palette.argtypes = [C.c_int, vp]
    L.glfer_hip_display_device.argtypes = [C.POINTER(Display), vp, vp, vp, sz, C.c_int, vp, vp, vp, vp]
    L.glfer_hip_avg_device.argtypes = [C.c_int, vp, sz, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                       C.c_int, vp, vp, vp]
    L.glfer_hip_frame_range.argtypes = [sz, C.c_uint, C.c_uint, C.POINTER(sz), C.POINTER(sz)]
    L.glfer_hip_frame_range.restype = None
    L.glfer_hip_prepare_device.argtypes = [vp, vp, sz, sz, sz, vp, vp]
    L.glfer_hip_mtm_ftest_device.argtypes = [vp, vp, sz, sz, sz, vp, C.c_int, vp]
    if hasattr(L, "glfer_hip_mtm_ftest_batch_device"):  # (absent from older builds loaded through GLFER_LIB_PATH for A/B runs)
        L.glfer_hip_mtm_ftest_batch_device.argtypes = [vp, vp, sz, sz, sz, sz, sz, vp, C.c_int, vp]
    if hasattr(L, "glfer_hip_mtm_rows_ftest_device"):
        L.glfer_hip_mtm_rows_ftest_device.argtypes = [vp, vp, sz, sz, sz, vp, vp, C.c_int, vp]
    if hasattr(L, "glfer_hip_mtm_rows_ftest_batch_device"):
        L.glfer_hip_mtm_rows_ftest_batch_device.argtypes = [vp, vp, sz, sz, sz, sz, sz, vp, vp, C.c_int, vp]
    if hasattr(L, "glfer_hip_spectrogram_ragged_device"):
        L.glfer_hip_spectrogram_ragged_device.argtypes = [vp, vp, sz, vp, vp, vp, vp, vp]
    if hasattr(L, "glfer_hip_mtm_ftest_ragged_device"):
        L.glfer_hip_mtm_ftest_ragged_device.argtypes = [vp, vp, sz, vp, vp, vp, C.c_int, vp, vp]
    if hasattr(L, "glfer_hip_mtm_rows_ftest_ragged_device"):
        L.glfer_hip_mtm_rows_ftest_ragged_device.argtypes = [vp, vp, sz, vp, vp, vp, vp, C.c_int, vp, vp]
    if hasattr(L, "glfer_hip_ragged_frames"):
        L.glfer_hip_ragged_frames.argtypes = [vp, sz, vp, vp]
        L.glfer_hip_ragged_frames.restype = sz
    if hasattr(L, "glfer_hip_avg_ragged_device"):
        L.glfer_hip_avg_ragged_device.argtypes = [C.c_int, vp, sz, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp]
    if hasattr(L, "glfer_hip_lmp_device"):
        L.glfer_hip_lmp_device.argtypes = [vp, sz, sz, sz, C.c_int, C.c_int, vp, vp]
        L.glfer_hip_lmp_batch_device.argtypes = [vp, sz, sz, sz, sz, sz, C.c_int, C.c_int, vp, sz, vp]
        L.glfer_hip_lmp_ragged_device.argtypes = [vp, sz, vp, C.c_int, C.c_int, vp, vp]
    if hasattr(L, "glfer_hip_spectrogram_avg_ragged_device"):
        L.glfer_hip_spectrogram_avg_ragged_device.argtypes = [vp, vp, sz, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                                              vp, vp, vp, vp, vp]
    if hasattr(L, "glfer_hip_waterfall_ragged_device"):
        L.glfer_hip_waterfall_ragged_device.argtypes = [C.POINTER(Display), sz, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, C.c_int, vp, vp,
                                                        vp, vp]
    if hasattr(L, "glfer_hip_deinterleave_device"):
        L.glfer_hip_deinterleave_device.argtypes = [vp, sz, C.c_int, C.c_int, vp, C.c_int, vp, sz, vp]
        L.glfer_hip_spectrogram_channels_device.argtypes = [vp, vp, sz, C.c_int, vp, C.c_int, sz, sz, vp, vp]
        L.glfer_hip_spectrogram_host_channels.argtypes = [vp, vp, sz, C.c_int, vp, C.c_int, vp, C.POINTER(sz)]
        L.glfer_hip_spectrogram_wav_channels.argtypes = [vp, C.c_char_p, vp, C.c_int, vp, sz, C.POINTER(sz), sz]
    if hasattr(L, "glfer_hip_spectrogram_iq_device"):
        L.glfer_hip_iq_supported.argtypes = [C.POINTER(Config)]
        L.glfer_hip_iq_tables.argtypes = [C.POINTER(Config), vp]
        L.glfer_hip_spectrogram_iq_device.argtypes = [vp, vp, sz, sz, sz, vp, sz, C.c_uint, vp]
        L.glfer_hip_spectrogram_iq_batch_device.argtypes = [vp, vp, sz, sz, sz, sz, sz, vp, sz, C.c_uint, vp]
    if hasattr(L, "glfer_hip_mtm_cross_device"):
        L.glfer_hip_cross_supported.argtypes = [C.POINTER(Config)]
        L.glfer_hip_mtm_cross_device.argtypes = [vp, vp, sz, sz, sz, vp, vp, vp, sz, vp, sz, vp]
        L.glfer_hip_mtm_cross_batch_device.argtypes = [vp, vp, sz, sz, sz, sz, sz, vp, vp, vp, sz, vp, sz, vp]
    if hasattr(L, "glfer_hip_welch_cross_device"):
        L.glfer_hip_welch_cross_supported.argtypes = [C.POINTER(Config), sz, sz]
        L.glfer_hip_welch_rows.argtypes = [vp, sz, sz, sz, sz]
        L.glfer_hip_welch_rows.restype = sz
        L.glfer_hip_welch_cross_device.argtypes = [vp, vp, sz, sz, sz, sz, sz, vp, vp, vp, sz, vp, sz, vp]
        L.glfer_hip_welch_cross_batch_device.argtypes = [vp, vp, sz, sz, sz, sz, sz, sz, sz, vp, vp, vp, sz, vp, sz, vp]
    if hasattr(L, "glfer_hip_mtm_adaptive_device"):
        L.glfer_hip_adaptive_supported.argtypes = [C.POINTER(Config)]
        L.glfer_hip_adaptive_weights.argtypes = [C.POINTER(Config), vp, vp]
        L.glfer_hip_mtm_adaptive_device.argtypes = [vp, vp, sz, sz, sz, vp, vp, sz, C.c_int, vp]
        L.glfer_hip_mtm_adaptive_batch_device.argtypes = [vp, vp, sz, sz, sz, sz, sz, vp, vp, sz, C.c_int, vp]
    if hasattr(L, "glfer_hip_mtm_jackknife_device"):
        L.glfer_hip_jackknife_supported.argtypes = [C.POINTER(Config)]
        L.glfer_hip_jackknife_factor.argtypes = [C.POINTER(Config), C.c_double, C.POINTER(C.c_double)]
        L.glfer_hip_mtm_jackknife_device.argtypes = [vp, vp, sz, sz, sz, vp, vp, vp, sz, C.c_int, vp]
        L.glfer_hip_mtm_jackknife_batch_device.argtypes = [vp, vp, sz, sz, sz, sz, sz, vp, vp, vp, sz, C.c_int, vp]
    if hasattr(L, "glfer_hip_ddc_device"):
        L.glfer_hip_ddc_phase_word.argtypes = [C.c_double]
        L.glfer_hip_ddc_phase_word.restype = C.c_ulonglong
        L.glfer_hip_ddc_design.argtypes = [C.c_int, C.c_int, C.c_double, C.c_double, vp]
        L.glfer_hip_ddc_supported.argtypes = [C.POINTER(DdcConfig)]
        L.glfer_hip_ddc_tables.argtypes = [C.POINTER(DdcConfig), vp, vp]
        L.glfer_hip_ddc_create.argtypes = [C.POINTER(DdcConfig), vp, C.POINTER(vp)]
        L.glfer_hip_ddc_destroy.argtypes = [vp]
        L.glfer_hip_ddc_destroy.restype = None
        L.glfer_hip_ddc_device.argtypes = [vp, vp, sz, sz, sz, vp, vp]
        L.glfer_hip_ddc_batch_device.argtypes = [vp, vp, sz, sz, sz, sz, sz, vp, sz, vp]
        L.glfer_hip_spectrogram_zoom_device.argtypes = [vp, vp, vp, sz, sz, sz, vp, sz, C.c_uint, vp]
    if hasattr(L, "glfer_hip_drift_device"):
        L.glfer_hip_drift_blocks.argtypes = [sz, sz, sz]
        L.glfer_hip_drift_blocks.restype = sz
        L.glfer_hip_drift_offsets.argtypes = [sz, C.c_int, C.c_int, vp]
        L.glfer_hip_drift_device.argtypes = [vp, sz, C.c_int, sz, sz, sz, sz, C.c_int, C.c_int, vp, vp, vp, vp]
        L.glfer_hip_drift_batch_device.argtypes = [vp, sz, sz, sz, C.c_int, sz, sz, sz, sz, C.c_int, C.c_int, vp, sz, vp, sz, vp, sz, vp]
        L.glfer_hip_spectrogram_drift_device.argtypes = [vp, vp, sz, sz, sz, sz, sz, C.c_int, C.c_int, vp, vp, vp, vp]
    L.glfer_hip_host_alloc.argtypes = [sz]
    L.glfer_hip_host_alloc.restype = vp
    L.glfer_hip_host_free.argtypes = [vp]
    L.glfer_hip_host_free.restype = None
    L.glfer_hip_spectrogram_host_multi.argtypes = [C.POINTER(Config), C.c_uint, vp, sz, vp, C.POINTER(sz)]
    L.glfer_hip_spectrogram_host_workers.argtypes = [C.POINTER(Config), C.POINTER(C.c_int), C.c_int, vp, sz, vp, C.POINTER(sz)]
    L.glfer_hip_spectrogram_wav_ex.argtypes = [vp, C.c_char_p, vp, sz, C.POINTER(sz), sz, C.c_uint]
    L.glfer_hip_avg_cum_device.argtypes = [vp, sz, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp]
    L.glfer_hip_waterfall_device.argtypes = [C.POINTER(Display), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, sz, C.c_int,
                                             vp, vp, vp, vp]
    L.glfer_hip_waterfall_host.argtypes = [vp, C.POINTER(Display), vp, sz, vp, vp, C.POINTER(sz)]
    cfgp, ip, dispp, szp = C.POINTER(Config), C.POINTER(C.c_int), C.POINTER(Display), C.POINTER(sz)
    L.glfer_hip_spectrogram_wav_range.argtypes = [vp, C.c_char_p, sz, sz, vp, szp, sz, C.c_uint]
    L.glfer_hip_spectrogram_wav_multi.argtypes = [cfgp, C.c_uint, C.c_char_p, vp, sz, szp, C.c_uint]
    L.glfer_hip_spectrogram_wav_workers.argtypes = [cfgp, ip, C.c_int, C.c_char_p, vp, sz, szp, C.c_uint]
    L.glfer_hip_waterfall_host_workers.argtypes = [cfgp, ip, C.c_int, dispp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                                   vp, sz, vp, vp, szp]
    L.glfer_hip_waterfall_wav_workers.argtypes = [cfgp, ip, C.c_int, dispp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                                  C.c_char_p, sz, vp, vp, szp, C.c_uint]
    L.glfer_hip_waterfall_wav_multi.argtypes = [cfgp, C.c_uint, dispp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                                C.c_char_p, sz, vp, vp, szp, C.c_uint]
    L.glfer_hip_levels_host.argtypes = [dispp, vp, sz, vp, C.c_int]
    L.glfer_hip_waterfall_map_device.argtypes = [dispp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, sz, sz, C.c_int,
                                                 vp, vp, vp, vp]
    L.glfer_hip_numa_node_of_bus_id.argtypes = [C.c_char_p, C.c_char_p]
    L.glfer_hip_numa_node_cpus.argtypes = [C.c_int, C.c_char_p, vp, sz]
    L.glfer_hip_scratch_trim.argtypes = [C.c_int, sz]
    L.glfer_hip_scratch_trim.restype = sz
    L.glfer_hip_scratch_held.argtypes = [C.c_int]
    L.glfer_hip_scratch_held.restype = sz
    L.glfer_hip_scratch_limit.argtypes = [sz]
    L.glfer_hip_scratch_limit.restype = None
    for f in ("glfer_hip_strerror", "glfer_hip_last_hip_error", "glfer_hip_version"):
        getattr(L, f).restype = C.c_char_p
    L.glfer_hip_strerror.argtypes = [C.c_int]
    L.glfer_hip_abi_version.argtypes = []
    L.glfer_hip_workers_create.argtypes = [C.POINTER(Config), C.POINTER(C.c_int), C.c_int, sz, C.POINTER(vp)]
    L.glfer_hip_workers_destroy.argtypes = [vp]
    L.glfer_hip_workers_destroy.restype = None
    L.glfer_hip_workers_spectrogram_wav.argtypes = [vp, C.c_char_p, vp, sz, C.POINTER(sz), C.c_uint, C.POINTER(Phases)]
    L.glfer_hip_workers_spectrogram_host.argtypes = [vp, vp, sz, vp, C.POINTER(sz), C.POINTER(Phases)]
    L.glfer_hip_spectrogram_avg_device.argtypes = [vp, vp, sz, sz, sz, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp]
    L.glfer_hip_waterfall_batch_device.argtypes = [dispp, sz, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, sz, C.c_int, vp, vp,
                                                   vp, vp]
    L.glfer_hip_avg_batch_device.argtypes = [C.c_int, vp, sz, sz, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp]
    L.glfer_hip_spectrogram_avg_batch_device.argtypes = [vp, vp, sz, sz, sz, sz, sz, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                                         C.c_int, vp, vp, vp, vp]
    _lib = L
    return L


def _check(rc, what):
    if rc != 0:
        L = lib()
        raise GlferHipError("%s failed: %s (%s)" % (
            what, L.glfer_hip_strerror(rc).decode(), L.glfer_hip_last_hip_error().decode()))


def version():
    return lib().glfer_hip_version().decode()


def make_window(window_type, n):
    """compute_window (fft.c:309-360), host code of the library."""
    w = np.empty(n, np.float32)
    _check(lib().glfer_hip_make_window(int(window_type), n, w.ctypes.data), "make_window")
    return w


def make_dpss(n, kmax, nw):
    """gl_dpss (g-l_dpss.c:288-347), host code of the library: (tapers[kmax+1][n], sig)."""
    v = np.empty((kmax + 1, n), np.float64)
    s = np.empty(kmax + 1, np.float64)
    _check(lib().glfer_hip_make_dpss(n, kmax, float(nw), v.ctypes.data, s.ctypes.data), "make_dpss")
    return v, s


def iq_supported(params):
    """Whether a plan of these parameters takes complex I/Q input (glfer_hip_iq_supported; host only)."""
    cfg = make_config(params)
    return lib().glfer_hip_iq_supported(C.byref(cfg)) == 0


def cross_supported(params):
    """Whether a plan of these parameters gives cross-spectra and coherence (glfer_hip_cross_supported; host only)."""
    cfg = make_config(params)
    return lib().glfer_hip_cross_supported(C.byref(cfg)) == 0


def welch_cross_supported(params, segments, step):
    """Whether a plan of these parameters gives cross-spectra and coherence averaged over `segments` frames, rows `step` frames
    apart (glfer_hip_welch_cross_supported; host only)."""
    cfg = make_config(params)
    return lib().glfer_hip_welch_cross_supported(C.byref(cfg), segments, step) == 0


def adaptive_supported(params):
    """Whether a plan of these parameters gives adaptively weighted rows (glfer_hip_adaptive_supported; host only)."""
    cfg = make_config(params)
    return lib().glfer_hip_adaptive_supported(C.byref(cfg)) == 0


def jackknife_supported(params):
    """Whether a plan of these parameters gives jackknife rows (glfer_hip_jackknife_supported; host only)."""
    cfg = make_config(params)
    return lib().glfer_hip_jackknife_supported(C.byref(cfg)) == 0


def jackknife_factor(params, level=0.95):
    """Student's quantile t_{K-1}((1 + level) / 2), what sqrt(logvar) is multiplied by for the interval at `level`
    (glfer_hip_jackknife_factor; host only)."""
    cfg = make_config(params)
    t = C.c_double()
    _check(lib().glfer_hip_jackknife_factor(C.byref(cfg), float(level), C.byref(t)), "glfer_hip_jackknife_factor")
    return t.value


def jackknife_interval(jk, params, level=0.95):
    """(lower, upper) of the interval at `level` around jk.psd: psd exp(-/+ t sqrt(logvar)), t = jackknife_factor(params, level);
    torch tensors on the rows' device.  No bias correction.  logvar = +inf gives (0, +inf) where psd > 0."""
    torch = _torch()
    half = jackknife_factor(params, level) * torch.sqrt(jk.logvar)
    # (psd = 0 has logvar = 0: the interval is the point 0, never 0 * inf)
    return jk.psd * torch.exp(-half), jk.psd * torch.exp(half)


def adaptive_weights(params):
    """(lambda, beta): the float32 weights the adaptive kernel gets for a plan of these parameters, one per taper
    (glfer_hip_adaptive_weights; host only)."""
    cfg = make_config(params)
    k = params.kmax + 1
    lam, beta = np.empty(k, np.float32), np.empty(k, np.float32)
    rc = lib().glfer_hip_adaptive_weights(C.byref(cfg), lam.ctypes.data, beta.ctypes.data)
    if rc != k:
        _check(rc if rc < 0 else -1, "glfer_hip_adaptive_weights")
    return lam, beta


def iq_tables(params):
    """The scaled float table [tapers][n] of the complex I/Q rows (glfer_hip_iq_tables; host only)."""
    cfg = make_config(params)
    nt = lib().glfer_hip_iq_tables(C.byref(cfg), None)
    if nt < 0:
        _check(nt, "glfer_hip_iq_tables")
    tab = np.empty((nt, params.n), np.float32)
    rc = lib().glfer_hip_iq_tables(C.byref(cfg), tab.ctypes.data)
    if rc < 0:
        _check(rc, "glfer_hip_iq_tables")
    return tab


def ddc_phase_word(freq):
    """W = round(freq 2^64) mod 2^64 (glfer_hip_ddc_phase_word; host only)."""
    return int(lib().glfer_hip_ddc_phase_word(float(freq)))


def ddc_design(decim, ntaps=0, cutoff=0.0, beta=0.0):
    """The Kaiser-windowed sinc low-pass of the down-converter as float32 taps (glfer_hip_ddc_design; host only).  Arguments <= 0
    take the defaults: ntaps = min(8 decim + 1, 8192), cutoff = 0.4 / decim cycles per input sample, beta = 8."""
    nt = lib().glfer_hip_ddc_design(int(decim), int(ntaps), float(cutoff), float(beta), None)
    if nt < 0:
        _check(nt, "glfer_hip_ddc_design")
    taps = np.empty(nt, np.float32)
    rc = lib().glfer_hip_ddc_design(int(decim), int(ntaps), float(cutoff), float(beta), taps.ctypes.data)
    if rc < 0:
        _check(rc, "glfer_hip_ddc_design")
    return taps


def ddc_supported(decim, ntaps, freq, complex_in=False, sample_format=SAMPLES_F32):
    """Whether a down-converter of this shape can be made (glfer_hip_ddc_supported; host only)."""
    cfg = DdcConfig(int(decim), int(ntaps), float(freq), int(complex_in), int(sample_format), 0)
    return lib().glfer_hip_ddc_supported(C.byref(cfg)) == 0


def ddc_tables(freq, taps):
    """The complex taps g[t] = taps[t] exp(+2 pi i phi(t)) as complex64 (glfer_hip_ddc_tables; host only)."""
    taps = np.ascontiguousarray(taps, np.float32)
    cfg = DdcConfig(1, len(taps), float(freq), 0, SAMPLES_F32, 0)
    g = np.empty((len(taps), 2), np.float32)
    _check(lib().glfer_hip_ddc_tables(C.byref(cfg), taps.ctypes.data, g.ctypes.data), "glfer_hip_ddc_tables")
    return g.view(np.complex64)[:, 0]


class Ddc:
    """A digital down-converter (glfer_hip_ddc, include/glfer_hip.h "Zoom"): y[m] = exp(-2 pi i phi(n0)) sum_t g[t] x[n0 - t],
    n0 = (m + 1) decim - 1 -- the band around `freq` (cycles per input sample) moved to 0 Hz, low-passed by `taps` (float32;
    None: ddc_design(decim, ntaps)) and decimated.  Real input: 1-D tensors of the sample format's dtype; complex input
    (complex_in=True): complex64 [S], or [S, 2] pairs of the sample format's dtype.  Output: complex64."""

    def __init__(self, decim, freq, taps=None, ntaps=0, complex_in=False, sample_format=SAMPLES_F32, device=0):
        self._h = None
        if taps is None:
            taps = ddc_design(decim, ntaps)
        self.taps = np.ascontiguousarray(taps, np.float32)
        assert self.taps.ndim == 1
        self.decim, self.freq, self.complex_in, self.sample_format, self.device = int(decim), float(freq), bool(complex_in), sample_format, device
        self.cfg = DdcConfig(self.decim, len(self.taps), self.freq, int(self.complex_in), sample_format, device)
        if lib().glfer_hip_ddc_supported(C.byref(self.cfg)) != 0:
            raise GlferHipError("unsupported down-converter: decim %d, %d taps, freq %r" % (self.decim, len(self.taps), self.freq))
        self.phase_word = ddc_phase_word(self.freq)
        self._destroy = lib().glfer_hip_ddc_destroy
        h = C.c_void_p()
        _check(lib().glfer_hip_ddc_create(C.byref(self.cfg), self.taps.ctypes.data, C.byref(h)), "glfer_hip_ddc_create")
        self._h = h

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._destroy(self._h)
            self._h.value = None

    __del__ = close

    def tables(self):
        """The complex taps g[T] as complex64 (glfer_hip_ddc_tables; host only)."""
        g = np.empty((len(self.taps), 2), np.float32)
        _check(lib().glfer_hip_ddc_tables(C.byref(self.cfg), self.taps.ctypes.data, g.ctypes.data), "glfer_hip_ddc_tables")
        return g.view(np.complex64)[:, 0]

    def num_out(self, nsamples):
        return nsamples // self.decim

    def _dtype(self):
        torch = _torch()
        return {SAMPLES_F32: torch.float32, SAMPLES_S16: torch.int16, SAMPLES_U8: torch.uint8}[self.sample_format]

    def _view(self, x, lead):
        """(tensor whose data_ptr is sample 0 of stream 0, samples per stream, stream pitch in input samples)"""
        torch = _torch()
        assert x.is_cuda, "the input lives on the GPU"
        if self.complex_in:
            if x.is_complex():
                assert x.dtype == torch.complex64, x.dtype
                x = torch.view_as_real(x)
            assert x.dim() == lead + 2 and x.size(-1) == 2, tuple(x.shape)
            assert x.dtype == self._dtype(), (x.dtype, self._dtype())
            assert x.stride(-1) == 1 and (x.stride(-2) == 2 or x.size(-2) <= 1), x.stride()
            ns = x.size(-2)
            if lead and x.size(0) > 1:
                assert x.stride(0) % 2 == 0, x.stride()
                return x, ns, x.stride(0) // 2
            return x, ns, ns
        assert x.dim() == lead + 1 and x.dtype == self._dtype(), (tuple(x.shape), x.dtype, self._dtype())
        assert x.stride(-1) == 1 or x.size(-1) <= 1, x.stride()
        ns = x.size(-1)
        return x, ns, (x.stride(0) if lead and x.size(0) > 1 else ns)

    def _out(self, out, shape, device):
        torch = _torch()
        if out is None:
            return torch.empty(shape, dtype=torch.complex64, device=device), shape[-1]
        assert out.is_cuda and out.dtype == torch.complex64 and tuple(out.shape) == tuple(shape), (tuple(out.shape), shape)
        assert out.stride(-1) == 1 or out.size(-1) <= 1
        pitch = out.stride(0) if len(shape) == 2 and out.size(0) > 1 else shape[-1]
        assert pitch >= shape[-1]
        return out, pitch

    def run(self, x, first_out=0, nout=None, out=None):
        """Outputs [first_out, first_out + nout) of the stream x as complex64 [nout], launched on torch's current stream
        (glfer_hip_ddc_device)."""
        torch = _torch()
        v, ns, _ = self._view(x, 0)
        if nout is None:
            nout = self.num_out(ns) - first_out
        out, _ = self._out(out, (nout,), v.device)
        st = C.c_void_p(torch.cuda.current_stream(v.device).cuda_stream)
        _check(lib().glfer_hip_ddc_device(self._h, C.c_void_p(v.data_ptr()), ns, first_out, nout, C.c_void_p(out.data_ptr()), st),
               "glfer_hip_ddc_device")
        return out

    def run_batch(self, xs, first_out=0, nout=None, out=None):
        """xs: [B, S] with stride(1) == 1 (complex input: complex64 [B, S] or [B, S, 2]); stride(0) is the distance between streams.
        Returns complex64 [B][nout]: out[b] is what run(xs[b]) gives; `out` may be a view with a row stride above nout
        (glfer_hip_ddc_batch_device)."""
        torch = _torch()
        v, ns, spitch = self._view(xs, 1)
        nb = v.size(0)
        if nout is None:
            nout = self.num_out(ns) - first_out
        out, opitch = self._out(out, (nb, nout), v.device)
        st = C.c_void_p(torch.cuda.current_stream(v.device).cuda_stream)
        _check(lib().glfer_hip_ddc_batch_device(self._h, C.c_void_p(v.data_ptr()), nb, spitch, ns, first_out, nout,
                                                C.c_void_p(out.data_ptr()), opitch, st), "glfer_hip_ddc_batch_device")
        return out


class FftParams:
    """What source.c:320-325 sets before fft_init(): n, window_type, overlap, a, limiter."""

    def __init__(self, n=1024, window_type=7, overlap=0.0, a=0.0, limiter=0, sub_mean=0,
                 history_mode=HISTORY_ZERO_FIRST, sample_format=SAMPLES_F32, psd_pitch=0):
        self.mode = MODE_FFT
        self.psd_pitch = psd_pitch                      # cfg.psd_pitch: floats from one PSD row to the next (0 = dense)
        self.n, self.window_type, self.overlap = n, window_type, overlap
        self.a, self.limiter, self.sub_mean = a, limiter, sub_mean
        self.history_mode, self.sample_format = history_mode, sample_format
        self.w, self.kmax = 0.0, 0


class MtmParams:
    """What source.c:343-350 sets before mtm_init(): fft.{n,overlap}, w (=N*W), kmax."""

    def __init__(self, n=1024, overlap=0.0, w=4.0, kmax=7, sub_mean=0,
                 history_mode=HISTORY_ZERO_FIRST, sample_format=SAMPLES_F32, psd_pitch=0):
        self.mode = MODE_MTM
        self.psd_pitch = psd_pitch
        self.n, self.overlap, self.w, self.kmax = n, overlap, w, kmax
        self.window_type = WINDOWS["rectangular"]       # source.c:344
        self.a, self.limiter, self.sub_mean = 0.0, 0, sub_mean
        self.history_mode, self.sample_format = history_mode, sample_format


class HparmaParams:
    """What source.c:368-376 sets before hparma_init(): fft.{n,overlap}, t, p_e (q_e = -1)."""

    def __init__(self, n=4096, overlap=0.0, t=96, p_e=16, sub_mean=0, history_mode=HISTORY_ZERO_FIRST,
                 sample_format=SAMPLES_F32, psd_pitch=0):
        self.mode = MODE_HPARMA
        self.psd_pitch = psd_pitch
        self.n, self.overlap, self.t, self.p_e = n, overlap, t, p_e
        self.window_type = WINDOWS["rectangular"]       # source.c:369
        self.a, self.limiter, self.sub_mean = 0.0, 0, sub_mean
        self.history_mode, self.sample_format = history_mode, sample_format
        self.w, self.kmax = 0.0, 0


class LmpParams:
    """What source.c:390-398 sets before lmp_init(): fft.{n,overlap}, avg = opt.lmp_av (window
    rectangular; a and the limiter act on a buffer lmp_do overwrites, lmp.c:114-116)."""

    def __init__(self, n=1024, overlap=0.0, avg=4, sub_mean=0, history_mode=HISTORY_ZERO_FIRST,
                 sample_format=SAMPLES_F32):
        self.mode = MODE_LMP
        self.n, self.overlap, self.avg = n, overlap, avg
        self.window_type = WINDOWS["rectangular"]       # source.c:395
        self.a, self.limiter, self.sub_mean = 0.0, 0, sub_mean
        self.history_mode, self.sample_format = history_mode, sample_format
        self.w, self.kmax = 0.0, 0


_TORCH_DTYPES = None


def _torch():
    import torch
    return torch


def make_config(params, device=0):
    return Config(params.mode, params.n, params.overlap, params.window_type, params.a,
                  params.limiter, params.sub_mean, params.history_mode, params.w, params.kmax,
                  params.sample_format, device, getattr(params, "t", 0), getattr(params, "p_e", 0),
                  getattr(params, "avg", 0), getattr(params, "psd_pitch", 0))


class Spectrogram:
    """A plan (fft_init / mtm_init) bound to one GPU, plus the batched hot path."""

    def __init__(self, params, device=0):
        cfg = make_config(params, device)
        self._h = C.c_void_p()
        self._destroy = lib().glfer_hip_plan_destroy     # held here: module globals are gone by the time __del__ runs at exit
        _check(lib().glfer_hip_plan_create(C.byref(cfg), C.byref(self._h)), "glfer_hip_plan_create")
        self.params, self.device = params, device
        self.n = params.n
        self.hop = lib().glfer_hip_hop(self._h)
        self.bins = lib().glfer_hip_bins(self._h)
        self.pitch = getattr(params, "psd_pitch", 0) or self.bins     # floats from one row of run()'s output to the next
        self.ntapers = lib().glfer_hip_num_tapers(self._h)

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._destroy(self._h)
            self._h.value = None

    __del__ = close

    def num_frames(self, nsamples):
        return lib().glfer_hip_num_frames(self._h, nsamples)

    def window(self):
        w = np.empty(self.n, np.float32)
        _check(lib().glfer_hip_get_window(self._h, w.ctypes.data), "get_window")
        return w

    def tapers(self):
        v = np.empty((self.ntapers, self.n), np.float64)
        s = np.empty(self.ntapers, np.float64)
        _check(lib().glfer_hip_get_tapers(self._h, v.ctypes.data, s.ctypes.data), "get_tapers")
        return v, s

    def _sample_dtype(self):
        torch = _torch()
        return {SAMPLES_F32: torch.float32, SAMPLES_S16: torch.int16,
                SAMPLES_U8: torch.uint8}[self.params.sample_format]

    def run(self, stream, first_frame=0, nframes=None, out=None, spectrum=False):
        """stream: 1-D torch tensor on this GPU.  Returns psd [nframes][bins] (and the
        halfcomplex spectra [nframes][n] when spectrum=True), launched on torch's current
        stream."""
        torch = _torch()
        assert stream.is_cuda and stream.dim() == 1 and stream.is_contiguous()
        assert stream.dtype == self._sample_dtype(), (stream.dtype, self._sample_dtype())
        total = self.num_frames(stream.numel())
        if nframes is None:
            nframes = total - first_frame
        if out is None:
            out = torch.empty((nframes, self.pitch), dtype=torch.float32, device=stream.device)
        assert out.is_contiguous() and out.numel() >= nframes * self.pitch
        st = C.c_void_p(torch.cuda.current_stream(stream.device).cuda_stream)
        if spectrum:
            spec = torch.empty((nframes, self.n), dtype=torch.float32, device=stream.device)
            _check(lib().glfer_hip_spectrum_device(self._h, stream.data_ptr(), stream.numel(),
                                                   first_frame, nframes, out.data_ptr(),
                                                   spec.data_ptr(), st), "glfer_hip_spectrum_device")
            return out, spec
        _check(lib().glfer_hip_spectrogram_device(self._h, stream.data_ptr(), stream.numel(),
                                                  first_frame, nframes, out.data_ptr(), st),
               "glfer_hip_spectrogram_device")
        return out                                       # (with cfg.psd_pitch: [nframes][pitch], a row's first `bins` floats are its bins)

    def run_batch(self, streams, first_frame=0, nframes=None, out=None):
        """streams: 2-D torch tensor [B, T] on this GPU, of the plan's sample dtype, stride(1) == 1 (stride(0) is the
        distance between streams, in samples).  Returns psd [B][nframes][pitch] -- out[b] is what run(streams[b]) gives --
        launched on torch's current stream (glfer_hip_spectrogram_batch_device)."""
        torch = _torch()
        assert streams.is_cuda and streams.dim() == 2 and (streams.stride(1) == 1 or streams.size(1) <= 1)
        assert streams.dtype == self._sample_dtype(), (streams.dtype, self._sample_dtype())
        nb, total = streams.size(0), streams.size(1)
        if nframes is None:
            nframes = self.num_frames(total) - first_frame
        if out is None:
            out = torch.empty((nb, nframes, self.pitch), dtype=torch.float32, device=streams.device)
        assert out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.numel() >= nb * nframes * self.pitch
        st = C.c_void_p(torch.cuda.current_stream(streams.device).cuda_stream)
        _check(lib().glfer_hip_spectrogram_batch_device(self._h, C.c_void_p(streams.data_ptr()), nb, streams.stride(0), total,
                                                        first_frame, nframes, C.c_void_p(out.data_ptr()), st),
               "glfer_hip_spectrogram_batch_device")
        return out

    def _iq_view(self, iq, lead):
        """The interleaved parts of a complex input as [lead dims..., S, 2] of the plan's sample dtype: complex64 [.., S] or
        [.., S, 2] float32 / int16 / uint8 with a contiguous inner part."""
        torch = _torch()
        assert iq.is_cuda, "complex I/Q input lives on the GPU"
        if iq.is_complex():
            assert iq.dtype == torch.complex64, iq.dtype
            iq = torch.view_as_real(iq)
        assert iq.dim() == lead + 2 and iq.size(-1) == 2, tuple(iq.shape)
        assert iq.dtype == self._sample_dtype(), (iq.dtype, self._sample_dtype())
        assert iq.stride(-1) == 1 and (iq.stride(-2) == 2 or iq.size(-2) <= 1), iq.stride()
        return iq

    def _iq_out(self, out, shape, device):
        torch = _torch()
        if out is None:
            return torch.empty(shape, dtype=torch.float32, device=device), self.n
        assert out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == tuple(shape), (tuple(out.shape), shape)
        assert out.stride(-1) == 1 or out.size(-1) <= 1
        pitch = out.stride(-2) if out.size(-2) > 1 else self.n          # a pitched view: its row stride is the row pitch
        assert pitch >= self.n
        if len(shape) == 3 and out.size(0) > 1:
            assert out.stride(0) == shape[1] * pitch, "batch rows lie (b * nframes + i) * row_pitch floats from the first"
        return out, pitch

    def run_iq(self, iq, first_frame=0, nframes=None, out=None, centered=False, swap=False):
        """iq: complex64 [S] or [S, 2] float32 / int16 / uint8 (I, Q pairs; the dtype is the plan's sample format) on this GPU.
        Returns the two-sided rows [nframes][n] float32 -- bin k of exp(+2 pi i k n / N) in column k, or column (k + n/2) mod n
        with centered=True; swap=True: the first value of a pair is Q -- launched on torch's current stream
        (glfer_hip_spectrogram_iq_device).  out: [nframes][n], its row stride may be larger than n."""
        torch = _torch()
        v = self._iq_view(iq, 0)
        ns = v.size(0)
        if nframes is None:
            nframes = self.num_frames(ns) - first_frame
        out, pitch = self._iq_out(out, (nframes, self.n), v.device)
        st = C.c_void_p(torch.cuda.current_stream(v.device).cuda_stream)
        flags = (IQ_CENTERED if centered else 0) | (IQ_SWAP if swap else 0)
        _check(lib().glfer_hip_spectrogram_iq_device(self._h, C.c_void_p(v.data_ptr()), ns, first_frame, nframes,
                                                     C.c_void_p(out.data_ptr()), pitch, flags, st), "glfer_hip_spectrogram_iq_device")
        return out

    def run_iq_batch(self, iqs, first_frame=0, nframes=None, out=None, centered=False, swap=False):
        """iqs: complex64 [B, S] or [B, S, 2] with a contiguous inner part; stride(0) is the distance between streams (in
        complex samples once divided by two for the [B, S, 2] form).  Returns [B][nframes][n] float32: out[b] is what
        run_iq(iqs[b]) gives (glfer_hip_spectrogram_iq_batch_device)."""
        torch = _torch()
        v = self._iq_view(iqs, 1)
        nb, ns = v.size(0), v.size(1)
        assert nb <= 1 or v.stride(0) % 2 == 0, v.stride()
        spitch = v.stride(0) // 2 if nb > 1 else ns
        if nframes is None:
            nframes = self.num_frames(ns) - first_frame
        out, pitch = self._iq_out(out, (nb, nframes, self.n), v.device)
        st = C.c_void_p(torch.cuda.current_stream(v.device).cuda_stream)
        flags = (IQ_CENTERED if centered else 0) | (IQ_SWAP if swap else 0)
        _check(lib().glfer_hip_spectrogram_iq_batch_device(self._h, C.c_void_p(v.data_ptr()), nb, spitch, ns, first_frame, nframes,
                                                           C.c_void_p(out.data_ptr()), pitch, flags, st),
               "glfer_hip_spectrogram_iq_batch_device")
        return out

    def _cross_outs(self, want, out, lead, nframes, device):
        """The four outputs of a cross call as (tensors by name, row pitch, sxy pitch): made here, or the caller's (out: a
        mapping or a Cross tuple of tensors [lead..., nframes, n/2+1] whose row stride may be larger; the float rows share one)."""
        torch = _torch()
        want = tuple(want)
        assert want and all(w in CROSS_FIELDS for w in want), want
        bins = self.n // 2 + 1
        shape = tuple(lead) + (nframes, bins)
        if out is not None and not isinstance(out, dict):
            out = out._asdict()
        ts, pitches = {}, {}
        for name in want:
            dt = torch.complex64 if name == "sxy" else torch.float32
            o = None if out is None else out.get(name)
            if o is None:
                ts[name], pitches[name] = torch.empty(shape, dtype=dt, device=device), bins
                continue
            assert o.is_cuda and o.dtype == dt and tuple(o.shape) == shape, (name, tuple(o.shape), shape)
            assert o.stride(-1) == 1 or o.size(-1) <= 1
            pitches[name] = o.stride(-2) if o.size(-2) > 1 else bins
            assert pitches[name] >= bins
            if lead and o.size(0) > 1:
                assert o.stride(0) == nframes * pitches[name], "batch rows lie (b * nframes + i) rows from the first"
            ts[name] = o
        rp = {pitches[k] for k in want if k != "sxy"}
        assert len(rp) <= 1, "sxx, syy and coh share one row pitch"
        return ts, (rp.pop() if rp else 0), pitches.get("sxy", 0)

    @staticmethod
    def _cross_ptr(ts, name):
        return C.c_void_p(ts[name].data_ptr()) if name in ts else None

    def cross(self, xy, first_frame=0, nframes=None, want=("coh", "sxy"), out=None):
        """xy: [S, 2] float32 / int16 / uint8 (x, y pairs; the dtype is the plan's sample format) or complex64 [S] (x in the real
        part) on this GPU; the plan is a multitaper one with kmax >= 1.  Returns Cross(sxx, syy, sxy, coh) with None for what
        `want` does not name: sxx, syy, coh float32 [nframes][n/2+1], sxy complex64 [nframes][n/2+1]; y lagging x by d samples
        gives angle(sxy[k]) = +2 pi k d / n.  One launch on torch's current stream (glfer_hip_mtm_cross_device)."""
        torch = _torch()
        v = self._iq_view(xy, 0)
        ns = v.size(0)
        if nframes is None:
            nframes = self.num_frames(ns) - first_frame
        ts, pitch, xpitch = self._cross_outs(want, out, (), nframes, v.device)
        st = C.c_void_p(torch.cuda.current_stream(v.device).cuda_stream)
        _check(lib().glfer_hip_mtm_cross_device(self._h, C.c_void_p(v.data_ptr()), ns, first_frame, nframes, self._cross_ptr(ts, "sxx"),
                                                self._cross_ptr(ts, "syy"), self._cross_ptr(ts, "coh"), pitch,
                                                self._cross_ptr(ts, "sxy"), xpitch, st), "glfer_hip_mtm_cross_device")
        return Cross(*(ts.get(k) for k in CROSS_FIELDS))

    def cross_batch(self, xys, first_frame=0, nframes=None, want=("coh", "sxy"), out=None):
        """xys: [B, S, 2] (or complex64 [B, S]) with a contiguous inner part; stride(0) is the distance between streams.  Returns
        Cross of [B][nframes][n/2+1] tensors: entry b is what cross(xys[b]) gives (glfer_hip_mtm_cross_batch_device)."""
        torch = _torch()
        v = self._iq_view(xys, 1)
        nb, ns = v.size(0), v.size(1)
        assert nb <= 1 or v.stride(0) % 2 == 0, v.stride()
        spitch = v.stride(0) // 2 if nb > 1 else ns
        if nframes is None:
            nframes = self.num_frames(ns) - first_frame
        ts, pitch, xpitch = self._cross_outs(want, out, (nb,), nframes, v.device)
        st = C.c_void_p(torch.cuda.current_stream(v.device).cuda_stream)
        _check(lib().glfer_hip_mtm_cross_batch_device(self._h, C.c_void_p(v.data_ptr()), nb, spitch, ns, first_frame, nframes,
                                                      self._cross_ptr(ts, "sxx"), self._cross_ptr(ts, "syy"), self._cross_ptr(ts, "coh"),
                                                      pitch, self._cross_ptr(ts, "sxy"), xpitch, st), "glfer_hip_mtm_cross_batch_device")
        return Cross(*(ts.get(k) for k in CROSS_FIELDS))

    def _adaptive_outs(self, want, out, lead, nframes, device, fields=ADAPTIVE_FIELDS):
        """The outputs of an adaptive (fields: a jackknife) call as (tensors by name, row pitch): made here, or the caller's (out:
        a mapping or an Adaptive tuple of float32 tensors [lead..., nframes, n/2+1] whose row stride may be larger; they share
        one)."""
        torch = _torch()
        want = tuple(want)
        assert want and all(w in fields for w in want), want
        bins = self.n // 2 + 1
        shape = tuple(lead) + (nframes, bins)
        if out is not None and not isinstance(out, dict):
            out = out._asdict()
        ts, pitches = {}, set()
        for name in want:
            o = None if out is None else out.get(name)
            if o is None:
                ts[name] = torch.empty(shape, dtype=torch.float32, device=device)
                pitches.add(bins)
                continue
            assert o.is_cuda and o.dtype == torch.float32 and tuple(o.shape) == shape, (name, tuple(o.shape), shape)
            assert o.stride(-1) == 1 or o.size(-1) <= 1
            pitch = o.stride(-2) if o.size(-2) > 1 else bins
            assert pitch >= bins
            if lead and o.size(0) > 1:
                assert o.stride(0) == nframes * pitch, "batch rows lie (b * nframes + i) rows from the first"
            pitches.add(pitch)
            ts[name] = o
        assert len(pitches) == 1, "psd and dof share one row pitch"
        return ts, pitches.pop()

    def adaptive(self, stream, first_frame=0, nframes=None, iters=8, want=("psd", "dof"), out=None):
        """stream: 1-D torch tensor on this GPU, of the plan's sample dtype; the plan is a multitaper one with 2 .. 8 tapers.
        Returns Adaptive(psd, dof) with None for what `want` does not name, float32 [nframes][n/2+1]: Thomson's adaptively
        weighted estimate after exactly `iters` sweeps -- a weighted MEAN of the eigenspectra, where run() gives a weighted
        sum -- and its degrees of freedom, 2 .. 2 K.  One launch on torch's current stream (glfer_hip_mtm_adaptive_device)."""
        torch = _torch()
        assert stream.is_cuda and stream.dim() == 1 and stream.is_contiguous()
        assert stream.dtype == self._sample_dtype(), (stream.dtype, self._sample_dtype())
        if nframes is None:
            nframes = self.num_frames(stream.numel()) - first_frame
        ts, pitch = self._adaptive_outs(want, out, (), nframes, stream.device)
        st = C.c_void_p(torch.cuda.current_stream(stream.device).cuda_stream)
        _check(lib().glfer_hip_mtm_adaptive_device(self._h, C.c_void_p(stream.data_ptr()), stream.numel(), first_frame, nframes,
                                                   self._cross_ptr(ts, "psd"), self._cross_ptr(ts, "dof"), pitch, iters, st),
               "glfer_hip_mtm_adaptive_device")
        return Adaptive(*(ts.get(k) for k in ADAPTIVE_FIELDS))

    def adaptive_batch(self, streams, first_frame=0, nframes=None, iters=8, want=("psd", "dof"), out=None):
        """streams: 2-D torch tensor [B, T] as run_batch takes it.  Returns Adaptive of [B][nframes][n/2+1] tensors: entry b is
        what adaptive(streams[b]) gives (glfer_hip_mtm_adaptive_batch_device)."""
        torch = _torch()
        assert streams.is_cuda and streams.dim() == 2 and (streams.stride(1) == 1 or streams.size(1) <= 1)
        assert streams.dtype == self._sample_dtype(), (streams.dtype, self._sample_dtype())
        nb, total = streams.size(0), streams.size(1)
        if nframes is None:
            nframes = self.num_frames(total) - first_frame
        ts, pitch = self._adaptive_outs(want, out, (nb,), nframes, streams.device)
        st = C.c_void_p(torch.cuda.current_stream(streams.device).cuda_stream)
        _check(lib().glfer_hip_mtm_adaptive_batch_device(self._h, C.c_void_p(streams.data_ptr()), nb, streams.stride(0), total,
                                                         first_frame, nframes, self._cross_ptr(ts, "psd"), self._cross_ptr(ts, "dof"),
                                                         pitch, iters, st), "glfer_hip_mtm_adaptive_batch_device")
        return Adaptive(*(ts.get(k) for k in ADAPTIVE_FIELDS))

    def jackknife(self, stream, first_frame=0, nframes=None, iters=8, want=JACKKNIFE_FIELDS, out=None):
        """stream and plan as adaptive() takes them.  Returns Jackknife(psd, dof, logvar) with None for what `want` does not name,
        float32 [nframes][n/2+1]: logvar is the delete-one jackknife variance of ln psd over the K tapers with the weights of
        the last sweep held fixed (0 on a silent frame, +inf where a delete-one estimate is 0, never NaN); psd and dof are the
        bits of adaptive() at the same `iters`.  iters = 0: no sweeps, the eigenvalue-weighted mean and its interval at close to
        run()'s cost.  jackknife_interval turns a result into bounds.  One launch on torch's current stream
        (glfer_hip_mtm_jackknife_device)."""
        torch = _torch()
        assert stream.is_cuda and stream.dim() == 1 and stream.is_contiguous()
        assert stream.dtype == self._sample_dtype(), (stream.dtype, self._sample_dtype())
        if nframes is None:
            nframes = self.num_frames(stream.numel()) - first_frame
        ts, pitch = self._adaptive_outs(want, out, (), nframes, stream.device, JACKKNIFE_FIELDS)
        st = C.c_void_p(torch.cuda.current_stream(stream.device).cuda_stream)
        _check(lib().glfer_hip_mtm_jackknife_device(self._h, C.c_void_p(stream.data_ptr()), stream.numel(), first_frame, nframes,
                                                    self._cross_ptr(ts, "psd"), self._cross_ptr(ts, "dof"),
                                                    self._cross_ptr(ts, "logvar"), pitch, iters, st),
               "glfer_hip_mtm_jackknife_device")
        return Jackknife(*(ts.get(k) for k in JACKKNIFE_FIELDS))

    def jackknife_batch(self, streams, first_frame=0, nframes=None, iters=8, want=JACKKNIFE_FIELDS, out=None):
        """streams: 2-D torch tensor [B, T] as run_batch takes it.  Returns Jackknife of [B][nframes][n/2+1] tensors: entry b is
        what jackknife(streams[b]) gives (glfer_hip_mtm_jackknife_batch_device)."""
        torch = _torch()
        assert streams.is_cuda and streams.dim() == 2 and (streams.stride(1) == 1 or streams.size(1) <= 1)
        assert streams.dtype == self._sample_dtype(), (streams.dtype, self._sample_dtype())
        nb, total = streams.size(0), streams.size(1)
        if nframes is None:
            nframes = self.num_frames(total) - first_frame
        ts, pitch = self._adaptive_outs(want, out, (nb,), nframes, streams.device, JACKKNIFE_FIELDS)
        st = C.c_void_p(torch.cuda.current_stream(streams.device).cuda_stream)
        _check(lib().glfer_hip_mtm_jackknife_batch_device(self._h, C.c_void_p(streams.data_ptr()), nb, streams.stride(0), total,
                                                          first_frame, nframes, self._cross_ptr(ts, "psd"),
                                                          self._cross_ptr(ts, "dof"), self._cross_ptr(ts, "logvar"), pitch, iters,
                                                          st), "glfer_hip_mtm_jackknife_batch_device")
        return Jackknife(*(ts.get(k) for k in JACKKNIFE_FIELDS))

    def welch_rows(self, nsamples, segments, step=None, first_frame=0):
        """Rows cross_welch gives for a stream of nsamples pairs: (frames - first_frame - segments) // step + 1, or 0."""
        return lib().glfer_hip_welch_rows(self._h, nsamples, first_frame, segments, segments if step is None else step)

    def cross_welch(self, xy, segments, step=None, first_frame=0, nrows=None, want=("coh", "sxy"), out=None):
        """Welch's estimate of what cross gives: row r averages |X|^2, |Y|^2 and X conj(Y) over the `segments` consecutive frames
        from first_frame + r * step (step=None: segments, the block average; smaller: a moving estimate), then takes the quotient.
        The plan is an FFT one with any window, or a multitaper one (all its tapers in every segment); xy and the returned
        Cross([nrows][n/2+1]) as cross.  One launch on torch's current stream (glfer_hip_welch_cross_device)."""
        torch = _torch()
        v = self._iq_view(xy, 0)
        ns = v.size(0)
        step = segments if step is None else step
        if nrows is None:
            nrows = self.welch_rows(ns, segments, step, first_frame)
        ts, pitch, xpitch = self._cross_outs(want, out, (), nrows, v.device)
        st = C.c_void_p(torch.cuda.current_stream(v.device).cuda_stream)
        _check(lib().glfer_hip_welch_cross_device(self._h, C.c_void_p(v.data_ptr()), ns, first_frame, segments, step, nrows,
                                                  self._cross_ptr(ts, "sxx"), self._cross_ptr(ts, "syy"), self._cross_ptr(ts, "coh"), pitch,
                                                  self._cross_ptr(ts, "sxy"), xpitch, st), "glfer_hip_welch_cross_device")
        return Cross(*(ts.get(k) for k in CROSS_FIELDS))

    def cross_welch_batch(self, xys, segments, step=None, first_frame=0, nrows=None, want=("coh", "sxy"), out=None):
        """xys as cross_batch takes them.  Returns Cross of [B][nrows][n/2+1] tensors: entry b is what cross_welch(xys[b], ...)
        gives (glfer_hip_welch_cross_batch_device)."""
        torch = _torch()
        v = self._iq_view(xys, 1)
        nb, ns = v.size(0), v.size(1)
        assert nb <= 1 or v.stride(0) % 2 == 0, v.stride()
        spitch = v.stride(0) // 2 if nb > 1 else ns
        step = segments if step is None else step
        if nrows is None:
            nrows = self.welch_rows(ns, segments, step, first_frame)
        ts, pitch, xpitch = self._cross_outs(want, out, (nb,), nrows, v.device)
        st = C.c_void_p(torch.cuda.current_stream(v.device).cuda_stream)
        _check(lib().glfer_hip_welch_cross_batch_device(self._h, C.c_void_p(v.data_ptr()), nb, spitch, ns, first_frame, segments, step,
                                                        nrows, self._cross_ptr(ts, "sxx"), self._cross_ptr(ts, "syy"),
                                                        self._cross_ptr(ts, "coh"), pitch, self._cross_ptr(ts, "sxy"), xpitch, st),
               "glfer_hip_welch_cross_batch_device")
        return Cross(*(ts.get(k) for k in CROSS_FIELDS))

    def run_zoom(self, ddc, x, first_frame=0, nframes=None, out=None, centered=False):
        """The two-sided rows of run_iq over ddc.run(x), bit for bit, without the caller holding the baseband: x is what ddc.run
        takes, the plan has the f32 sample format, frames count the ddc.num_out(len(x)) baseband samples.  Two kernels, the
        baseband in stream-ordered scratch; not under graph capture (glfer_hip_spectrogram_zoom_device)."""
        torch = _torch()
        v, ns, _ = ddc._view(x, 0)
        if nframes is None:
            nframes = self.num_frames(ddc.num_out(ns)) - first_frame
        out, pitch = self._iq_out(out, (nframes, self.n), v.device)
        st = C.c_void_p(torch.cuda.current_stream(v.device).cuda_stream)
        _check(lib().glfer_hip_spectrogram_zoom_device(self._h, ddc._h, C.c_void_p(v.data_ptr()), ns, first_frame, nframes,
                                                       C.c_void_p(out.data_ptr()), pitch, IQ_CENTERED if centered else 0, st),
               "glfer_hip_spectrogram_zoom_device")
        return out

    def run_drift(self, stream, frames, step=None, dmin=None, dmax=None, first_frame=0, nblocks=None, want=("best", "drift"), out=None):
        """drift_sums over the plan's rows of `stream` (what run takes) without the caller holding them: block b is frames
        first_frame + b step .. + frames - 1; nblocks defaults to every block that fits behind first_frame.  Returns Drift(sums,
        best, drift), bit for bit drift_sums(run(stream, first_frame, ...), ...); the rows go through stream-ordered scratch in
        pieces of whole blocks, so not under graph capture (glfer_hip_spectrogram_drift_device)."""
        torch = _torch()
        if not (stream.is_cuda and stream.dim() == 1 and stream.is_contiguous() and stream.dtype == self._sample_dtype()):
            raise ValueError("stream: a contiguous 1-D tensor of the plan's sample dtype on the GPU")
        frames, step, dmin, dmax = _drift_args(frames, step, dmin, dmax)
        first_frame = int(first_frame)
        total = self.num_frames(stream.numel())
        if first_frame < 0 or first_frame > total:
            raise ValueError("first_frame: 0 .. the stream's frames")
        fit = drift_blocks(total - first_frame, frames, step)
        nblocks = fit if nblocks is None else int(nblocks)
        if nblocks < 0 or nblocks > fit:
            raise ValueError("nblocks: at most the %d blocks behind first_frame" % fit)
        ts = _drift_outs(want, out, (), nblocks, dmax - dmin + 1, self.bins, stream.device)
        st = C.c_void_p(torch.cuda.current_stream(stream.device).cuda_stream)
        _check(lib().glfer_hip_spectrogram_drift_device(self._h, C.c_void_p(stream.data_ptr()), stream.numel(), first_frame, frames, step,
                                                        nblocks, dmin, dmax, *(_drift_ptr(ts, k) for k in DRIFT_FIELDS), st),
               "glfer_hip_spectrogram_drift_device")
        return Drift(*(ts.get(k) for k in DRIFT_FIELDS))

    def run_channels(self, samples, channels=None, select=None, first_frame=0, nframes=None, out=None):
        """samples: an interleaved recording on this GPU, of the plan's sample dtype -- a 1-D tensor (`channels` says how many
        channels it holds) or a contiguous [S][C] tensor (channels = C).  select: channel indices (duplicates allowed; None =
        all, in order).  Returns psd [nselect][nframes][pitch] -- out[j] is what run() gives on a contiguous copy of channel
        select[j] -- launched on torch's current stream (glfer_hip_spectrogram_channels_device)."""
        torch = _torch()
        assert samples.is_cuda and samples.is_contiguous() and samples.dim() in (1, 2)
        assert samples.dtype == self._sample_dtype(), (samples.dtype, self._sample_dtype())
        if samples.dim() == 2:
            assert channels is None or channels == samples.size(1)
            channels = samples.size(1)
        assert channels is not None and channels >= 1 and samples.numel() % channels == 0
        per = samples.numel() // channels
        sel, nsel = _selection(channels, select)
        if nframes is None:
            nframes = self.num_frames(per) - first_frame
        if out is None:
            out = torch.empty((nsel, nframes, self.pitch), dtype=torch.float32, device=samples.device)
        assert out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.numel() >= nsel * nframes * self.pitch
        st = C.c_void_p(torch.cuda.current_stream(samples.device).cuda_stream)
        _check(lib().glfer_hip_spectrogram_channels_device(self._h, C.c_void_p(samples.data_ptr()), per, channels, sel, nsel,
                                                           first_frame, nframes, C.c_void_p(out.data_ptr()), st),
               "glfer_hip_spectrogram_channels_device")
        return out

    def run_host_channels(self, samples, channels, select=None, pinned=False):
        """samples: an interleaved recording on the host (numpy, 1-D or [S][C]); returns numpy psd [nselect][frames][bins],
        plane j the rows run_host gives on channel select[j].  One pass through the chunk ring
        (glfer_hip_spectrogram_host_channels).  pinned=True: the rows come back in pinned memory."""
        want = {SAMPLES_F32: np.float32, SAMPLES_S16: np.int16, SAMPLES_U8: np.uint8}[self.params.sample_format]
        samples = np.ascontiguousarray(samples, want)
        assert samples.size % channels == 0
        per = samples.size // channels
        sel, nsel = _selection(channels, select)
        frames = self.num_frames(per)
        shape = (nsel, frames, self.bins)
        out = pinned_empty(shape, np.float32) if pinned and frames else np.empty(shape, np.float32)
        nf = C.c_size_t(0)
        _check(lib().glfer_hip_spectrogram_host_channels(self._h, samples.ctypes.data, per, channels, sel, nsel, out.ctypes.data,
                                                         C.byref(nf)), "glfer_hip_spectrogram_host_channels")
        assert nf.value == frames
        return out

    def run_wav_channels(self, path, select=None, chunk_frames=0, max_frames=None):
        """A multi-channel WAV file -> numpy psd [nselect][frames][bins]: the file's channels (from its header) as streams of
        their own, one pass over the file (glfer_hip_spectrogram_wav_channels).  run_wav keeps reading such a file as one
        stream of interleaved samples, as the reference does."""
        info = wav_probe(path)
        sel, nsel = _selection(info.channels, select)
        frames = (info.data_bytes // (info.channels * (info.bits_per_sample // 8))) // self.hop
        if max_frames is not None:
            frames = min(frames, max_frames)
        out = np.empty((nsel, frames, self.bins), np.float32)
        nf = C.c_size_t(0)
        _check(lib().glfer_hip_spectrogram_wav_channels(self._h, os.fsencode(path), sel, nsel, out.ctypes.data, frames,
                                                        C.byref(nf), chunk_frames), "glfer_hip_spectrogram_wav_channels")
        assert nf.value == frames
        return out

    def ragged_frames(self, lengths):
        """(total rows, row_starts int64 [len(lengths) + 1]) of a ragged call over streams of these lengths, in samples
        (glfer_hip_ragged_frames; no device involved)."""
        lens = np.ascontiguousarray(lengths, dtype=np.uint64).reshape(-1)
        starts = np.zeros(lens.size + 1, np.uint64)
        total = lib().glfer_hip_ragged_frames(self._h, lens.size, lens.ctypes.data, starts.ctypes.data)
        return int(total), starts.astype(np.int64)

    def run_ragged(self, samples, offsets, lengths, out=None):
        """Streams of unequal length in one call (glfer_hip_spectrogram_ragged_device).  samples: 1-D torch tensor of the plan's
        sample dtype on this GPU; stream b is samples[offsets[b] : offsets[b] + lengths[b]] (any order, gaps and overlaps
        allowed; even offsets for s16 / u8).  Returns (psd [sum of frames][pitch], row_starts): stream b's rows are
        psd[row_starts[b] : row_starts[b + 1]] and equal run(samples[offsets[b] : offsets[b] + lengths[b]]); row_starts is a
        numpy int64 array of len(offsets) + 1.  Launched on torch's current stream."""
        torch = _torch()
        assert samples.is_cuda and samples.dim() == 1 and samples.is_contiguous()
        assert samples.dtype == self._sample_dtype(), (samples.dtype, self._sample_dtype())
        offs = np.ascontiguousarray(offsets, dtype=np.uint64).reshape(-1)
        lens = np.ascontiguousarray(lengths, dtype=np.uint64).reshape(-1)
        assert offs.size == lens.size
        total, _ = self.ragged_frames(lens)
        if total == 2 ** 64 - 1:
            raise GlferHipError("run_ragged: the row count overflows")
        # (a stream past the tensor's end is the caller's error, as in C; checked here because it is cheap)
        if lens.size:
            assert max(int(o) + int(n) for o, n in zip(offs, lens)) <= samples.numel(), "a stream reaches past `samples`"
        if out is None:
            out = torch.empty((total, self.pitch), dtype=torch.float32, device=samples.device)
        assert out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.numel() >= total * self.pitch
        starts = np.zeros(lens.size + 1, np.uint64)
        st = C.c_void_p(torch.cuda.current_stream(samples.device).cuda_stream)
        _check(lib().glfer_hip_spectrogram_ragged_device(self._h, C.c_void_p(samples.data_ptr()), lens.size, offs.ctypes.data,
                                                         lens.ctypes.data, C.c_void_p(out.data_ptr()), starts.ctypes.data, st),
               "glfer_hip_spectrogram_ragged_device")
        return out, starts.astype(np.int64)

    def run_list(self, streams):
        """streams: a list of 1-D torch tensors of the plan's sample dtype on this GPU.  Concatenates them on the device (every
        stream at an even offset, which the integer formats need) and returns the list of per-stream row views
        [frames_b][pitch] of one run_ragged call."""
        buf, offs, lens = self._pack_list(streams)
        psd, starts = self.run_ragged(buf, offs, lens)
        return [psd[int(starts[b]):int(starts[b + 1])] for b in range(len(streams))]

    def run_avg_ragged(self, samples, offsets, lengths, avg_mode, depth, minbin, maxbin, max0=0, n_out=None, want_psd=False,
                       want_ret=True):
        """run_avg for streams of unequal length in one call (glfer_hip_spectrogram_avg_ragged_device).  samples, offsets and
        lengths as run_ragged takes them.  Returns (avg [sum of frames][n_out] float64, ret [sum of frames][4] float64 or None,
        psd [sum of frames][bins] float32 or None, row_starts): stream b's rows are [row_starts[b], row_starts[b + 1]) of each
        and equal run() followed by update_avg() on that stream."""
        torch = _torch()
        if samples.dim() != 1 or samples.dtype != self._sample_dtype():
            raise ValueError("samples: a 1-D tensor of the plan's sample dtype")
        if not (samples.is_cuda and samples.is_contiguous()):
            raise ValueError("samples: contiguous, on the GPU")
        offs = np.ascontiguousarray(offsets, dtype=np.uint64).reshape(-1)
        lens = np.ascontiguousarray(lengths, dtype=np.uint64).reshape(-1)
        if offs.size != lens.size:
            raise ValueError("one offset and one length per stream")
        total, _ = self.ragged_frames(lens)
        if total == 2 ** 64 - 1:
            raise GlferHipError("run_avg_ragged: the row count overflows")
        if lens.size and max(int(o) + int(n) for o, n in zip(offs, lens)) > samples.numel():
            raise ValueError("a stream reaches past `samples`")
        n_out = n_out or self.bins
        dev = samples.device
        avg = torch.empty((total, n_out), dtype=torch.float64, device=dev)
        ret = torch.empty((total, 4), dtype=torch.float64, device=dev) if want_ret else None
        psd = torch.empty((total, self.bins), dtype=torch.float32, device=dev) if want_psd else None
        starts = np.zeros(lens.size + 1, np.uint64)
        st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        _check(lib().glfer_hip_spectrogram_avg_ragged_device(self._h, C.c_void_p(samples.data_ptr()), lens.size, offs.ctypes.data,
                                                             lens.ctypes.data, int(avg_mode), int(depth), int(minbin), int(maxbin),
                                                             int(max0), int(n_out), C.c_void_p(psd.data_ptr() if want_psd else None),
                                                             C.c_void_p(avg.data_ptr()), C.c_void_p(ret.data_ptr() if want_ret else None),
                                                             starts.ctypes.data, st),
               "glfer_hip_spectrogram_avg_ragged_device")
        return avg, ret, psd, starts.astype(np.int64)

    def run_avg(self, stream, avg_mode, depth, minbin, maxbin, max0=0, n_out=None, want_psd=False, want_ret=True,
                first_frame=0, nframes=None):
        """fft_do + fft_psd + update_avg_* in one call (glfer_hip_spectrogram_avg_device): returns (avg [nframes][n_out] float64,
        ret [nframes][4] float64 or None, psd [nframes][bins] float32 or None)."""
        torch = _torch()
        assert stream.is_cuda and stream.dim() == 1 and stream.is_contiguous() and stream.dtype == self._sample_dtype()
        if nframes is None:
            nframes = self.num_frames(stream.numel()) - first_frame
        n_out = n_out or self.bins
        avg = torch.empty((nframes, n_out), dtype=torch.float64, device=stream.device)
        ret = torch.empty((nframes, 4), dtype=torch.float64, device=stream.device) if want_ret else None
        psd = torch.empty((nframes, self.bins), dtype=torch.float32, device=stream.device) if want_psd else None
        st = C.c_void_p(torch.cuda.current_stream(stream.device).cuda_stream)
        _check(lib().glfer_hip_spectrogram_avg_device(self._h, C.c_void_p(stream.data_ptr()), stream.numel(), first_frame, nframes,
                                                      int(avg_mode), int(depth), int(minbin), int(maxbin), int(max0), int(n_out),
                                                      C.c_void_p(psd.data_ptr() if want_psd else None), C.c_void_p(avg.data_ptr()),
                                                      C.c_void_p(ret.data_ptr() if want_ret else None), st),
               "glfer_hip_spectrogram_avg_device")
        return avg, ret, psd

    def run_avg_batch(self, streams, avg_mode, depth, minbin, maxbin, max0=0, n_out=None, want_psd=False, want_ret=True,
                      first_frame=0, nframes=None):
        """run_avg for many streams in one call (glfer_hip_spectrogram_avg_batch_device).  streams as run_batch takes them: 2-D
        [B, T] on this GPU, of the plan's sample dtype, stride(1) == 1.  Returns (avg [B][nframes][n_out] float64, ret
        [B][nframes][4] float64 or None, psd [B][nframes][bins] float32 or None); stream b's outputs are run_avg(streams[b])'s,
        launched on torch's current stream."""
        torch = _torch()
        assert streams.is_cuda and streams.dim() == 2 and (streams.stride(1) == 1 or streams.size(1) <= 1)
        assert streams.dtype == self._sample_dtype(), (streams.dtype, self._sample_dtype())
        nb, total = streams.size(0), streams.size(1)
        if nframes is None:
            nframes = self.num_frames(total) - first_frame
        n_out = n_out or self.bins
        dev = streams.device
        avg = torch.empty((nb, nframes, n_out), dtype=torch.float64, device=dev)
        ret = torch.empty((nb, nframes, 4), dtype=torch.float64, device=dev) if want_ret else None
        psd = torch.empty((nb, nframes, self.bins), dtype=torch.float32, device=dev) if want_psd else None
        st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        _check(lib().glfer_hip_spectrogram_avg_batch_device(self._h, C.c_void_p(streams.data_ptr()), nb, streams.stride(0), total,
                                                            first_frame, nframes, int(avg_mode), int(depth), int(minbin), int(maxbin),
                                                            int(max0), int(n_out), C.c_void_p(psd.data_ptr() if want_psd else None),
                                                            C.c_void_p(avg.data_ptr()), C.c_void_p(ret.data_ptr() if want_ret else None),
                                                            st),
               "glfer_hip_spectrogram_avg_batch_device")
        return avg, ret, psd

    def run_wav(self, path, chunk_frames=0, max_frames=None, partial_tail=False):
        """Whole WAV file -> numpy psd [frames][bins], streamed through pinned buffers.
        partial_tail: also the reference's extra frame for a trailing partial block
        (wav_fmt.c:102-119; GLFER_WAV_PARTIAL_TAIL)."""
        info = wav_probe(path)
        frames = info.nsamples // self.hop + (1 if partial_tail else 0)
        if max_frames is not None:
            frames = min(frames, max_frames)
        out = np.empty((frames, self.bins), np.float32)
        nf = C.c_size_t(0)
        _check(lib().glfer_hip_spectrogram_wav_ex(self._h, os.fsencode(path), out.ctypes.data, frames,
                                                  C.byref(nf), chunk_frames, WAV_PARTIAL_TAIL if partial_tail else 0),
               "glfer_hip_spectrogram_wav_ex")
        return out[:nf.value]

    def ftest(self, stream, first_frame=0, nframes=None, mu_live=True):
        """The harmonic F statistic of mtm_do (mtm.c:165-174, 203-233) for every frame: a float
        tensor [nframes][bins].  mu_live=False restates the reference build without FFTW."""
        torch = _torch()
        assert stream.is_cuda and stream.dim() == 1 and stream.is_contiguous()
        assert stream.dtype == self._sample_dtype()
        if nframes is None:
            nframes = self.num_frames(stream.numel()) - first_frame
        out = torch.empty((nframes, self.bins), dtype=torch.float32, device=stream.device)
        st = C.c_void_p(torch.cuda.current_stream(stream.device).cuda_stream)
        _check(lib().glfer_hip_mtm_ftest_device(self._h, stream.data_ptr(), stream.numel(), first_frame, nframes,
                                                out.data_ptr(), 1 if mu_live else 0, st), "glfer_hip_mtm_ftest_device")
        return out

    def ftest_batch(self, streams, first_frame=0, nframes=None, mu_live=True, out=None):
        """ftest for many streams in one call (glfer_hip_mtm_ftest_batch_device).  streams as run_batch takes them: 2-D [B, T]
        on this GPU, of the plan's sample dtype, stride(1) == 1 (stride(0) is the distance between streams, in samples).
        Returns a float tensor [B][nframes][bins] -- out[b] holds the bits of ftest(streams[b]) -- launched on torch's
        current stream."""
        torch = _torch()
        assert streams.is_cuda and streams.dim() == 2 and (streams.stride(1) == 1 or streams.size(1) <= 1)
        assert streams.dtype == self._sample_dtype(), (streams.dtype, self._sample_dtype())
        nb, total = streams.size(0), streams.size(1)
        if nframes is None:
            nframes = self.num_frames(total) - first_frame
        if out is None:
            out = torch.empty((nb, nframes, self.bins), dtype=torch.float32, device=streams.device)
        assert out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.numel() >= nb * nframes * self.bins
        st = C.c_void_p(torch.cuda.current_stream(streams.device).cuda_stream)
        _check(lib().glfer_hip_mtm_ftest_batch_device(self._h, C.c_void_p(streams.data_ptr()), nb, streams.stride(0), total,
                                                      first_frame, nframes, C.c_void_p(out.data_ptr()), 1 if mu_live else 0, st),
               "glfer_hip_mtm_ftest_batch_device")
        return out

    def rows_ftest(self, stream, first_frame=0, nframes=None, mu_live=True, out=None):
        """The multitaper rows and the harmonic F rows of the same frames from one pass over the samples
        (glfer_hip_mtm_rows_ftest_device): (psd [nframes][pitch], ftest [nframes][bins]).  The F rows hold the bits of
        ftest(stream, ...); the PSD rows are run(stream, ...)'s to float rounding.  out: a (psd, ftest) pair to write into.
        stream as ftest takes it; launched on torch's current stream."""
        torch = _torch()
        assert stream.is_cuda and stream.dim() == 1 and stream.is_contiguous()
        assert stream.dtype == self._sample_dtype(), (stream.dtype, self._sample_dtype())
        if nframes is None:
            nframes = self.num_frames(stream.numel()) - first_frame
        if out is None:
            out = (torch.empty((nframes, self.pitch), dtype=torch.float32, device=stream.device),
                   torch.empty((nframes, self.bins), dtype=torch.float32, device=stream.device))
        psd, ft = out
        for o, w in ((psd, self.pitch), (ft, self.bins)):
            assert o.is_cuda and o.dtype == torch.float32 and o.is_contiguous() and o.numel() >= nframes * w
        st = C.c_void_p(torch.cuda.current_stream(stream.device).cuda_stream)
        _check(lib().glfer_hip_mtm_rows_ftest_device(self._h, C.c_void_p(stream.data_ptr()), stream.numel(), first_frame, nframes,
                                                     C.c_void_p(psd.data_ptr()), C.c_void_p(ft.data_ptr()), 1 if mu_live else 0, st),
               "glfer_hip_mtm_rows_ftest_device")
        return psd, ft

    def rows_ftest_batch(self, streams, first_frame=0, nframes=None, mu_live=True, out=None):
        """rows_ftest for many streams in one call (glfer_hip_mtm_rows_ftest_batch_device).  streams as ftest_batch takes them:
        2-D [B, T] on this GPU, of the plan's sample dtype, stride(1) == 1.  Returns (psd [B][nframes][pitch],
        ftest [B][nframes][bins]); both hold, for stream b, the bits of rows_ftest(streams[b])."""
        torch = _torch()
        assert streams.is_cuda and streams.dim() == 2 and (streams.stride(1) == 1 or streams.size(1) <= 1)
        assert streams.dtype == self._sample_dtype(), (streams.dtype, self._sample_dtype())
        nb, total = streams.size(0), streams.size(1)
        if nframes is None:
            nframes = self.num_frames(total) - first_frame
        if out is None:
            out = (torch.empty((nb, nframes, self.pitch), dtype=torch.float32, device=streams.device),
                   torch.empty((nb, nframes, self.bins), dtype=torch.float32, device=streams.device))
        psd, ft = out
        for o, w in ((psd, self.pitch), (ft, self.bins)):
            assert o.is_cuda and o.dtype == torch.float32 and o.is_contiguous() and o.numel() >= nb * nframes * w
        st = C.c_void_p(torch.cuda.current_stream(streams.device).cuda_stream)
        _check(lib().glfer_hip_mtm_rows_ftest_batch_device(self._h, C.c_void_p(streams.data_ptr()), nb, streams.stride(0), total,
                                                           first_frame, nframes, C.c_void_p(psd.data_ptr()), C.c_void_p(ft.data_ptr()),
                                                           1 if mu_live else 0, st),
               "glfer_hip_mtm_rows_ftest_batch_device")
        return psd, ft

    def _ragged_args(self, what, samples, offsets, lengths):
        """run_ragged's validation for the ragged F entries: (offsets uint64, lengths uint64, total rows)"""
        assert samples.is_cuda and samples.dim() == 1 and samples.is_contiguous()
        assert samples.dtype == self._sample_dtype(), (samples.dtype, self._sample_dtype())
        offs = np.ascontiguousarray(offsets, dtype=np.uint64).reshape(-1)
        lens = np.ascontiguousarray(lengths, dtype=np.uint64).reshape(-1)
        assert offs.size == lens.size
        total, _ = self.ragged_frames(lens)
        if total == 2 ** 64 - 1:
            raise GlferHipError(what + ": the row count overflows")
        if lens.size:
            assert max(int(o) + int(n) for o, n in zip(offs, lens)) <= samples.numel(), "a stream reaches past `samples`"
        return offs, lens, total

    def ftest_ragged(self, samples, offsets, lengths, mu_live=True, out=None):
        """ftest for streams of unequal length in one call (glfer_hip_mtm_ftest_ragged_device).  samples, offsets and lengths
        as run_ragged takes them.  Returns (ftest [sum of frames][bins], row_starts): stream b's rows are
        ftest[row_starts[b] : row_starts[b + 1]] and hold the bits of ftest(samples[offsets[b] : offsets[b] + lengths[b]]);
        row_starts is a numpy int64 array of len(offsets) + 1.  Launched on torch's current stream."""
        torch = _torch()
        offs, lens, total = self._ragged_args("ftest_ragged", samples, offsets, lengths)
        if out is None:
            out = torch.empty((total, self.bins), dtype=torch.float32, device=samples.device)
        assert out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.numel() >= total * self.bins
        starts = np.zeros(lens.size + 1, np.uint64)
        st = C.c_void_p(torch.cuda.current_stream(samples.device).cuda_stream)
        _check(lib().glfer_hip_mtm_ftest_ragged_device(self._h, C.c_void_p(samples.data_ptr()), lens.size, offs.ctypes.data,
                                                       lens.ctypes.data, C.c_void_p(out.data_ptr()), 1 if mu_live else 0,
                                                       starts.ctypes.data, st),
               "glfer_hip_mtm_ftest_ragged_device")
        return out, starts.astype(np.int64)

    def rows_ftest_ragged(self, samples, offsets, lengths, mu_live=True, out=None):
        """rows_ftest for streams of unequal length in one call (glfer_hip_mtm_rows_ftest_ragged_device).  Returns
        (psd [sum of frames][pitch], ftest [sum of frames][bins], row_starts); rows row_starts[b] : row_starts[b + 1] of both
        hold the bits of rows_ftest(samples[offsets[b] : offsets[b] + lengths[b]]).  out: a (psd, ftest) pair to write into."""
        torch = _torch()
        offs, lens, total = self._ragged_args("rows_ftest_ragged", samples, offsets, lengths)
        if out is None:
            out = (torch.empty((total, self.pitch), dtype=torch.float32, device=samples.device),
                   torch.empty((total, self.bins), dtype=torch.float32, device=samples.device))
        psd, ft = out
        for o, w in ((psd, self.pitch), (ft, self.bins)):
            assert o.is_cuda and o.dtype == torch.float32 and o.is_contiguous() and o.numel() >= total * w
        starts = np.zeros(lens.size + 1, np.uint64)
        st = C.c_void_p(torch.cuda.current_stream(samples.device).cuda_stream)
        _check(lib().glfer_hip_mtm_rows_ftest_ragged_device(self._h, C.c_void_p(samples.data_ptr()), lens.size, offs.ctypes.data,
                                                            lens.ctypes.data, C.c_void_p(psd.data_ptr()), C.c_void_p(ft.data_ptr()),
                                                            1 if mu_live else 0, starts.ctypes.data, st),
               "glfer_hip_mtm_rows_ftest_ragged_device")
        return psd, ft, starts.astype(np.int64)

    def _pack_list(self, streams):
        """run_list's packing: the streams concatenated on the device at even offsets: (buffer, offsets, lengths)"""
        torch = _torch()
        assert len(streams) > 0
        offs, at = [], 0
        for t in streams:
            assert t.dim() == 1 and t.dtype == self._sample_dtype()
            offs.append(at)
            at += t.numel() + (t.numel() & 1)
        buf = torch.zeros(max(at, 1), dtype=self._sample_dtype(), device=streams[0].device)
        for o, t in zip(offs, streams):
            buf[o:o + t.numel()] = t
        return buf, offs, [t.numel() for t in streams]

    def ftest_list(self, streams):
        """streams: a list of 1-D torch tensors as run_list takes them.  Returns the list of per-stream F row views
        [frames_b][bins] of one ftest_ragged call."""
        buf, offs, lens = self._pack_list(streams)
        ft, starts = self.ftest_ragged(buf, offs, lens)
        return [ft[int(starts[b]):int(starts[b + 1])] for b in range(len(streams))]

    def rows_ftest_list(self, streams):
        """As ftest_list, from one rows_ftest_ragged call: the list of per-stream (psd [frames_b][pitch], ftest [frames_b][bins])."""
        buf, offs, lens = self._pack_list(streams)
        psd, ft, starts = self.rows_ftest_ragged(buf, offs, lens)
        return [(psd[int(starts[b]):int(starts[b + 1])], ft[int(starts[b]):int(starts[b + 1])]) for b in range(len(streams))]

    def prepare(self, stream, first_frame=0, nframes=None):
        """prepare_audio's inbuf_fft (fft.c:66-165) for every frame: float tensor [nframes][n]."""
        torch = _torch()
        assert stream.is_cuda and stream.dim() == 1 and stream.is_contiguous()
        assert stream.dtype == self._sample_dtype()
        if nframes is None:
            nframes = self.num_frames(stream.numel()) - first_frame
        out = torch.empty((nframes, self.n), dtype=torch.float32, device=stream.device)
        st = C.c_void_p(torch.cuda.current_stream(stream.device).cuda_stream)
        _check(lib().glfer_hip_prepare_device(self._h, stream.data_ptr(), stream.numel(), first_frame, nframes,
                                              out.data_ptr(), st), "glfer_hip_prepare_device")
        return out

    def waterfall_host(self, samples, disp, want_lev=True):
        """Host samples -> (rgb uint8 [frames][bins][3], lev int16 [frames][bins] | None) through the
        chunked ring, mapping done on the device (glfer_hip_waterfall_host)."""
        want = {SAMPLES_F32: np.float32, SAMPLES_S16: np.int16, SAMPLES_U8: np.uint8}[self.params.sample_format]
        samples = np.ascontiguousarray(samples, want)
        frames = self.num_frames(samples.size)
        rgb = np.empty((frames, self.bins, 3), np.uint8)
        lev = np.empty((frames, self.bins), np.int16) if want_lev else None
        nf = C.c_size_t(0)
        _check(lib().glfer_hip_waterfall_host(self._h, C.byref(disp), samples.ctypes.data, samples.size, rgb.ctypes.data,
                                              lev.ctypes.data if want_lev else None, C.byref(nf)), "glfer_hip_waterfall_host")
        assert nf.value == frames
        return rgb, lev

    def run_host(self, samples, pinned=False):
        """samples: numpy array on the host; returns numpy psd [frames][bins].
        pinned=True: the rows come back in pinned memory (glfer_hip_host_alloc; DMA straight into it,
        3-4x the rate of a pageable array); the memory is released when the array is collected."""
        want = {SAMPLES_F32: np.float32, SAMPLES_S16: np.int16, SAMPLES_U8: np.uint8}[
            self.params.sample_format]
        samples = np.ascontiguousarray(samples, want)
        frames = self.num_frames(samples.size)
        out = pinned_empty((frames, self.bins), np.float32) if pinned and frames else np.empty((frames, self.bins), np.float32)
        nf = C.c_size_t(0)
        _check(lib().glfer_hip_spectrogram_host(self._h, samples.ctypes.data, samples.size,
                                                out.ctypes.data, C.byref(nf)),
               "glfer_hip_spectrogram_host")
        assert nf.value == frames
        return out


def _selection(channels, select):
    """(ctypes int array or None, count) of a channel selection for the *_channels entries."""
    if select is None:
        return None, channels
    idx = [int(c) for c in select]
    return (C.c_int * len(idx))(*idx), len(idx)


def deinterleave(samples, channels, select=None, out=None):
    """samples: interleaved recording on a GPU (1-D or contiguous [S][C]) of dtype float32 / int16 / uint8.  Returns the selected
    channels as planes, [nselect][S] (out: a 2-D tensor with stride(1) == 1 and stride(0) >= S), on torch's current stream
    (glfer_hip_deinterleave_device: bytes are moved, never converted)."""
    torch = _torch()
    fmt = {torch.float32: SAMPLES_F32, torch.int16: SAMPLES_S16, torch.uint8: SAMPLES_U8}[samples.dtype]
    assert samples.is_cuda and samples.is_contiguous() and samples.numel() % channels == 0
    per = samples.numel() // channels
    sel, nsel = _selection(channels, select)
    if out is None:
        out = torch.empty((nsel, per), dtype=samples.dtype, device=samples.device)
    assert out.is_cuda and out.dtype == samples.dtype and out.dim() == 2 and out.size(0) == nsel and out.size(1) == per
    assert (out.stride(1) == 1 or per <= 1) and (out.stride(0) >= per or nsel <= 1)
    st = C.c_void_p(torch.cuda.current_stream(samples.device).cuda_stream)
    _check(lib().glfer_hip_deinterleave_device(C.c_void_p(samples.data_ptr()), per, channels, fmt, sel, nsel,
                                               C.c_void_p(out.data_ptr()), out.stride(0) if nsel > 1 else max(out.stride(0), per), st),
           "glfer_hip_deinterleave_device")
    return out


def frame_range(total_frames, rank, world):
    """glfer_hip_frame_range: (first, count) of a rank's contiguous frame block."""
    a, b = C.c_size_t(0), C.c_size_t(0)
    lib().glfer_hip_frame_range(total_frames, rank, world, C.byref(a), C.byref(b))
    return a.value, b.value


def spectrogram_host_multi(params, samples, devices, out=None):
    """glfer_hip_spectrogram_host_multi: one stream on the host, its frames dealt out over
    `devices` (a list of HIP device ordinals), numpy psd [frames][bins] back."""
    want = {SAMPLES_F32: np.float32, SAMPLES_S16: np.int16, SAMPLES_U8: np.uint8}[params.sample_format]
    samples = np.ascontiguousarray(samples, want)
    cfg = make_config(params, 0)
    hop = int(params.n * (1.0 - float(np.float32(params.overlap))))
    frames = samples.size // hop
    if out is None:
        out = np.empty((frames, params.n // 2 + 1), np.float32)
    nf = C.c_size_t(0)
    if len(set(devices)) == len(devices):
        mask = 0
        for d in devices:
            mask |= 1 << d
        _check(lib().glfer_hip_spectrogram_host_multi(C.byref(cfg), mask, samples.ctypes.data, samples.size,
                                                      out.ctypes.data, C.byref(nf)), "glfer_hip_spectrogram_host_multi")
    else:                                   # workers sharing a GPU: glfer_hip_spectrogram_host_workers
        devs = (C.c_int * len(devices))(*devices)
        _check(lib().glfer_hip_spectrogram_host_workers(C.byref(cfg), devs, len(devices), samples.ctypes.data, samples.size,
                                                        out.ctypes.data, C.byref(nf)), "glfer_hip_spectrogram_host_workers")
    return out[:nf.value]


def _hop_of(params):
    return int(params.n * (1.0 - float(np.float32(params.overlap))))


def spectrogram_wav_workers(params, path, devices, partial_tail=False, max_frames=None):
    """glfer_hip_spectrogram_wav_workers / _multi: a WAV file's frames dealt out over `devices` (HIP
    ordinals; one may repeat), every worker reading its own part of the file; numpy psd [frames][bins]."""
    info = wav_probe(path)
    cfg = make_config(params, 0)
    frames = info.nsamples // _hop_of(params) + (1 if partial_tail else 0)
    if max_frames is not None:
        frames = min(frames, max_frames)
    out = np.empty((frames, params.n // 2 + 1), np.float32)
    nf = C.c_size_t(0)
    flags = WAV_PARTIAL_TAIL if partial_tail else 0
    if len(set(devices)) == len(devices):
        mask = 0
        for d in devices:
            mask |= 1 << d
        _check(lib().glfer_hip_spectrogram_wav_multi(C.byref(cfg), mask, os.fsencode(path), out.ctypes.data, frames,
                                                     C.byref(nf), flags), "glfer_hip_spectrogram_wav_multi")
    else:
        devs = (C.c_int * len(devices))(*devices)
        _check(lib().glfer_hip_spectrogram_wav_workers(C.byref(cfg), devs, len(devices), os.fsencode(path), out.ctypes.data,
                                                       frames, C.byref(nf), flags), "glfer_hip_spectrogram_wav_workers")
    return out[:nf.value]


def waterfall_workers(params, disp, devices, samples=None, path=None, avg_mode=0, depth=1, minbin=0, maxbin=1, max0=0,
                      want_lev=True, partial_tail=False):
    """glfer_hip_waterfall_host_workers (samples: numpy array) or glfer_hip_waterfall_wav_workers (path):
    (rgb uint8 [frames][bins][3], lev int16 [frames][bins] | None), the columns dealt out over `devices`."""
    cfg = make_config(params, 0)
    hop, bins = _hop_of(params), params.n // 2 + 1
    devs = (C.c_int * len(devices))(*devices)
    nf = C.c_size_t(0)
    if path is None:
        want = {SAMPLES_F32: np.float32, SAMPLES_S16: np.int16, SAMPLES_U8: np.uint8}[params.sample_format]
        samples = np.ascontiguousarray(samples, want)
        frames = samples.size // hop
    else:
        frames = wav_probe(path).nsamples // hop + (1 if partial_tail else 0)
    rgb = np.empty((frames, bins, 3), np.uint8)
    lev = np.empty((frames, bins), np.int16) if want_lev else None
    levp = lev.ctypes.data if want_lev else None
    if path is None:
        _check(lib().glfer_hip_waterfall_host_workers(C.byref(cfg), devs, len(devices), C.byref(disp), int(avg_mode), depth, minbin,
                                                      maxbin, int(max0), samples.ctypes.data, samples.size, rgb.ctypes.data, levp,
                                                      C.byref(nf)), "glfer_hip_waterfall_host_workers")
    else:
        _check(lib().glfer_hip_waterfall_wav_workers(C.byref(cfg), devs, len(devices), C.byref(disp), int(avg_mode), depth, minbin,
                                                     maxbin, int(max0), os.fsencode(path), frames, rgb.ctypes.data, levp,
                                                     C.byref(nf), WAV_PARTIAL_TAIL if partial_tail else 0),
               "glfer_hip_waterfall_wav_workers")
    return rgb[:nf.value], (lev[:nf.value] if want_lev else None)


class Workers:
    """glfer_hip_workers: a kept set of workers (one plan + chunk ring per entry of `devices`) for the file / host-buffer entries."""

    def __init__(self, params, devices, hint_frames=0):
        cfg = make_config(params, devices[0])
        devs = (C.c_int * len(devices))(*devices)
        self._h = C.c_void_p()
        self._destroy = lib().glfer_hip_workers_destroy
        _check(lib().glfer_hip_workers_create(C.byref(cfg), devs, len(devices), hint_frames, C.byref(self._h)), "glfer_hip_workers_create")
        self.params, self.devices = params, list(devices)
        self.bins = params.n // 2 + 1

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._destroy(self._h)
            self._h.value = None

    __del__ = close

    def run_wav(self, path, out, partial_tail=False, phases=True):
        """rows into `out` (a numpy array [frames][bins], ideally pinned); returns (frames, phases dict or None).  phases=False: no
        timing events are recorded (they cost a few per cent with one worker and more with several sharing a GPU)."""
        nf, ph = C.c_size_t(0), Phases()
        _check(lib().glfer_hip_workers_spectrogram_wav(self._h, os.fsencode(path), out.ctypes.data, out.shape[0], C.byref(nf),
                                                       WAV_PARTIAL_TAIL if partial_tail else 0, C.byref(ph) if phases else None),
               "glfer_hip_workers_spectrogram_wav")
        return nf.value, (ph.as_dict() if phases else None)

    def run_host(self, samples, out, phases=True):
        nf, ph = C.c_size_t(0), Phases()
        _check(lib().glfer_hip_workers_spectrogram_host(self._h, samples.ctypes.data, samples.size, out.ctypes.data, C.byref(nf),
                                                        C.byref(ph) if phases else None), "glfer_hip_workers_spectrogram_host")
        return nf.value, (ph.as_dict() if phases else None)


class PinnedArray:
    """A numpy view of pinned host memory from glfer_hip_host_alloc (rows land in it by DMA)."""

    def __init__(self, shape, dtype):
        self.nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
        self.ptr = lib().glfer_hip_host_alloc(self.nbytes)
        if not self.ptr:
            raise GlferHipError("glfer_hip_host_alloc(%d) failed" % self.nbytes)
        buf = (C.c_ubyte * self.nbytes).from_address(self.ptr)
        self.array = np.frombuffer(buf, dtype=dtype).reshape(shape)

    def free(self):
        if self.ptr:
            self.array = None
            lib().glfer_hip_host_free(self.ptr)
            self.ptr = None


def pinned_empty(shape, dtype):
    """numpy.empty in pinned host memory; freed when the array (and every view of it) is gone."""
    import weakref
    nbytes = max(1, int(np.prod(shape)) * np.dtype(dtype).itemsize)
    ptr = lib().glfer_hip_host_alloc(nbytes)
    if not ptr:
        raise GlferHipError("glfer_hip_host_alloc(%d) failed" % nbytes)
    buf = (C.c_ubyte * nbytes).from_address(ptr)
    weakref.finalize(buf, lib().glfer_hip_host_free, ptr)      # buf is the base of every view
    return np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape))).reshape(shape)


def wav_probe(path):
    """open_wav_file()'s header parse (wav_fmt.c:45-80) with fixed-width fields."""
    info = WavInfo()
    _check(lib().glfer_hip_wav_probe(os.fsencode(path), C.byref(info)), "glfer_hip_wav_probe")
    return info


def compute_floor(psd):
    """compute_floor (fft.c:240-294) for every row of a device PSD tensor.
    Returns a [frames][4] float tensor: sig, floor, peak value, peak bin."""
    torch = _torch()
    assert psd.is_cuda and psd.dtype == torch.float32 and psd.is_contiguous() and psd.dim() == 2
    out = torch.empty((psd.shape[0], 4), dtype=torch.float32, device=psd.device)
    st = C.c_void_p(torch.cuda.current_stream(psd.device).cuda_stream)
    _check(lib().glfer_hip_floor_device(psd.data_ptr(), psd.shape[0], psd.shape[1], out.data_ptr(), st),
           "glfer_hip_floor_device")
    return out


def palette(p_n):
    """set_palette (g_main.c:651-762) as a uint8 [256][3] numpy array (host table)."""
    import numpy as np
    tab = (C.c_ubyte * 768)()
    _check(lib().glfer_hip_palette(int(p_n), tab), "glfer_hip_palette")
    return np.frombuffer(bytes(tab), np.uint8).reshape(256, 3).copy()


def display(disp, src, stats, want_lev=True, want_levels=True):
    """The column mapping of main_window_draw (g_main.c:1099-1236) for every row of `src`
    (float32 PSD, or float64 averaged spectrum from update_avg) with compute_floor's `stats`.
    `disp` (a Display) carries first_buffer / display_*_lvl across calls and is updated.
    Returns (rgb uint8 [frames][bins][3], lev int16 [frames][bins] | None,
    levels float32 [frames][4] | None)."""
    torch = _torch()
    assert src.is_cuda and src.is_contiguous() and src.dim() == 2
    assert src.dtype in (torch.float32, torch.float64)
    assert stats.is_cuda and stats.dtype == torch.float32 and stats.is_contiguous()
    assert stats.shape == (src.shape[0], 4)
    frames, bins = src.shape
    rgb = torch.empty((frames, bins, 3), dtype=torch.uint8, device=src.device)
    lev = torch.empty((frames, bins), dtype=torch.int16, device=src.device) if want_lev else None
    levels = torch.empty((frames, 4), dtype=torch.float32, device=src.device) if want_levels else None
    st = C.c_void_p(torch.cuda.current_stream(src.device).cuda_stream)
    is_d = src.dtype == torch.float64
    _check(lib().glfer_hip_display_device(
        C.byref(disp), None if is_d else C.c_void_p(src.data_ptr()),
        C.c_void_p(src.data_ptr()) if is_d else None, C.c_void_p(stats.data_ptr()), frames, bins,
        C.c_void_p(rgb.data_ptr()), C.c_void_p(lev.data_ptr()) if want_lev else None,
        C.c_void_p(levels.data_ptr()) if want_levels else None, st), "glfer_hip_display_device")
    return rgb, lev, levels


def waterfall(disp, psd, avg_mode=0, depth=1, minbin=0, maxbin=1, max0=0, want_lev=True, want_stats=False):
    """glfer_hip_waterfall_device: floor statistics, optional moving average, level tracking and the
    pixel map of a batch of PSD rows, tile by tile.  Returns (rgb, lev | None, stats | None)."""
    torch = _torch()
    assert psd.is_cuda and psd.dtype == torch.float32 and psd.is_contiguous() and psd.dim() == 2
    frames, bins = psd.shape
    rgb = torch.empty((frames, bins, 3), dtype=torch.uint8, device=psd.device)
    lev = torch.empty((frames, bins), dtype=torch.int16, device=psd.device) if want_lev else None
    stats = torch.empty((frames, 4), dtype=torch.float32, device=psd.device) if want_stats else None
    st = C.c_void_p(torch.cuda.current_stream(psd.device).cuda_stream)
    _check(lib().glfer_hip_waterfall_device(C.byref(disp), int(avg_mode), depth, minbin, maxbin, int(max0), psd.data_ptr(), frames,
                                            bins, rgb.data_ptr(), lev.data_ptr() if want_lev else None,
                                            stats.data_ptr() if want_stats else None, st), "glfer_hip_waterfall_device")
    return rgb, lev, stats


def waterfall_batch(disps, psd, avg_mode=0, depth=1, minbin=0, maxbin=1, max0=0, want_lev=True, want_stats=False):
    """glfer_hip_waterfall_batch_device: waterfall() over B independent streams in one call.  psd [B][frames][bins] float32 on
    the GPU (Spectrogram.run_batch's rows), disps a sequence of B Display objects with the same options, each carrying its
    stream's state in and out (updated in place).  Returns (rgb [B][frames][bins][3], lev [B][frames][bins] | None,
    stats [B][frames][4] | None); stream b's are waterfall(disps[b], psd[b], ...)'s."""
    torch = _torch()
    assert psd.is_cuda and psd.dtype == torch.float32 and psd.is_contiguous() and psd.dim() == 3
    nb, frames, bins = psd.shape
    assert len(disps) == nb
    arr = (Display * nb)(*disps)
    rgb = torch.empty((nb, frames, bins, 3), dtype=torch.uint8, device=psd.device)
    lev = torch.empty((nb, frames, bins), dtype=torch.int16, device=psd.device) if want_lev else None
    stats = torch.empty((nb, frames, 4), dtype=torch.float32, device=psd.device) if want_stats else None
    st = C.c_void_p(torch.cuda.current_stream(psd.device).cuda_stream)
    _check(lib().glfer_hip_waterfall_batch_device(arr, nb, int(avg_mode), depth, minbin, maxbin, int(max0), psd.data_ptr(), frames,
                                                  bins, rgb.data_ptr(), lev.data_ptr() if want_lev else None,
                                                  stats.data_ptr() if want_stats else None, st), "glfer_hip_waterfall_batch_device")
    for d, out in zip(disps, arr):
        C.memmove(C.addressof(d), C.addressof(out), C.sizeof(Display))
    return rgb, lev, stats


def _row_starts(row_starts, rows):
    """row_starts as the C entries take it: uint64 [nstreams + 1], non-decreasing, ending at most at `rows`."""
    starts = np.asarray(row_starts)
    if starts.ndim != 1 or starts.size < 1 or starts.dtype.kind not in "iu":
        raise ValueError("row_starts: a 1-D integer array of nstreams + 1 entries")
    if starts.size and (int(starts.min()) < 0 or np.any(np.diff(starts.astype(np.int64)) < 0)):
        raise ValueError("row_starts: non-negative and non-decreasing")
    if int(starts[-1]) > rows:
        raise ValueError("row_starts: the last entry reaches past the rows given")
    return np.ascontiguousarray(starts, dtype=np.uint64)


def waterfall_ragged(disps, psd, row_starts, avg_mode=0, depth=1, minbin=0, maxbin=1, max0=0, want_lev=True, want_stats=False):
    """glfer_hip_waterfall_ragged_device: waterfall() over streams of unequal length in one call.  psd [rows][bins] float32 on
    the GPU, packed as Spectrogram.run_ragged returns it; stream b is rows [row_starts[b], row_starts[b + 1]).  Rows at a
    pitch (displays that carry psd_pitch): give the view rows[:, :bins] of the [rows][pitch] tensor.  disps: one Display per
    stream, the same options, each carrying its stream's state in and out (updated in place; a stream without rows keeps its
    own).  Returns (rgb [rows][bins][3], lev [rows][bins] | None, stats [rows][4] | None, row_starts)."""
    torch = _torch()
    if psd.dim() != 2 or psd.dtype != torch.float32:
        raise ValueError("psd: a 2-D float32 tensor")
    starts = _row_starts(row_starts, psd.size(0))
    nb = starts.size - 1
    if len(disps) != nb:
        raise ValueError("one Display per stream: len(disps) == len(row_starts) - 1")
    if not psd.is_cuda:
        raise ValueError("psd: on the GPU")
    bins = psd.size(1)
    pitch = (int(disps[0].psd_pitch) if nb else 0) or bins
    if psd.size(0) > 1 and not (psd.stride(1) == 1 and psd.stride(0) == pitch):
        raise ValueError("psd: rows of `bins` floats, psd_pitch (or bins) floats apart")
    rows = int(starts[-1])
    arr = (Display * max(nb, 1))(*disps)
    rgb = torch.empty((rows, bins, 3), dtype=torch.uint8, device=psd.device)
    lev = torch.empty((rows, bins), dtype=torch.int16, device=psd.device) if want_lev else None
    stats = torch.empty((rows, 4), dtype=torch.float32, device=psd.device) if want_stats else None
    st = C.c_void_p(torch.cuda.current_stream(psd.device).cuda_stream)
    _check(lib().glfer_hip_waterfall_ragged_device(arr, nb, int(avg_mode), depth, minbin, maxbin, int(max0), psd.data_ptr(),
                                                   starts.ctypes.data, bins, rgb.data_ptr(), lev.data_ptr() if want_lev else None,
                                                   stats.data_ptr() if want_stats else None, st), "glfer_hip_waterfall_ragged_device")
    for d, out in zip(disps, arr):
        C.memmove(C.addressof(d), C.addressof(out), C.sizeof(Display))
    return rgb, lev, stats, starts.astype(np.int64)


def update_avg_ragged(mode, psd, row_starts, depth, minbin, maxbin, max0=0, n_out=None):
    """update_avg over packed rows of streams of unequal length (glfer_hip_avg_ragged_device): psd [rows][bins] float32 on the
    GPU as Spectrogram.run_ragged returns it (dense rows), stream b its rows [row_starts[b], row_starts[b + 1]), the averaging
    state empty at row 0 of each stream.  Returns (avg [rows][n_out] float64, ret [rows][4] float64, row_starts); stream b's
    rows are update_avg(mode, psd[row_starts[b]:row_starts[b + 1]], ...)'s."""
    torch = _torch()
    if psd.dim() != 2 or psd.dtype != torch.float32:
        raise ValueError("psd: a 2-D float32 tensor")
    starts = _row_starts(row_starts, psd.size(0))
    if not (psd.is_cuda and psd.is_contiguous()):
        raise ValueError("psd: contiguous, on the GPU")
    bins = psd.size(1)
    n_out = bins if n_out is None else n_out
    rows = int(starts[-1])
    avg = torch.empty((rows, n_out), dtype=torch.float64, device=psd.device)
    ret = torch.empty((rows, 4), dtype=torch.float64, device=psd.device)
    st = C.c_void_p(torch.cuda.current_stream(psd.device).cuda_stream)
    _check(lib().glfer_hip_avg_ragged_device(int(mode), psd.data_ptr(), starts.size - 1, starts.ctypes.data, bins, n_out, depth, minbin,
                                             maxbin, int(max0), avg.data_ptr(), ret.data_ptr(), st),
           "glfer_hip_avg_ragged_device")
    return avg, ret, starts.astype(np.int64)


def avg_cum(psd, depth, minbin, maxbin, n_out=None):
    """avgdata->cum after each frame (avg.c:114-127): float64 [frames][n_out], zeros out of band."""
    torch = _torch()
    assert psd.is_cuda and psd.dtype == torch.float32 and psd.is_contiguous() and psd.dim() == 2
    frames, bins = psd.shape
    n_out = bins if n_out is None else n_out
    cum = torch.zeros((frames, n_out), dtype=torch.float64, device=psd.device)
    st = C.c_void_p(torch.cuda.current_stream(psd.device).cuda_stream)
    _check(lib().glfer_hip_avg_cum_device(psd.data_ptr(), frames, bins, n_out, depth, minbin, maxbin, cum.data_ptr(), st),
           "glfer_hip_avg_cum_device")
    return cum


def update_avg(mode, psd, depth, minbin, maxbin, max0=0, n_out=None):
    """update_avg_{sumavg,plain,sumextreme} (avg.c:108-298) applied to consecutive rows of a
    device PSD tensor, starting from an empty averaging state (alloc_avg, avg.c:38-60).
    Returns (avg [frames][n_out] float64, ret [frames][4] float64 = value, peakbin, variance,
    effdepth)."""
    torch = _torch()
    assert psd.is_cuda and psd.dtype == torch.float32 and psd.is_contiguous() and psd.dim() == 2
    frames, bins = psd.shape
    n_out = bins if n_out is None else n_out
    avg = torch.empty((frames, n_out), dtype=torch.float64, device=psd.device)
    ret = torch.empty((frames, 4), dtype=torch.float64, device=psd.device)
    st = C.c_void_p(torch.cuda.current_stream(psd.device).cuda_stream)
    _check(lib().glfer_hip_avg_device(int(mode), psd.data_ptr(), frames, bins, n_out, depth, minbin,
                                      maxbin, int(max0), avg.data_ptr(), ret.data_ptr(), st),
           "glfer_hip_avg_device")
    return avg, ret


def _lmp_rows(rows, dim, avg, first_frame, lead):
    """the checks lmp_statistic and lmp_statistic_batch share: returns (frames held, frames out, bins)"""
    torch = _torch()
    if rows.dim() != dim or rows.dtype != torch.float32:
        raise ValueError("rows: a %d-D float32 tensor" % dim)
    if not 1 <= int(avg) <= 4096:
        raise ValueError("avg: 1 .. 4096")
    first_frame, lead = int(first_frame), int(lead)
    if first_frame < 0 or lead < 0 or lead > first_frame:
        raise ValueError("first_frame >= lead >= 0")
    if lead < min(int(avg) - 1, first_frame):
        raise ValueError("lead: the rows must reach back min(avg - 1, first_frame) frames")
    held, bins = rows.size(dim - 2), rows.size(dim - 1)
    if held < lead or bins < 1:
        raise ValueError("rows: at least `lead` rows of at least one bin")
    if not rows.is_cuda:
        raise ValueError("rows: on the GPU")
    return held, held - lead, bins


def lmp_statistic(rows, avg, first_frame=0, lead=0):
    """The LMP detection statistic (lmp.c:132-160, glfer_hip_lmp_device) over rectangular-window periodogram rows already on the
    GPU: rows [lead + frames][bins] float32 are frames first_frame - lead .. of one stream (FftParams(window_type=rectangular)
    rows, from run / run_batch / run_ragged), lead >= min(avg - 1, first_frame): the frames the ring still holds at first_frame.
    Returns [frames][bins] float32: bit for bit Spectrogram(LmpParams(avg=avg, ...)).run(x, first_frame, frames)."""
    torch = _torch()
    held, frames, bins = _lmp_rows(rows, 2, avg, first_frame, lead)
    if not rows.is_contiguous():
        raise ValueError("rows: contiguous")
    out = torch.empty((frames, bins), dtype=torch.float32, device=rows.device)
    st = C.c_void_p(torch.cuda.current_stream(rows.device).cuda_stream)
    _check(lib().glfer_hip_lmp_device(rows.data_ptr(), int(first_frame) - int(lead), int(first_frame), frames, bins, int(avg),
                                      out.data_ptr(), st), "glfer_hip_lmp_device")
    return out


def lmp_statistic_batch(rows, avg, first_frame=0, lead=0):
    """lmp_statistic over B independent streams in one launch set (glfer_hip_lmp_batch_device): rows [B][lead + frames][bins]
    float32 on the GPU, the same first_frame and lead for every stream, each stream's ring empty before its frame 0.  The
    streams may be any number of floats apart (rows.stride(0): a slice along the frames of a larger tensor is taken as it is).
    Returns [B][frames][bins] float32; stream b's rows are lmp_statistic(rows[b], ...)'s."""
    torch = _torch()
    held, frames, bins = _lmp_rows(rows, 3, avg, first_frame, lead)
    nb = rows.size(0)
    if nb > 1 and held > 0 and not (rows.stride(2) == 1 and (held == 1 or rows.stride(1) == bins) and rows.stride(0) >= held * bins):
        raise ValueError("rows: each stream's rows dense, the streams at least a stream's rows apart")
    if nb <= 1 or held == 0:
        rows = rows.contiguous()
    out = torch.empty((nb, frames, bins), dtype=torch.float32, device=rows.device)
    st = C.c_void_p(torch.cuda.current_stream(rows.device).cuda_stream)
    _check(lib().glfer_hip_lmp_batch_device(rows.data_ptr(), nb, rows.stride(0) if nb > 1 else held * bins, int(first_frame) - int(lead),
                                            int(first_frame), frames, bins, int(avg), out.data_ptr(), frames * bins, st),
           "glfer_hip_lmp_batch_device")
    return out


def lmp_statistic_ragged(rows, row_starts, avg, out=None):
    """lmp_statistic over packed rows of streams of unequal length (glfer_hip_lmp_ragged_device): rows [rows][bins] float32 on
    the GPU as Spectrogram.run_ragged returns them for a rectangular-window FFT plan, stream b its rows
    [row_starts[b], row_starts[b + 1]), whole from its frame 0.  Returns ([rows][bins] float32 packed the same way,
    row_starts); rows outside every stream are left unwritten (out: a tensor like rows to write into)."""
    torch = _torch()
    if rows.dim() != 2 or rows.dtype != torch.float32:
        raise ValueError("rows: a 2-D float32 tensor")
    if not 1 <= int(avg) <= 4096:
        raise ValueError("avg: 1 .. 4096")
    starts = _row_starts(row_starts, rows.size(0))
    if not (rows.is_cuda and rows.is_contiguous()) or rows.size(1) < 1:
        raise ValueError("rows: contiguous, on the GPU")
    if out is None:
        out = torch.empty_like(rows)
    elif not (out.is_cuda and out.is_contiguous() and out.dtype == torch.float32 and out.shape == rows.shape and out.device == rows.device):
        raise ValueError("out: a contiguous float32 tensor of the shape of rows, on their device")
    st = C.c_void_p(torch.cuda.current_stream(rows.device).cuda_stream)
    _check(lib().glfer_hip_lmp_ragged_device(rows.data_ptr(), starts.size - 1, starts.ctypes.data, rows.size(1), int(avg), out.data_ptr(), st),
           "glfer_hip_lmp_ragged_device")
    return out, starts.astype(np.int64)


def _drift_args(frames, step, dmin, dmax):
    """the checks the drift wrappers share: returns (frames, step, dmin, dmax) with the defaults filled in"""
    frames = int(frames)
    if not 2 <= frames <= 4096:
        raise ValueError("frames: 2 .. 4096")
    step = frames if step is None else int(step)
    if step < 1:
        raise ValueError("step: at least 1")
    reach = min(frames - 1, 127)
    dmin = -reach if dmin is None else int(dmin)
    dmax = reach if dmax is None else int(dmax)
    if not (-(frames - 1) <= dmin <= 0 <= dmax <= frames - 1):
        raise ValueError("dmin, dmax: -(frames - 1) <= dmin <= 0 <= dmax <= frames - 1")
    if dmax - dmin + 1 > 255:
        raise ValueError("dmin, dmax: at most 255 drifts")
    return frames, step, dmin, dmax


def _drift_outs(want, out, lead, nblocks, ndrifts, bins, device):
    """The outputs of a drift call by name: made here, or the caller's (out: a mapping or a Drift tuple of dense tensors):
    sums float32 [lead..., nblocks, ndrifts, bins], best float32 and drift int16 [lead..., nblocks, bins]."""
    torch = _torch()
    want = tuple(want)
    if not want or any(w not in DRIFT_FIELDS for w in want):
        raise ValueError("want: a non-empty subset of %s" % (DRIFT_FIELDS,))
    if out is not None and not isinstance(out, dict):
        out = out._asdict()
    ts = {}
    for name in want:
        shape = tuple(lead) + ((nblocks, ndrifts, bins) if name == "sums" else (nblocks, bins))
        dtype = torch.int16 if name == "drift" else torch.float32
        o = None if out is None else out.get(name)
        if o is None:
            o = torch.empty(shape, dtype=dtype, device=device)
        elif not (o.is_cuda and o.dtype == dtype and tuple(o.shape) == shape and o.is_contiguous()):
            raise ValueError("out[%r]: a dense %s tensor of shape %s on the GPU" % (name, dtype, shape))
        ts[name] = o
    return ts


def _drift_ptr(ts, name):
    return C.c_void_p(ts[name].data_ptr()) if name in ts and ts[name].numel() else None


def _drift_rows(rows, dim):
    """the checks drift_sums and drift_sums_batch share on the rows: returns (rows held, bins, pitch)"""
    torch = _torch()
    if rows.dim() != dim or rows.dtype != torch.float32:
        raise ValueError("rows: a %d-D float32 tensor" % dim)
    held, bins = rows.size(dim - 2), rows.size(dim - 1)
    if bins < 1:
        raise ValueError("rows: at least one bin")
    if bins > 1 and rows.stride(dim - 1) != 1:
        raise ValueError("rows: a row's bins adjacent (stride(-1) == 1)")
    pitch = rows.stride(dim - 2) if held > 1 else bins
    if pitch < bins:
        raise ValueError("rows: the rows at least `bins` floats apart")
    if not rows.is_cuda:
        raise ValueError("rows: on the GPU")
    return held, bins, pitch


def drift_blocks(nrows, frames, step=None):
    """blocks of `frames` rows, `step` (default: frames) rows apart, in a run of nrows rows: (nrows - frames) // step + 1, none in
    a shorter run (glfer_hip_drift_blocks)"""
    frames = int(frames)
    step = frames if step is None else int(step)
    if nrows < 0 or not 2 <= frames <= 4096 or step < 1:
        raise ValueError("nrows >= 0, frames 2 .. 4096, step >= 1")
    return int(lib().glfer_hip_drift_blocks(int(nrows), frames, step))


def drift_offsets(frames, dmin, dmax):
    """o(d, t) = d t / (frames - 1) rounded half away from zero, as the kernel takes it: numpy int32 [dmax - dmin + 1][frames]
    (glfer_hip_drift_offsets)"""
    frames, _, dmin, dmax = _drift_args(frames, None, dmin, dmax)
    offs = np.empty((dmax - dmin + 1, frames), np.int32)
    _check(lib().glfer_hip_drift_offsets(frames, dmin, dmax, offs.ctypes.data), "glfer_hip_drift_offsets")
    return offs


def drift_sums(rows, frames, step=None, dmin=None, dmax=None, want=("best", "drift"), out=None):
    """The drift search over rows already on the GPU (glfer_hip_drift_device): rows [F][bins] float32 with stride(1) == 1 and
    stride(0) >= bins (rows of run / run_batch / update_avg's inputs, a slice of wider rows included).  Block b is rows
    b step .. b step + frames - 1 (step defaults to frames); along every straight line of drift d = dmin .. dmax bins across the
    block (defaults -+min(frames - 1, 127)) the rows are summed in float32 in frame order, a bin outside the row adding nothing.
    Returns Drift(sums [blocks][drifts][bins], best [blocks][bins], drift [blocks][bins] int16) with None for what `want` does
    not name: best is the largest sum at a bin and drift the d that gave it (ties: the smallest |d|, +d before -d).  One launch
    on torch's current stream, no allocation inside the library: legal under graph capture with `out` given."""
    torch = _torch()
    held, bins, pitch = _drift_rows(rows, 2)
    frames, step, dmin, dmax = _drift_args(frames, step, dmin, dmax)
    nblocks = drift_blocks(held, frames, step)
    ts = _drift_outs(want, out, (), nblocks, dmax - dmin + 1, bins, rows.device)
    st = C.c_void_p(torch.cuda.current_stream(rows.device).cuda_stream)
    _check(lib().glfer_hip_drift_device(C.c_void_p(rows.data_ptr()), held, bins, pitch, frames, step, nblocks, dmin, dmax,
                                        *(_drift_ptr(ts, k) for k in DRIFT_FIELDS), st), "glfer_hip_drift_device")
    return Drift(*(ts.get(k) for k in DRIFT_FIELDS))


def drift_sums_batch(rows, frames, step=None, dmin=None, dmax=None, want=("best", "drift"), out=None):
    """drift_sums over B independent streams in one launch (glfer_hip_drift_batch_device): rows [B][F][bins] float32 on the GPU,
    stride(2) == 1, stride(1) >= bins, the streams at least a stream's rows apart (stride(0)).  Returns Drift of
    [B][blocks][...] tensors; entry b is bit for bit drift_sums(rows[b], ...)."""
    torch = _torch()
    held, bins, pitch = _drift_rows(rows, 3)
    frames, step, dmin, dmax = _drift_args(frames, step, dmin, dmax)
    nb = rows.size(0)
    need = (held - 1) * pitch + bins if held else 0
    stride = rows.stride(0) if nb > 1 else need
    if stride < need:
        raise ValueError("rows: the streams at least a stream's rows apart")
    nblocks = drift_blocks(held, frames, step)
    D = dmax - dmin + 1
    ts = _drift_outs(want, out, (nb,), nblocks, D, bins, rows.device)
    st = C.c_void_p(torch.cuda.current_stream(rows.device).cuda_stream)
    _check(lib().glfer_hip_drift_batch_device(C.c_void_p(rows.data_ptr()), nb, stride, held, bins, pitch, frames, step, nblocks, dmin, dmax,
                                              _drift_ptr(ts, "sums"), nblocks * D * bins, _drift_ptr(ts, "best"), nblocks * bins,
                                              _drift_ptr(ts, "drift"), nblocks * bins, st), "glfer_hip_drift_batch_device")
    return Drift(*(ts.get(k) for k in DRIFT_FIELDS))


def update_avg_batch(mode, psd, depth, minbin, maxbin, max0=0, n_out=None):
    """update_avg over the rows of B independent streams (glfer_hip_avg_batch_device): psd [B][frames][bins] float32 on the
    GPU, the averaging state empty at row 0 of each stream.  Returns (avg [B][frames][n_out] float64, ret [B][frames][4]
    float64); stream b's are update_avg(mode, psd[b], ...)'s."""
    torch = _torch()
    assert psd.is_cuda and psd.dtype == torch.float32 and psd.is_contiguous() and psd.dim() == 3
    nb, frames, bins = psd.shape
    n_out = bins if n_out is None else n_out
    avg = torch.empty((nb, frames, n_out), dtype=torch.float64, device=psd.device)
    ret = torch.empty((nb, frames, 4), dtype=torch.float64, device=psd.device)
    st = C.c_void_p(torch.cuda.current_stream(psd.device).cuda_stream)
    _check(lib().glfer_hip_avg_batch_device(int(mode), psd.data_ptr(), nb, frames, bins, n_out, depth, minbin, maxbin, int(max0),
                                            avg.data_ptr(), ret.data_ptr(), st),
           "glfer_hip_avg_batch_device")
    return avg, ret
