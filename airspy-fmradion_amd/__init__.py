"""airspy-fmradion_amd -- MI355X-native FM/AM demodulation hot path.

Python-side binding of the C-ABI (include/fmradion_amd.h) used by the tests
and by bench.py.  The product is libfmradion_amd.so (hand-written HIP kernels,
csrc/); this module only loads it with ctypes.  There is no CPU fallback: if
the library is missing or no GPU is present, creation fails loudly.

The directory name carries a hyphen (the contract's package name), so import it
with importlib:  fmr = importlib.import_module("airspy-fmradion_amd").
"""
import collections
import ctypes as C
import math
import os
import subprocess

import numpy as np

_DIR = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_DIR, "libfmradion_amd.so")
# The same sources with -DFMR_AB_PARTNERS: the product plus the slower forms two GPU tests compare it with (the PLL's
# seven-launch Newton round, FMR_PLL_V1) and a test hook (FMR_TEST_AGC_LATE).  Loaded only by chains that are created while
# Chain(..., ab=True) -- the two tests that need them say so; the switches themselves are read from the environment by that
# library only.  The product library does not carry them, and a leftover variable in the environment selects nothing.
LIB_PATH_AB = os.path.join(_DIR, "libfmradion_amd_ab.so")
SRC = os.path.join(_DIR, "csrc", "fmradion_amd.hip")
HIPCC_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared"]

MODE_NONE, MODE_FM, MODE_NBFM, MODE_AM, MODE_DSB, MODE_USB, MODE_LSB, MODE_CW, MODE_WSPR = -1, 0, 1, 2, 3, 4, 5, 6, 7
IQ_CF32, IQ_S16, IQ_U8, IQ_S8 = 0, 1, 2, 3
RESAMPLER_FAST, RESAMPLER_R8B = 0, 1
_IQ_DTYPE = {0: np.complex64, 1: np.int16, 2: np.uint8, 3: np.int8}
OK, ERR_NO_DEVICE, ERR_BAD_ARG, ERR_UNSUPPORTED, ERR_CAPACITY, ERR_HIP = 0, -1, -2, -3, -4, -5
# FMR_FE_* (include/fmradion_amd.h): the kernel forms of the IF resampler, by bit
FE_FORMS = {"fused": 1 << 0, "decim16": 1 << 1, "decim2_16": 1 << 2, "decim2_24": 1 << 3, "decim": 1 << 4,
            "poly5h": 1 << 5, "poly5h_disc": 1 << 6, "poly4": 1 << 7, "poly4_am": 1 << 8, "poly3": 1 << 9,
            "poly2": 1 << 10, "poly_frac": 1 << 11, "poly": 1 << 12}
# FMR_CB_* (include/fmradion_amd.h): the kernel forms of a channel bank's stage A (fmr_resampler_info which = 8)
CB_FORMS = {"modtap": 1 << 0}

EXPORTS = [
    "fmr_create", "fmr_destroy", "fmr_last_error", "fmr_version", "fmr_resampler_info", "fmr_process",
    "fmr_process_blocks", "fmr_process_blocks_device", "fmr_synchronize", "fmr_resample", "fmr_get_status",
    "fmr_get_pps_events", "fmr_get_multipath_coefficients", "fmr_debug_read", "fmr_debug_live_resources", "fmr_debug_chain_shape",
    "fmr_get_kernel_times",
    "fmr_probe_read_bandwidth", "fmr_probe_shader_clock", "fmr_get_kernel_trace",
    "fmr_enable_kernel_timing", "fmr_filter_table", "fmr_fourth_convert", "fmr_design_taps", "fmr_design_taps_class",
    "fmr_host_alloc", "fmr_host_free", "fmr_create_sized", "fmr_get_status_sized",
    "fmr_create_channelizer", "fmr_resample_blocks", "fmr_resample_blocks_device", "fmr_create_rds",
    "fmr_get_rds_groups", "fmr_get_rds_status", "fmr_set_rds_correction",
    "fmr_spectrum_create", "fmr_spectrum_destroy", "fmr_spectrum_process", "fmr_spectrum_process_device",
    "fmr_spectrum_synchronize", "fmr_spectrum_read", "fmr_spectrum_reset", "fmr_find_stations",
    "fmr_spectrum_create_waterfall", "fmr_spectrum_read_waterfall",
    "fmr_enable_monitor", "fmr_monitor_read", "fmr_monitor_derive",
    "fmr_enable_loudness", "fmr_loudness_read", "fmr_loudness_derive",
    "fmr_enable_analyser", "fmr_analyser_read", "fmr_analyser_derive",
    "fmr_enable_rf_monitor", "fmr_rf_monitor_read", "fmr_rf_monitor_derive",
    "fmr_enable_output", "fmr_output_read", "fmr_squelch_level_from_db",
    "fmr_set_output_rate", "fmr_get_output_rate", "fmr_output_rate_taps",
    "fmr_enable_mpx_output", "fmr_mpx_output_read", "fmr_mpx_output_taps",
    "fmr_create_mpx_decoder", "fmr_process_mpx_blocks", "fmr_process_mpx_blocks_device", "fmr_get_mpx_input_info",
    "fmr_mpx_input_geometry", "fmr_debug_mpx_chain_shape",
    "fmr_enable_weak_signal", "fmr_weak_signal_read", "fmr_weak_signal_derive",
    "fmr_enable_blanker", "fmr_blanker_read", "fmr_blanker_derive",
    "fmr_enable_iq_correction", "fmr_iq_correction_read", "fmr_iq_correction_derive",
]
# FMR_WINDOW_* (include/fmradion_amd.h): windows of the band spectrum
WINDOW_HANN, WINDOW_RECT, WINDOW_BLACKMAN_HARRIS = 0, 1, 2
# FMR_WATERFALL_* (include/fmradion_amd.h): what a waterfall line holds
WATERFALL_MEAN, WATERFALL_PEAK = 0, 1
# FMR_RDS_* (include/fmradion_amd.h): per-block status of an RDS group
RDS_OK, RDS_CORRECTED, RDS_BAD, RDS_CPRIME = 0, 1, 2, 4
# FMR_RDS_FEC_* (include/fmradion_amd.h): error correction of synchronised blocks (Chain.set_rds_correction)
RDS_FEC_OFF, RDS_FEC_BURST, RDS_FEC_SOFT = 0, 1, 2
# fmr_rds_group as a numpy structured type (24 bytes)
RDS_GROUP = np.dtype([("sample_index", np.uint64), ("block", np.uint16, 4), ("status", np.uint8, 4), ("reserved", np.uint32)])
# fmr_monitor_record as a numpy structured type (56 bytes)
MONITOR_RECORD = np.dtype([("index", np.uint64), ("first_sample", np.uint64), ("n_finite", np.uint32),
                           ("n_nonfinite", np.uint32), ("segments", np.uint32), ("segments_skipped", np.uint32),
                           ("min", np.float32), ("max", np.float32), ("sum", np.float64), ("sumsq", np.float64)])
MONITOR_PSD_BINS = 513
# fmr_loudness_record as a numpy structured type (104 bytes)
LOUDNESS_RECORD = np.dtype([("index", np.uint64), ("first_sample", np.uint64), ("n_nonfinite", np.uint32),
                            ("channels", np.uint32), ("step_samples", np.uint32), ("reserved", np.uint32),
                            ("kw_sumsq", np.float64, 2), ("sumsq", np.float64, 2), ("sum_lr", np.float64),
                            ("sample_peak", np.float64, 2), ("true_peak", np.float64, 2)])
# fmr_analyser_record as a numpy structured type (72 bytes)
ANALYSER_RECORD = np.dtype([("index", np.uint64), ("first_sample", np.uint64), ("segments", np.uint32),
                            ("skipped", np.uint32), ("n_nonfinite", np.uint32), ("channels", np.uint32),
                            ("fft_size", np.uint32), ("interval_samples", np.uint32), ("sum", np.float64, 2),
                            ("sumsq", np.float64, 2)])
ANALYSER_VIEWS = {"L": 0, "R": 1, "M": 2, "S": 3}
# fmr_rf_monitor_record as a numpy structured type (56 bytes)
RF_MONITOR_RECORD = np.dtype([("index", np.uint64), ("first_sample", np.uint64), ("n_finite", np.uint32),
                              ("n_nonfinite", np.uint32), ("segments", np.uint32), ("segments_skipped", np.uint32),
                              ("p_min", np.float32), ("p_max", np.float32), ("m2", np.float64), ("m4", np.float64)])
RF_HIST_BINS, RF_PSD_BINS = 384, 513
# FMR_PCM_* (include/fmradion_amd.h): sample format of the output stage
PCM_S16, PCM_F32 = 0, 1
_PCM_DTYPE = {PCM_S16: np.int16, PCM_F32: np.float32}
# fmr_output_block as a numpy structured type (56 bytes)
OUTPUT_BLOCK = np.dtype([("block", np.uint64), ("first_frame", np.uint64), ("n_frames", np.uint32), ("channels", np.uint32),
                         ("if_rms", np.float32), ("if_level", np.float32), ("audio_mean", np.float32),
                         ("audio_rms", np.float32), ("audio_level", np.float32), ("gate_open", np.uint32),
                         ("n_clipped", np.uint32), ("n_nonfinite", np.uint32)])
# FMR_WS_* (include/fmradion_amd.h): mode and actions of the weak-signal stage
WS_MEASURE, WS_ACT = 0, 1
WS_BLEND, WS_HIGHCUT, WS_MUTE = 1, 2, 4
# fmr_weak_signal_record as a numpy structured type (96 bytes)
WEAK_SIGNAL_RECORD = np.dtype([("index", np.uint64), ("first_interval", np.uint64), ("n_intervals", np.uint32),
                               ("n_nonfinite", np.uint32), ("usn_sum", np.float64), ("usn_peak", np.float64),
                               ("smoothed", np.float64), ("t_blend", np.float64), ("t_highcut", np.float64),
                               ("t_mute", np.float64), ("max_blend", np.float64), ("max_highcut", np.float64),
                               ("max_mute", np.float64)])
# FMR_NB_* (include/fmradion_amd.h): mode of the impulse blanker; NB_Q: samples per interval
NB_MEASURE, NB_ACT = 0, 1
NB_Q = 4096
# fmr_blanker_record as a numpy structured type (72 bytes)
BLANKER_RECORD = np.dtype([("index", np.uint64), ("first_interval", np.uint64), ("n_triggers", np.uint64),
                           ("n_blanked", np.uint64), ("n_nonfinite", np.uint64), ("n_runs", np.uint64),
                           ("power_q", np.uint64), ("threshold", np.float64), ("n_intervals", np.uint32),
                           ("peak", np.float32)])
# FMR_IQC_* (include/fmradion_amd.h): mode of the IQ corrector, and the mask of what it applies
IQC_MEASURE, IQC_ACT = 0, 1
IQC_DC, IQC_BALANCE = 1, 2
# fmr_iq_correction_record as a numpy structured type (112 bytes)
IQ_CORRECTION_RECORD = np.dtype([("index", np.uint64), ("first_interval", np.uint64), ("n_usable", np.uint64),
                                 ("n_nonfinite", np.uint64), ("n_skipped", np.uint64), ("n_refused", np.uint64),
                                 ("sum_re", np.int64), ("sum_im", np.int64), ("sum_rr", np.int64), ("sum_ii", np.int64),
                                 ("sum_ri", np.int64), ("n_intervals", np.uint32), ("dc_re", np.float32),
                                 ("dc_im", np.float32), ("w_re", np.float32), ("w_im", np.float32),
                                 ("reserved", np.uint32)])


class FmrError(RuntimeError):
    pass


def output_rate_taps(rate):
    """fmr_output_rate_taps: (h float64 [T L], L, M, T) -- the prototype filter of the output stage at `rate` (host only)."""
    Lb = lib()
    l, m, t = C.c_int(), C.c_int(), C.c_int()
    n = Lb.fmr_output_rate_taps(int(rate), None, 0, C.byref(l), C.byref(m), C.byref(t))
    if n < 0:
        raise FmrError(f"fmradion_amd error {n}: {Lb.fmr_last_error().decode()}")
    h = np.zeros(n, dtype=np.float64)
    Lb.fmr_output_rate_taps(int(rate), h.ctypes.data_as(C.POINTER(C.c_double)), n, None, None, None)
    return h, l.value, m.value, t.value


def mpx_output_taps(rate):
    """fmr_mpx_output_taps: (h float64 [T L], L, M, T) -- the prototype filter of the MPX output at `rate` (host only)."""
    Lb = lib()
    l, m, t = C.c_int(), C.c_int(), C.c_int()
    n = Lb.fmr_mpx_output_taps(int(rate), None, 0, C.byref(l), C.byref(m), C.byref(t))
    if n < 0:
        raise FmrError(f"fmradion_amd error {n}: {Lb.fmr_last_error().decode()}")
    h = np.zeros(n, dtype=np.float64)
    Lb.fmr_mpx_output_taps(int(rate), h.ctypes.data_as(C.POINTER(C.c_double)), n, None, None, None)
    return h, l.value, m.value, t.value


def mpx_input_geometry(rate):
    """fmr_mpx_input_geometry: (L, M, T, K, delay_samples) of an MPX input at `rate` (host only)."""
    Lb = lib()
    l, m, t, k, d = C.c_int(), C.c_int(), C.c_int(), C.c_int(), C.c_double()
    rc = Lb.fmr_mpx_input_geometry(int(rate), C.byref(l), C.byref(m), C.byref(t), C.byref(k), C.byref(d))
    if rc < 0:
        raise FmrError(f"fmradion_amd error {rc}: {Lb.fmr_last_error().decode()}")
    return l.value, m.value, t.value, k.value, d.value


def output_frame_of(first_frame, rate):
    """The first ring frame made from a block whose first_frame is `first_frame`: ceil(first_frame L / M)."""
    g = math.gcd(int(rate) if rate else 48000, 48000)
    l, m = (int(rate) if rate else 48000) // g, 48000 // g
    return -(-int(first_frame) * l // m)


class Config(C.Structure):
    _fields_ = [
        ("device", C.c_int), ("n_streams", C.c_int), ("mode", C.c_int), ("input_rate", C.c_double),
        ("enable_resampler", C.c_int), ("enable_fourth_down", C.c_int), ("fmfilter_enable", C.c_int),
        ("filter_coeff", C.POINTER(C.c_float)), ("n_filter_coeff", C.c_int), ("stereo", C.c_int),
        ("deemphasis_us", C.c_double), ("pilot_shift", C.c_int), ("multipath_stages", C.c_uint),
        ("max_block_len", C.c_size_t), ("max_blocks", C.c_int), ("nbfm_freq_dev", C.c_double),
        ("input_format", C.c_int), ("output_rate", C.c_double), ("resampler_class", C.c_int), ("struct_size", C.c_uint),
        ("in_order", C.c_int), ("channel_offset_hz", C.POINTER(C.c_int32)),
    ]


class Status(C.Structure):
    _fields_ = [
        ("if_rms", C.c_float), ("baseband_mean", C.c_float), ("baseband_level", C.c_float),
        ("pilot_level", C.c_double), ("stereo_detected", C.c_int), ("if_agc_gain", C.c_float),
        ("af_agc_gain", C.c_double), ("multipath_error", C.c_double), ("pll_freq_err", C.c_double),
        ("multipath_resets", C.c_uint32),
        ("agc_iterations", C.c_int), ("pll_iterations", C.c_int), ("agc_fallback", C.c_int),
        ("pll_fallback", C.c_int), ("pll_residual", C.c_double),
        ("agc_residual_history", C.c_float * 16), ("pll_residual_history", C.c_double * 16),
        ("pll_residual_components", C.c_double * 8),
        ("pll_mismatch_history", C.c_double * 16), ("pll_mismatch_accepted", C.c_int), ("af_agc_fallback", C.c_int),
        ("agc_sync_timeouts", C.c_uint32),
    ]


class PpsEvent(C.Structure):
    _fields_ = [("pps_index", C.c_uint64), ("sample_index", C.c_uint64), ("block_position", C.c_double),
                ("block", C.c_uint32), ("stream", C.c_uint32)]


class SpectrumConfig(C.Structure):
    _fields_ = [("struct_size", C.c_uint), ("device", C.c_int), ("n_rows", C.c_int), ("input_rate", C.c_double),
                ("input_format", C.c_int), ("fft_size", C.c_int), ("hop", C.c_int), ("window", C.c_int),
                ("max_call_len", C.c_size_t)]


class SpectrumInfo(C.Structure):
    _fields_ = [("segments", C.c_uint64), ("segments_skipped", C.c_uint64), ("first_segment", C.c_uint64),
                ("samples_seen", C.c_uint64), ("bin_hz", C.c_double), ("enbw_hz", C.c_double)]


class WaterfallConfig(C.Structure):
    _fields_ = [("struct_size", C.c_uint), ("segments_per_line", C.c_int), ("max_lines", C.c_int), ("which", C.c_int)]


class WaterfallInfo(C.Structure):
    _fields_ = [("first_line", C.c_uint64), ("lines_ready", C.c_uint64), ("lines_dropped", C.c_uint64),
                ("line_seconds", C.c_double)]


class StationRule(C.Structure):
    _fields_ = [("raster_hz", C.c_int32), ("raster_offset_hz", C.c_int32), ("bandwidth_hz", C.c_int32),
                ("max_abs_offset_hz", C.c_int32), ("threshold_db", C.c_double), ("floor_percentile", C.c_double)]


class Station(C.Structure):
    _fields_ = [("offset_hz", C.c_int32), ("reserved", C.c_int32), ("level_db", C.c_double), ("snr_db", C.c_double),
                ("centroid_hz", C.c_double)]


class MonitorConfig(C.Structure):
    _fields_ = [("struct_size", C.c_uint), ("interval_samples", C.c_uint32), ("hist_bins", C.c_int),
                ("hist_range", C.c_double), ("max_records", C.c_int)]


class MonitorInfo(C.Structure):
    _fields_ = [("struct_size", C.c_uint), ("hist_bins", C.c_int), ("psd_bins", C.c_int),
                ("records_complete", C.c_uint64), ("records_dropped", C.c_uint64), ("first_unread", C.c_uint64),
                ("records_ready", C.c_uint64), ("interval_samples", C.c_uint32), ("max_records", C.c_int),
                ("hist_range", C.c_double), ("bin_hz", C.c_double)]


class MonitorLevels(C.Structure):
    _fields_ = [("struct_size", C.c_uint), ("reserved", C.c_int), ("tuning_offset_hz", C.c_double),
                ("peak_deviation_hz", C.c_double), ("rms", C.c_double), ("mpx_power_dbr", C.c_double),
                ("pilot_deviation_hz", C.c_double), ("rds_deviation_hz", C.c_double), ("hf_noise_density", C.c_double),
                ("n_finite", C.c_uint64), ("segments", C.c_uint64)]


class RfMonitorConfig(C.Structure):
    _fields_ = [("struct_size", C.c_uint), ("interval_samples", C.c_uint32), ("max_records", C.c_int)]


class RfMonitorInfo(C.Structure):
    _fields_ = [("struct_size", C.c_uint), ("hist_bins", C.c_int), ("psd_bins", C.c_int),
                ("records_complete", C.c_uint64), ("records_dropped", C.c_uint64), ("first_unread", C.c_uint64),
                ("records_ready", C.c_uint64), ("interval_samples", C.c_uint32), ("max_records", C.c_int),
                ("bin_hz", C.c_double)]


class RfMonitorLevels(C.Structure):
    _fields_ = [("struct_size", C.c_uint), ("reserved", C.c_int), ("level_dbfs", C.c_double), ("carrier_dbfs", C.c_double),
                ("noise_dbfs", C.c_double), ("cn_db", C.c_double), ("am_rms", C.c_double), ("am_audio_db", C.c_double),
                ("am_pilot_db", C.c_double), ("am_floor_dbc_hz", C.c_double), ("p10_dbfs", C.c_double),
                ("p50_dbfs", C.c_double), ("p90_dbfs", C.c_double), ("n_finite", C.c_uint64), ("segments", C.c_uint64)]


class WeakSignalConfig(C.Structure):
    _fields_ = [("struct_size", C.c_uint), ("mode", C.c_int), ("actions", C.c_uint), ("record_intervals", C.c_int),
                ("max_records", C.c_int), ("reserved", C.c_int), ("attack_ms", C.c_double), ("release_ms", C.c_double),
                ("blend_lo_db", C.c_double), ("blend_hi_db", C.c_double), ("highcut_lo_db", C.c_double),
                ("highcut_hi_db", C.c_double), ("mute_lo_db", C.c_double), ("mute_hi_db", C.c_double),
                ("highcut_hz", C.c_double), ("mute_floor_db", C.c_double)]


class WeakSignalInfo(C.Structure):
    _fields_ = [("struct_size", C.c_uint), ("channels", C.c_int), ("records_complete", C.c_uint64),
                ("records_dropped", C.c_uint64), ("first_unread", C.c_uint64), ("records_ready", C.c_uint64),
                ("intervals_complete", C.c_uint64), ("record_intervals", C.c_int), ("max_records", C.c_int),
                ("mode", C.c_int), ("actions", C.c_uint)]


class WeakSignalLevels(C.Structure):
    _fields_ = [("struct_size", C.c_uint), ("reserved", C.c_int), ("usn_mean_db", C.c_double), ("usn_peak_db", C.c_double),
                ("usn_mean_hz", C.c_double), ("usn_peak_hz", C.c_double), ("blend_share", C.c_double),
                ("highcut_share", C.c_double), ("mute_share", C.c_double), ("t_blend", C.c_double),
                ("t_highcut", C.c_double), ("t_mute", C.c_double), ("n_intervals", C.c_uint64), ("n_nonfinite", C.c_uint64)]


class BlankerConfig(C.Structure):
    _fields_ = [("struct_size", C.c_uint), ("mode", C.c_int), ("threshold_db", C.c_double), ("gate_samples", C.c_int),
                ("max_run_samples", C.c_int), ("average_intervals", C.c_int), ("record_intervals", C.c_int),
                ("max_records", C.c_int), ("reserved", C.c_int)]


class BlankerInfo(C.Structure):
    _fields_ = [("struct_size", C.c_uint), ("rows", C.c_int), ("records_complete", C.c_uint64),
                ("records_dropped", C.c_uint64), ("first_unread", C.c_uint64), ("records_ready", C.c_uint64),
                ("intervals_complete", C.c_uint64), ("mode", C.c_int), ("gate_samples", C.c_int),
                ("max_run_samples", C.c_int), ("average_intervals", C.c_int), ("record_intervals", C.c_int),
                ("max_records", C.c_int)]


class BlankerLevels(C.Structure):
    _fields_ = [("struct_size", C.c_uint), ("reserved", C.c_int), ("blanked_share", C.c_double),
                ("runs_per_second", C.c_double), ("level_dbfs", C.c_double), ("peak_dbfs", C.c_double),
                ("n_intervals", C.c_uint64), ("n_triggers", C.c_uint64), ("n_blanked", C.c_uint64),
                ("n_nonfinite", C.c_uint64), ("n_runs", C.c_uint64)]


class IqCorrectionConfig(C.Structure):
    _fields_ = [("struct_size", C.c_uint), ("mode", C.c_int), ("correct", C.c_int), ("average_intervals", C.c_int),
                ("record_intervals", C.c_int), ("max_records", C.c_int), ("reserved", C.c_int)]


class IqCorrectionInfo(C.Structure):
    _fields_ = [("struct_size", C.c_uint), ("rows", C.c_int), ("records_complete", C.c_uint64),
                ("records_dropped", C.c_uint64), ("first_unread", C.c_uint64), ("records_ready", C.c_uint64),
                ("intervals_complete", C.c_uint64), ("mode", C.c_int), ("correct", C.c_int),
                ("average_intervals", C.c_int), ("record_intervals", C.c_int), ("max_records", C.c_int),
                ("reserved", C.c_int)]


class IqCorrectionLevels(C.Structure):
    _fields_ = [("struct_size", C.c_uint), ("refused", C.c_int), ("dc_re", C.c_double), ("dc_im", C.c_double),
                ("dc_dbfs", C.c_double), ("w_re", C.c_double), ("w_im", C.c_double), ("image_rejection_db", C.c_double),
                ("gain_imbalance_db", C.c_double), ("phase_error_deg", C.c_double), ("usable_share", C.c_double),
                ("n_intervals", C.c_uint64), ("n_usable", C.c_uint64), ("n_nonfinite", C.c_uint64),
                ("n_skipped", C.c_uint64), ("n_refused", C.c_uint64)]


class LoudnessConfig(C.Structure):
    _fields_ = [("struct_size", C.c_uint), ("step_samples", C.c_uint32), ("max_records", C.c_int)]


class LoudnessInfo(C.Structure):
    _fields_ = [("struct_size", C.c_uint), ("channels", C.c_int), ("records_complete", C.c_uint64),
                ("records_dropped", C.c_uint64), ("first_unread", C.c_uint64), ("records_ready", C.c_uint64),
                ("step_samples", C.c_uint32), ("max_records", C.c_int)]


class LoudnessLevels(C.Structure):
    _fields_ = [("struct_size", C.c_uint), ("reserved", C.c_int), ("momentary_lufs", C.c_double),
                ("momentary_max_lufs", C.c_double), ("short_term_lufs", C.c_double), ("short_term_max_lufs", C.c_double),
                ("integrated_lufs", C.c_double), ("sample_peak_dbfs", C.c_double), ("true_peak_dbtp", C.c_double),
                ("correlation", C.c_double), ("side_to_mid_db", C.c_double), ("longest_silence_blocks", C.c_uint64),
                ("trailing_silence_blocks", C.c_uint64), ("n_nonfinite", C.c_uint64), ("momentary_windows", C.c_uint64),
                ("gated_windows", C.c_uint64)]


class AnalyserConfig(C.Structure):
    _fields_ = [("struct_size", C.c_uint), ("fft_size", C.c_int), ("interval_samples", C.c_uint32), ("max_records", C.c_int)]


class AnalyserInfo(C.Structure):
    _fields_ = [("struct_size", C.c_uint), ("channels", C.c_int), ("records_complete", C.c_uint64),
                ("records_dropped", C.c_uint64), ("first_unread", C.c_uint64), ("records_ready", C.c_uint64),
                ("interval_samples", C.c_uint32), ("max_records", C.c_int), ("fft_size", C.c_int), ("bins", C.c_int),
                ("bin_hz", C.c_double)]


class AnalyserRule(C.Structure):
    _fields_ = [("struct_size", C.c_uint), ("view", C.c_int), ("band_lo_hz", C.c_double), ("band_hi_hz", C.c_double),
                ("tone_hz", C.c_double), ("tone_search_hz", C.c_double), ("max_harmonic", C.c_int), ("reserved", C.c_int),
                ("min_tone_dbfs", C.c_double)]


class AnalyserLevels(C.Structure):
    _fields_ = [("struct_size", C.c_uint), ("tone_found", C.c_int), ("tone_hz", C.c_double), ("tone_dbfs", C.c_double),
                ("thd", C.c_double), ("thd_n", C.c_double), ("sinad_db", C.c_double), ("noise_dbfs", C.c_double),
                ("band_dbfs", C.c_double), ("harmonic_dbc", C.c_double * 8), ("dc", C.c_double), ("total_dbfs", C.c_double),
                ("segments", C.c_uint64), ("skipped", C.c_uint64), ("n_nonfinite", C.c_uint64),
                ("harmonics_counted", C.c_int), ("reserved", C.c_int)]


class OutputConfig(C.Structure):
    _fields_ = [("struct_size", C.c_uint), ("format", C.c_int), ("squelch_level", C.c_double), ("gain", C.c_double),
                ("max_frames", C.c_uint32), ("max_blocks", C.c_uint32)]


class OutputBlock(C.Structure):
    _fields_ = [("block", C.c_uint64), ("first_frame", C.c_uint64), ("n_frames", C.c_uint32), ("channels", C.c_uint32),
                ("if_rms", C.c_float), ("if_level", C.c_float), ("audio_mean", C.c_float), ("audio_rms", C.c_float),
                ("audio_level", C.c_float), ("gate_open", C.c_uint32), ("n_clipped", C.c_uint32),
                ("n_nonfinite", C.c_uint32)]


class OutputInfo(C.Structure):
    _fields_ = [("struct_size", C.c_uint), ("format", C.c_int), ("channels", C.c_int), ("first_frame", C.c_uint64),
                ("frames_waiting", C.c_uint64), ("frames_dropped", C.c_uint64), ("blocks_waiting", C.c_uint64),
                ("blocks_dropped", C.c_uint64)]


class OutputRateConfig(C.Structure):
    _fields_ = [("struct_size", C.c_uint), ("rate", C.c_int), ("mono", C.c_int), ("reserved", C.c_int)]


class OutputRateInfo(C.Structure):
    _fields_ = [("struct_size", C.c_uint), ("rate", C.c_int), ("channels", C.c_int), ("L", C.c_int), ("M", C.c_int),
                ("taps_per_phase", C.c_int), ("delay_frames", C.c_double), ("frames_in", C.c_uint64),
                ("pcm_clipped", C.c_uint64), ("pcm_nonfinite", C.c_uint64)]


class MpxOutputConfig(C.Structure):
    _fields_ = [("struct_size", C.c_uint), ("format", C.c_int), ("rate", C.c_int), ("gain", C.c_double),
                ("max_frames", C.c_uint32)]


class MpxOutputInfo(C.Structure):
    _fields_ = [("struct_size", C.c_uint), ("format", C.c_int), ("rate", C.c_int), ("L", C.c_int), ("M", C.c_int),
                ("taps_per_phase", C.c_int), ("delay_frames", C.c_double), ("full_scale_hz", C.c_double),
                ("first_frame", C.c_uint64), ("frames_waiting", C.c_uint64), ("frames_dropped", C.c_uint64),
                ("samples_in", C.c_uint64), ("pcm_clipped", C.c_uint64), ("pcm_nonfinite", C.c_uint64)]


class MpxInputConfig(C.Structure):
    _fields_ = [("struct_size", C.c_uint), ("format", C.c_int), ("rate", C.c_int), ("gain", C.c_double), ("rds", C.c_int)]


class MpxInputInfo(C.Structure):
    _fields_ = [("struct_size", C.c_uint), ("format", C.c_int), ("rate", C.c_int), ("L", C.c_int), ("M", C.c_int),
                ("taps_per_phase", C.c_int), ("taps_per_sample", C.c_int), ("delay_samples", C.c_double),
                ("full_scale_hz", C.c_double), ("frames_in", C.c_uint64), ("samples_out", C.c_uint64),
                ("nonfinite_in", C.c_uint64)]


def build_library(force=False, verbose=False):
    """Compile the HIP library (and its A/B partner build) in-tree for gfx950 (hipcc cross-compiles without a GPU)."""
    import glob
    deps = sorted(glob.glob(os.path.join(_DIR, "csrc", "*")))      # every header of the translation unit
    deps.append(os.path.join(os.path.dirname(_DIR), "include", "fmradion_amd.h"))
    deps.append(os.path.join(_DIR, "host", "fmradion_rds.hpp"))          # (the library's RDS entry point compiles it in)
    procs = []
    for path, extra in ((LIB_PATH, []), (LIB_PATH_AB, ["-DFMR_AB_PARTNERS"])):
        if not force and os.path.exists(path) and all(os.path.getmtime(path) >= os.path.getmtime(d) for d in deps):
            continue
        cmd = ["hipcc"] + HIPCC_FLAGS + extra + ["-o", path, SRC]
        if verbose:
            print(" ".join(cmd))
        procs.append((cmd, subprocess.Popen(cmd)))
    for cmd, pr in procs:
        if pr.wait() != 0:
            raise subprocess.CalledProcessError(pr.returncode, cmd)
    return LIB_PATH


_libs = {}


def lib(ab=False):
    """The product library; ab=True: its A/B partner build (tests only)."""
    if ab in _libs:
        return _libs[ab]
    path = LIB_PATH_AB if ab else LIB_PATH
    if not os.path.exists(path):
        raise FmrError(f"{path} is missing: run __graft_entry__.build() (there is no CPU fallback)" if not ab else
                       f"{path} (the A/B partner build two GPU tests load) is missing: run __graft_entry__.build()")
    L = C.CDLL(path)
    vp, u32p, fp, dp = C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_float), C.POINTER(C.c_double)
    L.fmr_create.restype = C.c_int
    L.fmr_create.argtypes = [C.POINTER(Config), C.POINTER(vp)]
    L.fmr_destroy.restype = None
    L.fmr_destroy.argtypes = [vp]
    L.fmr_last_error.restype = C.c_char_p
    L.fmr_version.restype = C.c_char_p
    L.fmr_resampler_info.restype = C.c_longlong
    L.fmr_resampler_info.argtypes = [vp, C.c_int]
    L.fmr_process.restype = C.c_int
    L.fmr_process.argtypes = [vp, fp, C.c_size_t, dp, C.c_size_t, C.POINTER(C.c_size_t)]
    L.fmr_process_blocks.restype = C.c_int
    L.fmr_process_blocks.argtypes = [vp, fp, C.c_size_t, u32p, C.c_int, dp, C.c_size_t, u32p]
    L.fmr_process_blocks_device.restype = C.c_int
    L.fmr_process_blocks_device.argtypes = [vp, vp, C.c_size_t, u32p, C.c_int, vp, C.c_size_t, u32p, C.c_int]
    L.fmr_synchronize.restype = C.c_int
    L.fmr_synchronize.argtypes = [vp]
    L.fmr_resample.restype = C.c_int
    L.fmr_resample.argtypes = [vp, fp, C.c_size_t, fp, C.c_size_t, C.POINTER(C.c_size_t)]
    L.fmr_create_channelizer.restype = C.c_int
    L.fmr_create_channelizer.argtypes = [C.POINTER(Config), C.c_size_t, C.POINTER(vp)]
    L.fmr_resample_blocks.restype = C.c_int
    L.fmr_resample_blocks.argtypes = [vp, vp, C.c_size_t, u32p, C.c_int, vp, C.c_size_t, u32p]
    L.fmr_resample_blocks_device.restype = C.c_int
    L.fmr_resample_blocks_device.argtypes = [vp, vp, C.c_size_t, u32p, C.c_int, vp, C.c_size_t, u32p, C.c_int]
    L.fmr_get_status.restype = C.c_int
    L.fmr_get_status.argtypes = [vp, C.c_int, C.POINTER(Status)]
    L.fmr_get_pps_events.restype = C.c_int
    L.fmr_get_pps_events.argtypes = [vp, C.c_int, C.POINTER(PpsEvent), C.c_int]
    L.fmr_get_multipath_coefficients.restype = C.c_int
    L.fmr_get_multipath_coefficients.argtypes = [vp, C.c_int, fp, C.c_int]
    L.fmr_debug_read.restype = C.c_longlong
    L.fmr_debug_read.argtypes = [vp, C.c_int, C.c_int, vp, C.c_size_t]
    L.fmr_debug_live_resources.restype = C.c_longlong
    L.fmr_debug_live_resources.argtypes = []
    L.fmr_get_kernel_times.restype = C.c_int
    L.fmr_get_kernel_times.argtypes = [vp, C.POINTER(C.c_char_p), fp, C.c_int]
    L.fmr_enable_kernel_timing.restype = None
    L.fmr_enable_kernel_timing.argtypes = [vp, C.c_int]
    L.fmr_fourth_convert.restype = C.c_int
    L.fmr_fourth_convert.argtypes = [vp, fp, C.c_size_t, fp, C.c_int, C.POINTER(C.c_uint)]
    L.fmr_design_taps.restype = C.c_longlong
    L.fmr_design_taps.argtypes = [C.c_double, C.c_double, C.c_double, C.c_int, dp, C.c_longlong, C.POINTER(C.c_longlong)]
    L.fmr_design_taps_class.restype = C.c_longlong
    L.fmr_design_taps_class.argtypes = [C.c_double, C.c_double, C.c_int, C.c_int, dp, C.c_longlong, C.POINTER(C.c_longlong)]
    L.fmr_filter_table.restype = C.c_int
    L.fmr_filter_table.argtypes = [C.c_char_p, C.POINTER(vp), C.POINTER(C.c_int)]
    L.fmr_spectrum_create.restype = C.c_int
    L.fmr_spectrum_create.argtypes = [C.POINTER(SpectrumConfig), C.c_size_t, C.POINTER(vp)]
    L.fmr_spectrum_destroy.restype = None
    L.fmr_spectrum_destroy.argtypes = [vp]
    L.fmr_spectrum_process.restype = C.c_int
    L.fmr_spectrum_process.argtypes = [vp, vp, C.c_size_t, C.c_size_t]
    L.fmr_spectrum_process_device.restype = C.c_int
    L.fmr_spectrum_process_device.argtypes = [vp, vp, C.c_size_t, C.c_size_t, C.c_int]
    L.fmr_spectrum_synchronize.restype = C.c_int
    L.fmr_spectrum_synchronize.argtypes = [vp]
    L.fmr_spectrum_read.restype = C.c_int
    L.fmr_spectrum_read.argtypes = [vp, C.c_int, C.c_int, dp, C.c_size_t, C.POINTER(SpectrumInfo)]
    L.fmr_spectrum_reset.restype = C.c_int
    L.fmr_spectrum_reset.argtypes = [vp]
    L.fmr_spectrum_create_waterfall.restype = C.c_int
    L.fmr_spectrum_create_waterfall.argtypes = [C.POINTER(SpectrumConfig), C.c_size_t, C.POINTER(WaterfallConfig), C.c_size_t,
                                                C.POINTER(vp)]
    L.fmr_spectrum_read_waterfall.restype = C.c_int
    L.fmr_spectrum_read_waterfall.argtypes = [vp, C.c_int, fp, u32p, C.c_size_t, C.POINTER(WaterfallInfo)]
    L.fmr_find_stations.restype = C.c_int
    L.fmr_find_stations.argtypes = [dp, C.c_int, C.c_double, C.POINTER(StationRule), C.POINTER(Station), C.c_int]
    L.fmr_enable_monitor.restype = C.c_int
    L.fmr_enable_monitor.argtypes = [vp, C.POINTER(MonitorConfig), C.c_size_t]
    L.fmr_monitor_read.restype = C.c_int
    L.fmr_monitor_read.argtypes = [vp, C.c_int, vp, vp, vp, C.c_int, C.POINTER(MonitorInfo), C.c_size_t]
    L.fmr_monitor_derive.restype = C.c_int
    L.fmr_monitor_derive.argtypes = [vp, vp, C.c_int, C.POINTER(MonitorLevels), C.c_size_t]
    L.fmr_enable_loudness.restype = C.c_int
    L.fmr_enable_loudness.argtypes = [vp, C.POINTER(LoudnessConfig), C.c_size_t]
    L.fmr_loudness_read.restype = C.c_int
    L.fmr_loudness_read.argtypes = [vp, C.c_int, vp, C.c_int, C.POINTER(LoudnessInfo), C.c_size_t]
    L.fmr_loudness_derive.restype = C.c_int
    L.fmr_loudness_derive.argtypes = [vp, C.c_int, C.c_double, C.POINTER(LoudnessLevels), C.c_size_t]
    L.fmr_enable_analyser.restype = C.c_int
    L.fmr_enable_analyser.argtypes = [vp, C.POINTER(AnalyserConfig), C.c_size_t]
    L.fmr_analyser_read.restype = C.c_int
    L.fmr_analyser_read.argtypes = [vp, C.c_int, vp, vp, C.c_int, C.POINTER(AnalyserInfo), C.c_size_t]
    L.fmr_analyser_derive.restype = C.c_int
    L.fmr_analyser_derive.argtypes = [vp, vp, C.c_int, C.POINTER(AnalyserRule), C.c_size_t, C.POINTER(AnalyserLevels), C.c_size_t]
    L.fmr_enable_rf_monitor.restype = C.c_int
    L.fmr_enable_rf_monitor.argtypes = [vp, C.POINTER(RfMonitorConfig), C.c_size_t]
    L.fmr_rf_monitor_read.restype = C.c_int
    L.fmr_rf_monitor_read.argtypes = [vp, C.c_int, vp, vp, vp, C.c_int, C.POINTER(RfMonitorInfo), C.c_size_t]
    L.fmr_rf_monitor_derive.restype = C.c_int
    L.fmr_rf_monitor_derive.argtypes = [vp, vp, vp, C.c_int, C.POINTER(RfMonitorLevels), C.c_size_t]
    L.fmr_enable_output.restype = C.c_int
    L.fmr_enable_output.argtypes = [vp, C.POINTER(OutputConfig), C.c_size_t]
    L.fmr_set_output_rate.restype = C.c_int
    L.fmr_set_output_rate.argtypes = [vp, C.POINTER(OutputRateConfig), C.c_size_t]
    L.fmr_get_output_rate.restype = C.c_int
    L.fmr_get_output_rate.argtypes = [vp, C.c_int, C.POINTER(OutputRateInfo), C.c_size_t]
    L.fmr_output_rate_taps.restype = C.c_int
    L.fmr_output_rate_taps.argtypes = [C.c_int, dp, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.fmr_output_read.restype = C.c_int
    L.fmr_output_read.argtypes = [vp, C.c_int, vp, C.c_size_t, vp, C.c_int, C.POINTER(C.c_size_t), C.POINTER(OutputInfo),
                                  C.c_size_t]
    L.fmr_squelch_level_from_db.restype = C.c_double
    L.fmr_squelch_level_from_db.argtypes = [C.c_double]
    L.fmr_enable_mpx_output.restype = C.c_int
    L.fmr_enable_mpx_output.argtypes = [vp, C.POINTER(MpxOutputConfig), C.c_size_t]
    L.fmr_mpx_output_read.restype = C.c_int
    L.fmr_mpx_output_read.argtypes = [vp, C.c_int, vp, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(MpxOutputInfo), C.c_size_t]
    L.fmr_mpx_output_taps.restype = C.c_int
    L.fmr_mpx_output_taps.argtypes = [C.c_int, dp, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.fmr_create_mpx_decoder.restype = C.c_int
    L.fmr_create_mpx_decoder.argtypes = [C.POINTER(Config), C.c_size_t, C.POINTER(MpxInputConfig), C.c_size_t, C.POINTER(vp)]
    L.fmr_process_mpx_blocks.restype = C.c_int
    L.fmr_process_mpx_blocks.argtypes = [vp, vp, C.c_size_t, u32p, C.c_int, dp, C.c_size_t, u32p]
    L.fmr_process_mpx_blocks_device.restype = C.c_int
    L.fmr_process_mpx_blocks_device.argtypes = [vp, vp, C.c_size_t, u32p, C.c_int, vp, C.c_size_t, u32p, C.c_int]
    L.fmr_get_mpx_input_info.restype = C.c_int
    L.fmr_get_mpx_input_info.argtypes = [vp, C.c_int, C.POINTER(MpxInputInfo), C.c_size_t]
    L.fmr_mpx_input_geometry.restype = C.c_int
    L.fmr_mpx_input_geometry.argtypes = [C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), dp]
    L.fmr_debug_mpx_chain_shape.restype = C.c_int
    L.fmr_debug_mpx_chain_shape.argtypes = [C.POINTER(Config), C.c_size_t, C.POINTER(MpxInputConfig), C.c_size_t,
                                            C.POINTER(ChainShapeInfo), C.c_size_t]
    L.fmr_enable_weak_signal.restype = C.c_int
    L.fmr_enable_weak_signal.argtypes = [vp, C.POINTER(WeakSignalConfig), C.c_size_t]
    L.fmr_weak_signal_read.restype = C.c_int
    L.fmr_weak_signal_read.argtypes = [vp, C.c_int, vp, C.c_int, C.POINTER(WeakSignalInfo), C.c_size_t]
    L.fmr_weak_signal_derive.restype = C.c_int
    L.fmr_weak_signal_derive.argtypes = [vp, C.c_int, C.POINTER(WeakSignalLevels), C.c_size_t]
    L.fmr_enable_blanker.restype = C.c_int
    L.fmr_enable_blanker.argtypes = [vp, C.POINTER(BlankerConfig), C.c_size_t]
    L.fmr_blanker_read.restype = C.c_int
    L.fmr_blanker_read.argtypes = [vp, C.c_int, vp, C.c_int, C.POINTER(BlankerInfo), C.c_size_t]
    L.fmr_blanker_derive.restype = C.c_int
    L.fmr_blanker_derive.argtypes = [vp, C.c_int, C.c_double, C.POINTER(BlankerLevels), C.c_size_t]
    L.fmr_enable_iq_correction.restype = C.c_int
    L.fmr_enable_iq_correction.argtypes = [vp, C.POINTER(IqCorrectionConfig), C.c_size_t]
    L.fmr_iq_correction_read.restype = C.c_int
    L.fmr_iq_correction_read.argtypes = [vp, C.c_int, vp, C.c_int, C.POINTER(IqCorrectionInfo), C.c_size_t]
    L.fmr_iq_correction_derive.restype = C.c_int
    L.fmr_iq_correction_derive.argtypes = [vp, C.c_int, C.POINTER(IqCorrectionLevels), C.c_size_t]
    _libs[ab] = L
    return L


def filter_table(name):
    """FilterParameters::<name> (include/FilterParameters.h:31-49) as a numpy array."""
    p, dbl = C.c_void_p(), C.c_int()
    n = lib().fmr_filter_table(name.encode(), C.byref(p), C.byref(dbl))
    if n < 0:
        raise FmrError(f"unknown filter table {name}")
    ct = C.c_double if dbl.value else C.c_float
    return np.ctypeslib.as_array(C.cast(p, C.POINTER(ct)), shape=(n,)).copy()


def design_taps(in_rate, out_rate, atten_db, stage):
    """The product's resampler design (host arithmetic of csrc/design.hpp; no GPU needed): (taps, info dict)."""
    info = (C.c_longlong * 6)()
    n = lib().fmr_design_taps(in_rate, out_rate, atten_db, stage, None, 0, info)
    if n < 0:
        raise FmrError(f"fmr_design_taps failed ({n}): {lib().fmr_last_error().decode()}")
    buf = np.empty(n, dtype=np.float64)
    lib().fmr_design_taps(in_rate, out_rate, atten_db, stage, buf.ctypes.data_as(C.POINTER(C.c_double)), n, info)
    d = dict(zip(["D", "NA", "LB", "MB", "TB", "LT"], [int(v) for v in info]))
    rows = d["LT"] + 1 if d["LT"] else d["LB"]          # fractional-phase form: LT + 1 rows, interpolated
    return (buf.reshape(rows, d["TB"]) if stage else buf), d


def design_taps_class(in_rate, out_rate, resampler_class, stage):
    """IfResampler(in_rate, out_rate) of a resampler class (RESAMPLER_FAST / RESAMPLER_R8B): (taps, info dict)."""
    info = (C.c_longlong * 6)()
    n = lib().fmr_design_taps_class(in_rate, out_rate, resampler_class, stage, None, 0, info)
    if n < 0:
        raise FmrError(f"fmr_design_taps_class failed ({n}): {lib().fmr_last_error().decode()}")
    buf = np.empty(n, dtype=np.float64)
    lib().fmr_design_taps_class(in_rate, out_rate, resampler_class, stage, buf.ctypes.data_as(C.POINTER(C.c_double)), n, info)
    d = dict(zip(["D", "NA", "LB", "MB", "TB", "LT"], [int(v) for v in info]))
    rows = d["LT"] + 1 if d["LT"] else d["LB"]
    return (buf.reshape(rows, d["TB"]) if stage else buf), d


def debug_live_resources(ab=False):
    """fmr_debug_live_resources: device buffers, pinned blocks, events and streams the library holds in this process."""
    return lib(ab=ab).fmr_debug_live_resources()


def probe_shader_clock(device=0):
    """The shader clock of the device right now [MHz] (a 20 us count on one wave)."""
    out = C.c_double(0.0)
    L = lib()
    L.fmr_probe_shader_clock.restype = C.c_int
    L.fmr_probe_shader_clock.argtypes = [C.c_int, C.POINTER(C.c_double)]
    rc = L.fmr_probe_shader_clock(int(device), C.byref(out))
    if rc != 0:
        raise FmrError(f"fmr_probe_shader_clock failed ({rc}): {L.fmr_last_error().decode()}")
    return out.value


def probe_read_bandwidth(device, dev_ptr, nbytes, reps=5):
    """GB/s of a plain streaming-read kernel over device memory [dev_ptr, dev_ptr + nbytes): what this box delivers."""
    out = C.c_double(0.0)
    L = lib()
    L.fmr_probe_read_bandwidth.restype = C.c_int
    L.fmr_probe_read_bandwidth.argtypes = [C.c_int, C.c_void_p, C.c_size_t, C.c_int, C.POINTER(C.c_double)]
    rc = L.fmr_probe_read_bandwidth(int(device), C.c_void_p(int(dev_ptr)), int(nbytes), int(reps), C.byref(out))
    if rc != 0:
        raise FmrError(f"fmr_probe_read_bandwidth failed ({rc}): {L.fmr_last_error().decode()}")
    return out.value


class RdsStatus(C.Structure):
    _fields_ = [("synced", C.c_int), ("reserved", C.c_int), ("blocks_ok", C.c_uint64), ("blocks_corrected", C.c_uint64),
                ("blocks_bad", C.c_uint64), ("groups_decoded", C.c_uint64), ("groups_dropped", C.c_uint64),
                ("injection", C.c_double), ("timing", C.c_double), ("carrier_phase", C.c_double),
                ("carrier_offset_hz", C.c_double)]


class RdsFec(C.Structure):
    _fields_ = [("struct_size", C.c_uint), ("mode", C.c_int), ("max_burst", C.c_int), ("soft_symbols", C.c_int),
                ("soft_max_cost", C.c_double)]


def squelch_level_from_db(db):
    """fmr_squelch_level_from_db (host only): the linear squelch level of the reference's -l option, pow(10, -(db / 20))."""
    return lib().fmr_squelch_level_from_db(float(db))


def loudness_levels(records, silence_dbfs=-60.0):
    """fmr_loudness_derive (host only): loudness, peaks, stereo and silence figures of the records (a LOUDNESS_RECORD
    array in ascending order, as Chain.loudness_records returns them), as a dict of fmr_loudness_levels."""
    L = lib()
    records = np.ascontiguousarray(records, dtype=LOUDNESS_RECORD)
    out = LoudnessLevels()
    rc = L.fmr_loudness_derive(records.ctypes.data, len(records), float(silence_dbfs), C.byref(out), C.sizeof(LoudnessLevels))
    if rc != OK:
        raise FmrError(f"fmr_loudness_derive failed ({rc}): {L.fmr_last_error().decode()}")
    return {k: getattr(out, k) for k, _ in LoudnessLevels._fields_ if k not in ("struct_size", "reserved")}


def blanker_levels(records, rate):
    """fmr_blanker_derive (host only): blanked_share, runs_per_second (at `rate` input samples per second), level_dbfs,
    peak_dbfs and the pooled counts of the records (a BLANKER_RECORD array as Chain.blanker_records returns them), as a dict
    of fmr_blanker_levels."""
    L = lib()
    records = np.ascontiguousarray(records, dtype=BLANKER_RECORD)
    out = BlankerLevels()
    rc = L.fmr_blanker_derive(records.ctypes.data, len(records), float(rate), C.byref(out), C.sizeof(BlankerLevels))
    if rc != OK:
        raise FmrError(f"fmr_blanker_derive failed ({rc}): {L.fmr_last_error().decode()}")
    return {k: getattr(out, k) for k, _ in BlankerLevels._fields_ if k not in ("struct_size", "reserved")}


def iq_correction_levels(records):
    """fmr_iq_correction_derive (host only): the DC offset, the image coefficient w, the image rejection of the uncorrected
    capture, gain imbalance and phase error, usable_share and the pooled counts of the records (an IQ_CORRECTION_RECORD
    array as Chain.iq_correction_records returns them), as a dict of fmr_iq_correction_levels."""
    L = lib()
    records = np.ascontiguousarray(records, dtype=IQ_CORRECTION_RECORD)
    out = IqCorrectionLevels()
    rc = L.fmr_iq_correction_derive(records.ctypes.data, len(records), C.byref(out), C.sizeof(IqCorrectionLevels))
    if rc != OK:
        raise FmrError(f"fmr_iq_correction_derive failed ({rc}): {L.fmr_last_error().decode()}")
    return {k: getattr(out, k) for k, _ in IqCorrectionLevels._fields_ if k != "struct_size"}


def weak_signal_levels(records):
    """fmr_weak_signal_derive (host only): the pooled ultrasonic noise, the share of intervals with each action engaged and
    the last control values of the records (a WEAK_SIGNAL_RECORD array as Chain.weak_signal_records returns them), as a
    dict of fmr_weak_signal_levels."""
    L = lib()
    records = np.ascontiguousarray(records, dtype=WEAK_SIGNAL_RECORD)
    out = WeakSignalLevels()
    rc = L.fmr_weak_signal_derive(records.ctypes.data, len(records), C.byref(out), C.sizeof(WeakSignalLevels))
    if rc != OK:
        raise FmrError(f"fmr_weak_signal_derive failed ({rc}): {L.fmr_last_error().decode()}")
    return {k: getattr(out, k) for k, _ in WeakSignalLevels._fields_ if k not in ("struct_size", "reserved")}


def analyser_levels(records, spectra, view="L", band_lo_hz=0.0, band_hi_hz=0.0, tone_hz=0.0, tone_search_hz=0.0,
                    max_harmonic=0, min_tone_dbfs=0.0):
    """fmr_analyser_derive (host only): tone, THD, THD+N, SINAD and noise of the pooled records (an ANALYSER_RECORD array
    with spectra [n, 3, N / 2 + 1], as Chain.analyser_records returns them) in view "L" | "R" | "M" | "S" (or 0 .. 3), as a
    dict of fmr_analyser_levels; every 0 is the rule's default."""
    L = lib()
    records = np.ascontiguousarray(records, dtype=ANALYSER_RECORD)
    spectra = np.ascontiguousarray(spectra, dtype=np.float64)
    if spectra.size != len(records) * 3 * (int(records["fft_size"][0]) // 2 + 1 if len(records) else 0):
        raise FmrError(f"analyser_levels: spectra of shape {spectra.shape} do not belong to {len(records)} records")
    rule = AnalyserRule(C.sizeof(AnalyserRule), int(ANALYSER_VIEWS.get(view, view)), float(band_lo_hz), float(band_hi_hz),
                        float(tone_hz), float(tone_search_hz), int(max_harmonic), 0, float(min_tone_dbfs))
    out = AnalyserLevels()
    rc = L.fmr_analyser_derive(records.ctypes.data, spectra.ctypes.data, len(records), C.byref(rule), C.sizeof(AnalyserRule),
                               C.byref(out), C.sizeof(AnalyserLevels))
    if rc != OK:
        raise FmrError(f"fmr_analyser_derive failed ({rc}): {L.fmr_last_error().decode()}")
    d = {k: getattr(out, k) for k, _ in AnalyserLevels._fields_ if k not in ("struct_size", "reserved")}
    d["harmonic_dbc"] = [float(v) for v in out.harmonic_dbc]
    return d


def rf_levels(records, hist, psd):
    """fmr_rf_monitor_derive (host only): level, C/N, envelope AM and fade percentiles of the pooled records (an
    RF_MONITOR_RECORD array with hist [n, 384] and psd [n, 513], as Chain.rf_monitor_records returns them), as a dict of
    fmr_rf_monitor_levels."""
    records = np.ascontiguousarray(records, dtype=RF_MONITOR_RECORD)
    hist = np.ascontiguousarray(hist, dtype=np.uint32)
    psd = np.ascontiguousarray(psd, dtype=np.float64)
    assert hist.shape == (len(records), RF_HIST_BINS) and psd.shape == (len(records), RF_PSD_BINS), (hist.shape, psd.shape)
    out = RfMonitorLevels()
    L = lib()
    rc = L.fmr_rf_monitor_derive(records.ctypes.data, hist.ctypes.data, psd.ctypes.data, len(records), C.byref(out),
                                 C.sizeof(RfMonitorLevels))
    if rc != OK:
        raise FmrError(f"fmr_rf_monitor_derive failed ({rc}): {L.fmr_last_error().decode()}")
    return {k: getattr(out, k) for k, _ in RfMonitorLevels._fields_ if k not in ("struct_size", "reserved")}


def monitor_levels(records, psd):
    """fmr_monitor_derive (host only): the levels of the pooled records (a MONITOR_RECORD array and their psd [n, 513], as
    Chain.monitor_records returns them), as a dict of fmr_monitor_levels."""
    records = np.ascontiguousarray(records, dtype=MONITOR_RECORD)
    psd = np.ascontiguousarray(psd, dtype=np.float64)
    assert psd.shape == (len(records), MONITOR_PSD_BINS), psd.shape
    out = MonitorLevels()
    L = lib()
    rc = L.fmr_monitor_derive(records.ctypes.data, psd.ctypes.data, len(records), C.byref(out), C.sizeof(MonitorLevels))
    if rc != OK:
        raise FmrError(f"fmr_monitor_derive failed ({rc}): {L.fmr_last_error().decode()}")
    return {k: getattr(out, k) for k, _ in MonitorLevels._fields_ if k not in ("struct_size", "reserved")}


def _rds_ok(g, i):
    return (int(g["status"][i]) & RDS_BAD) == 0


def rds_pi(groups):
    """Programme identification: the most frequent block A among the groups whose block A is good (None: none)."""
    vals = [int(g["block"][0]) for g in groups if _rds_ok(g, 0)]
    return max(set(vals), key=vals.count) if vals else None


def rds_ps(groups):
    """Programme service name from the groups 0A / 0B (segment address in block B, two characters in block D); None
    until all four segments have been seen.  The latest value of each segment wins."""
    ps, seen = [" "] * 8, 0
    for g in groups:
        if not (_rds_ok(g, 1) and _rds_ok(g, 3)) or int(g["block"][1]) >> 12 != 0:
            continue
        seg, d = int(g["block"][1]) & 3, int(g["block"][3])
        ps[2 * seg], ps[2 * seg + 1] = chr(d >> 8), chr(d & 0xFF)
        seen |= 1 << seg
    return "".join(ps) if seen == 0xF else None


DELAY_3TAPS = np.array([0.0, 1.0, 0.0], dtype=np.float32)  # FilterParameters::delay_3taps_only_iq


def _make_config(mode, input_rate, enable_resampler, fourth_down, fmfilter_enable, filter_coeff, stereo, deemphasis_us,
                 pilot_shift, multipath_stages, max_block_len, max_blocks, n_streams, device, nbfm_freq_dev, input_format,
                 output_rate, resampler_class, in_order, channel_offsets_hz):
    """(fmr_config of Chain's arguments, the arrays it points to: keep them alive as long as the config is used)."""
    offsets = None
    if channel_offsets_hz is not None:
        offsets = (C.c_int32 * len(channel_offsets_hz))(*[int(f) for f in channel_offsets_hz])
        if n_streams == 1:
            n_streams = len(channel_offsets_hz)
        assert n_streams == len(channel_offsets_hz), "channel_offsets_hz needs n_streams entries"
    coeff = np.ascontiguousarray(DELAY_3TAPS if filter_coeff is None else filter_coeff, dtype=np.float32)
    cfg = Config()
    cfg.device, cfg.n_streams, cfg.mode, cfg.input_rate = device, n_streams, mode, float(input_rate)
    cfg.enable_resampler, cfg.enable_fourth_down = int(enable_resampler), int(fourth_down)
    cfg.fmfilter_enable = int(fmfilter_enable)
    cfg.filter_coeff = coeff.ctypes.data_as(C.POINTER(C.c_float))
    cfg.n_filter_coeff = len(coeff)
    cfg.stereo, cfg.deemphasis_us, cfg.pilot_shift = int(stereo), float(deemphasis_us), int(pilot_shift)
    cfg.multipath_stages = int(multipath_stages)
    cfg.max_block_len, cfg.max_blocks = int(max_block_len), int(max_blocks)
    cfg.nbfm_freq_dev = float(nbfm_freq_dev)
    cfg.input_format = int(input_format)
    cfg.output_rate = float(output_rate)
    cfg.resampler_class = int(resampler_class)
    cfg.struct_size = C.sizeof(Config)
    cfg.in_order = int(bool(in_order))
    if offsets is not None:
        cfg.channel_offset_hz = offsets
    return cfg, (coeff, offsets)


class ChainShapeInfo(C.Structure):
    _fields_ = [("struct_size", C.c_uint), ("D", C.c_int), ("NA", C.c_int), ("LB", C.c_longlong), ("MB", C.c_longlong),
                ("TB", C.c_int), ("LT", C.c_int), ("stage_b", C.c_uint), ("fused", C.c_int), ("decim16", C.c_int),
                ("poly5h_disc", C.c_int), ("fir", C.c_int), ("qa", C.c_int), ("pipelined", C.c_int),
                ("max_if", C.c_uint64), ("max_au", C.c_uint64), ("mpx_in", C.c_int), ("mpx_format", C.c_int),
                ("mpx_L", C.c_int), ("mpx_M", C.c_int), ("mpx_T", C.c_int), ("mpx_K", C.c_int)]


ChainShape = collections.namedtuple("ChainShape", "design stage_b fused decim16 poly5h_disc fir qa pipelined max_if max_au")


def chain_shape(mode=MODE_FM, input_rate=384000.0, enable_resampler=False, fourth_down=False, fmfilter_enable=False,
                filter_coeff=None, stereo=True, deemphasis_us=50.0, pilot_shift=False, multipath_stages=0,
                max_block_len=65536, max_blocks=1, n_streams=1, device=0, nbfm_freq_dev=0.0, input_format=0, output_rate=0.0,
                resampler_class=RESAMPLER_FAST, in_order=False, ab=False, channel_offsets_hz=None, enable_rds=False,
                channelizer=False):
    """fmr_debug_chain_shape: what creating Chain(...) (channelizer=True: fmr_create_channelizer) would decide before it
    builds anything -- no device is opened, so this runs without a GPU.  A configuration the create would refuse raises
    FmrError with the create's code (.code) and message (.message).  Otherwise: design (D, NA, LB, MB, TB, LT; None without
    the resampler), stage_b (FE_FORMS name of stage B of a call that takes no upgrade), fused (None, "if_only", "disc"),
    decim16, poly5h_disc, fir (None, "poly4_disc", "poly4_finish"), qa, pipelined, max_if, max_au."""
    cfg, _keep = _make_config(mode, input_rate, enable_resampler, fourth_down, fmfilter_enable, filter_coeff, stereo,
                              deemphasis_us, pilot_shift, multipath_stages, max_block_len, max_blocks, n_streams, device,
                              nbfm_freq_dev, input_format, output_rate, resampler_class, in_order, channel_offsets_hz)
    return chain_shape_config(cfg, channelizer=channelizer, ab=ab)


def chain_shape_config(cfg, channelizer=False, ab=False):
    """chain_shape for an fmr_config (Config) filled in by the caller."""
    L = lib(ab=bool(ab))
    L.fmr_debug_chain_shape.restype = C.c_int
    L.fmr_debug_chain_shape.argtypes = [C.POINTER(Config), C.c_size_t, C.c_int, C.POINTER(ChainShapeInfo), C.c_size_t]
    o = ChainShapeInfo()
    rc = L.fmr_debug_chain_shape(C.byref(cfg), C.sizeof(Config), int(bool(channelizer)), C.byref(o), C.sizeof(ChainShapeInfo))
    if rc != OK:
        e = FmrError(f"fmr_debug_chain_shape failed ({rc}): {L.fmr_last_error().decode()}")
        e.code, e.message = rc, L.fmr_last_error().decode()
        raise e
    b = [k for k, bit in FE_FORMS.items() if bit == o.stage_b]
    return ChainShape({k: int(getattr(o, k)) for k in ("D", "NA", "LB", "MB", "TB", "LT")} if cfg.enable_resampler else None,
                      b[0] if b else None, [None, "if_only", "disc"][o.fused], bool(o.decim16), bool(o.poly5h_disc),
                      [None, "poly4_disc", "poly4_finish"][o.fir], o.qa, bool(o.pipelined), int(o.max_if), int(o.max_au))


class Chain:
    """One decoder chain (fmr_chain) for n_streams independent IQ streams."""

    def __init__(self, mode=MODE_FM, input_rate=384000.0, enable_resampler=False, fourth_down=False,
                 fmfilter_enable=False, filter_coeff=None, stereo=True, deemphasis_us=50.0, pilot_shift=False,
                 multipath_stages=0, max_block_len=65536, max_blocks=1, n_streams=1, device=0, nbfm_freq_dev=0.0, input_format=0,
                 output_rate=0.0, resampler_class=RESAMPLER_FAST, in_order=False, ab=False, channel_offsets_hz=None,
                 enable_rds=False):
        """channel_offsets_hz: a channel bank -- n_streams offsets [Hz] (n_streams may be left at 1: it follows the
        list); every iq argument then holds one row, the capture, and stream s decodes the station at +offset[s] Hz.
        enable_rds: the chain is made by fmr_create_rds (RDS groups of every stream: rds_groups / rds_status)."""
        self.enable_rds = bool(enable_rds)
        self._L = lib(ab=bool(ab))
        self.bank = channel_offsets_hz is not None
        cfg, self._keep = _make_config(mode, input_rate, enable_resampler, fourth_down, fmfilter_enable, filter_coeff, stereo,
                                       deemphasis_us, pilot_shift, multipath_stages, max_block_len, max_blocks, n_streams,
                                       device, nbfm_freq_dev, input_format, output_rate, resampler_class, in_order,
                                       channel_offsets_hz)
        n_streams = cfg.n_streams
        self.input_format = int(input_format)
        self.n_streams, self.mode, self.stereo = n_streams, mode, bool(stereo) and mode == MODE_FM
        self.h = C.c_void_p()
        rc = self._create(cfg)
        if rc != OK:
            self.h = None
            raise FmrError(f"{self._CREATE} failed ({rc}): {self._L.fmr_last_error().decode()}")

    _CREATE = "fmr_create"

    def _create(self, cfg):
        if self.enable_rds:
            self._CREATE = "fmr_create_rds"
            L = self._L
            L.fmr_create_rds.restype = C.c_int
            L.fmr_create_rds.argtypes = [C.POINTER(Config), C.c_size_t, C.POINTER(C.c_void_p)]
            return L.fmr_create_rds(C.byref(cfg), C.sizeof(Config), C.byref(self.h))
        return self._L.fmr_create(C.byref(cfg), C.byref(self.h))

    def close(self):
        if getattr(self, "h", None) and getattr(self, "_L", None) is not None:
            self._L.fmr_destroy(self.h)
        self.h = None

    def __del__(self):
        self.close()

    def _chk(self, rc):
        if rc < 0:
            raise FmrError(f"fmradion_amd error {rc}: {self._L.fmr_last_error().decode()}")
        return rc

    def resampler_info(self):
        return {k: self._L.fmr_resampler_info(self.h, i) for i, k in enumerate(["D", "NA", "LB", "MB", "TB", "LT"])}

    def front_end_forms(self):
        """Names (FE_FORMS) of the IF-resampler kernel forms this chain has launched since create, both stages."""
        mask = self._L.fmr_resampler_info(self.h, 6) | self._L.fmr_resampler_info(self.h, 7)
        return {k for k, bit in FE_FORMS.items() if mask >= 0 and mask & bit}

    def channel_bank_forms(self):
        """Names (CB_FORMS) of the channel-bank kernel forms this chain has launched since create (empty: no bank)."""
        mask = self._L.fmr_resampler_info(self.h, 8)
        return {k for k, bit in CB_FORMS.items() if mask >= 0 and mask & bit}

    # --- host-buffer API ---------------------------------------------------------
    def process(self, iq):
        """FmDecoder::process / AmDecoder::process shape: one block in, audio doubles out."""
        iq = np.ascontiguousarray(iq, dtype=np.complex64)
        out = np.empty(2 * (len(iq) + 64), dtype=np.float64)
        n = C.c_size_t()
        self._chk(self._L.fmr_process(self.h, iq.ctypes.data_as(C.POINTER(C.c_float)), len(iq),
                                    out.ctypes.data_as(C.POINTER(C.c_double)), len(out), C.byref(n)))
        return out[:n.value].copy()

    def process_blocks(self, iq, block_len):
        """iq: (n_streams, N) complex64 (a channel bank: the capture, shape (N,) or (1, N)); block_len: consecutive block
        lengths. Returns (audio[S][total], audio_len)."""
        if self.input_format == IQ_CF32:
            iq = np.ascontiguousarray(np.atleast_2d(iq), dtype=np.complex64)
        else:   # raw formats: (n_streams, N, 2) interleaved I,Q of the format's integer type
            iq = np.ascontiguousarray(iq, dtype=_IQ_DTYPE[self.input_format])
            assert iq.ndim == 3 and iq.shape[2] == 2
        assert iq.shape[0] == (1 if self.bank else self.n_streams)
        bl = np.ascontiguousarray(block_len, dtype=np.uint32)
        assert int(bl.sum()) <= iq.shape[1]
        acap = 2 * (int(bl.sum()) + 64 * len(bl))
        audio = np.zeros((self.n_streams, acap), dtype=np.float64)
        alen = np.zeros(len(bl), dtype=np.uint32)
        u32p = C.POINTER(C.c_uint32)
        self._chk(self._L.fmr_process_blocks(self.h, iq.ctypes.data_as(C.POINTER(C.c_float)), iq.shape[1],
                                           bl.ctypes.data_as(u32p), len(bl),
                                           audio.ctypes.data_as(C.POINTER(C.c_double)), acap,
                                           alen.ctypes.data_as(u32p)))
        return audio[:, :int(alen.sum())].copy(), alen

    def fourth_convert(self, iq, index=0, up=False):
        """FourthConverterIQ::process on one block; returns (shifted block, new table index)."""
        iq = np.ascontiguousarray(iq, dtype=np.complex64)
        out = np.empty_like(iq)
        idx = C.c_uint(index)
        self._chk(self._L.fmr_fourth_convert(self.h, iq.ctypes.data_as(C.POINTER(C.c_float)), len(iq),
                                           out.ctypes.data_as(C.POINTER(C.c_float)), int(up), C.byref(idx)))
        return out, idx.value

    def resample(self, iq):
        iq = np.ascontiguousarray(iq, dtype=np.complex64)
        out = np.empty(len(iq) + 64, dtype=np.complex64)
        n = C.c_size_t()
        self._chk(self._L.fmr_resample(self.h, iq.ctypes.data_as(C.POINTER(C.c_float)), len(iq),
                                     out.ctypes.data_as(C.POINTER(C.c_float)), len(out), C.byref(n)))
        return out[:n.value].copy()

    def resample_blocks(self, iq, block_len):
        """Front end only, batched (fmr_resample_blocks): iq (n_streams, N) complex64 -- a channelizer: the capture, shape
        (N,) or (1, N); block_len: consecutive block lengths.  Returns (rows complex64 [n_streams, n], out_len)."""
        if self.input_format == IQ_CF32:
            iq = np.ascontiguousarray(np.atleast_2d(iq), dtype=np.complex64)
        else:   # raw formats: (n_streams, N, 2) interleaved I,Q of the format's integer type
            iq = np.ascontiguousarray(iq, dtype=_IQ_DTYPE[self.input_format])
            assert iq.ndim == 3 and iq.shape[2] == 2
        assert iq.shape[0] == (1 if self.bank else self.n_streams)
        bl = np.ascontiguousarray(block_len, dtype=np.uint32)
        assert int(bl.sum()) <= iq.shape[1]
        ocap = int(bl.sum()) + 64 * len(bl)
        out = np.zeros((self.n_streams, ocap), dtype=np.complex64)
        olen = np.zeros(len(bl), dtype=np.uint32)
        u32p = C.POINTER(C.c_uint32)
        self._chk(self._L.fmr_resample_blocks(self.h, iq.ctypes.data, iq.shape[1], bl.ctypes.data_as(u32p), len(bl),
                                            out.ctypes.data, ocap, olen.ctypes.data_as(u32p)))
        return out[:, :int(olen.sum())].copy(), olen

    # --- device-buffer API (pointers are raw device addresses, e.g. torch .data_ptr()) -------------
    def resample_blocks_device(self, d_iq_ptr, stream_stride, block_len, d_out_ptr, out_stride, sync=False):
        """fmr_resample_blocks_device: rows of out_stride complex samples at d_out_ptr; returns out_len (complete after
        synchronize() or a call with sync=True)."""
        bl = np.ascontiguousarray(block_len, dtype=np.uint32)
        olen = np.zeros(len(bl), dtype=np.uint32)
        u32p = C.POINTER(C.c_uint32)
        self._chk(self._L.fmr_resample_blocks_device(self.h, C.c_void_p(d_iq_ptr), stream_stride,
                                                   bl.ctypes.data_as(u32p), len(bl), C.c_void_p(d_out_ptr), out_stride,
                                                   olen.ctypes.data_as(u32p), int(sync)))
        return olen

    def process_blocks_device(self, d_iq_ptr, stream_stride, block_len, d_audio_ptr, audio_stride, sync=False):
        """A channel bank reads one row at d_iq_ptr (stream_stride is ignored)."""
        bl = np.ascontiguousarray(block_len, dtype=np.uint32)
        alen = np.zeros(len(bl), dtype=np.uint32)
        u32p = C.POINTER(C.c_uint32)
        self._chk(self._L.fmr_process_blocks_device(self.h, C.c_void_p(d_iq_ptr), stream_stride,
                                                  bl.ctypes.data_as(u32p), len(bl), C.c_void_p(d_audio_ptr),
                                                  audio_stride, alen.ctypes.data_as(u32p), int(sync)))
        return alen

    def synchronize(self):
        self._chk(self._L.fmr_synchronize(self.h))

    # --- getters -----------------------------------------------------------------------
    def status(self, stream=0):
        st = Status()
        self._chk(self._L.fmr_get_status(self.h, stream, C.byref(st)))
        return st

    def rds_groups(self, stream=0, cap=4096):
        """fmr_get_rds_groups: the groups decoded so far on `stream` (drained from its queue), as an RDS_GROUP array."""
        out = np.zeros(cap, dtype=RDS_GROUP)
        L = self._L
        L.fmr_get_rds_groups.restype = C.c_int
        L.fmr_get_rds_groups.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int]
        n = self._chk(L.fmr_get_rds_groups(self.h, int(stream), out.ctypes.data, cap))
        return out[:n].copy()

    def rds_status(self, stream=0):
        st = RdsStatus()
        L = self._L
        L.fmr_get_rds_status.restype = C.c_int
        L.fmr_get_rds_status.argtypes = [C.c_void_p, C.c_int, C.POINTER(RdsStatus), C.c_size_t]
        self._chk(L.fmr_get_rds_status(self.h, int(stream), C.byref(st), C.sizeof(RdsStatus)))
        return st

    def set_rds_correction(self, mode, max_burst=0, soft_symbols=0, soft_max_cost=0.0):
        """fmr_set_rds_correction: RDS_FEC_OFF / RDS_FEC_BURST / RDS_FEC_SOFT for every stream, from each decoder's next
        block boundary on (0 = the default: bursts of up to 2 bits, the 4 least reliable symbols, cost up to 1.0)."""
        fec = RdsFec(C.sizeof(RdsFec), int(mode), int(max_burst), int(soft_symbols), float(soft_max_cost))
        L = self._L
        L.fmr_set_rds_correction.restype = C.c_int
        L.fmr_set_rds_correction.argtypes = [C.c_void_p, C.POINTER(RdsFec), C.c_size_t]
        self._chk(L.fmr_set_rds_correction(self.h, C.byref(fec), C.sizeof(RdsFec)))

    def rds_reliabilities(self, stream=0, cap=1 << 16):
        """fmr_debug_read 5: the signed reliabilities rho_k of the symbols the most recent call decided (float32)."""
        buf = np.empty(cap, dtype=np.float32)
        n = self._chk(self._L.fmr_debug_read(self.h, int(stream), 5, buf.ctypes.data_as(C.c_void_p), buf.nbytes))
        return buf[:n].copy()

    def _read_records(self, read, info_cls, arrays, stream, cap):
        """The two-step read of a monitor's records: a probe (cap 0) that fills the info and says how many wait, then the
        read of at most `cap` records (None: all that wait).  arrays lists what the C function fills, in its order, as
        (dtype, columns): None for the records themselves, a number, or the name of the info field that holds it.
        Returns the arrays cut to the records read, then the info as a dict."""
        info = info_cls()
        tail = (C.byref(info), C.sizeof(info_cls))
        waiting = self._chk(read(self.h, int(stream), *([None] * len(arrays)), 0, *tail))
        cap = int(waiting if cap is None else cap)
        bufs = [np.zeros(cap if cols is None else (cap, int(getattr(info, cols) if isinstance(cols, str) else cols)), dtype=dt)
                for dt, cols in arrays]
        n = 0
        if cap > 0:
            n = self._chk(read(self.h, int(stream), *(b.ctypes.data for b in bufs), cap, *tail))
        return (*(b[:n] for b in bufs), {k: getattr(info, k) for k, _ in info_cls._fields_})

    def enable_monitor(self, interval_samples=0, hist_bins=0, hist_range=0.0, max_records=0):
        """fmr_enable_monitor: the modulation monitor of every stream / channel (FM chains, once, before the first call);
        0 = the defaults (one-second records, 256 bins over +-2.0, 64 records kept)."""
        cfg = MonitorConfig(C.sizeof(MonitorConfig), int(interval_samples), int(hist_bins), float(hist_range), int(max_records))
        self._chk(self._L.fmr_enable_monitor(self.h, C.byref(cfg), C.sizeof(MonitorConfig)))

    def monitor_records(self, stream=0, cap=None):
        """fmr_monitor_read: the oldest unread complete records of `stream` (at most cap; None: all that wait) as
        (records MONITOR_RECORD [n], hist uint32 [n, B], psd float64 [n, 513], info dict).  Reading drains them."""
        return self._read_records(self._L.fmr_monitor_read, MonitorInfo, ((MONITOR_RECORD, None), (np.uint32, "hist_bins"),
                                                                          (np.float64, MONITOR_PSD_BINS)), stream, cap)

    def enable_loudness(self, step_samples=0, max_records=0):
        """fmr_enable_loudness: the audio monitor of every stream / channel (FM chains, once, before the first call);
        0 = the defaults (sub-blocks of 4800 audio samples, 1024 records kept)."""
        cfg = LoudnessConfig(C.sizeof(LoudnessConfig), int(step_samples), int(max_records))
        self._chk(self._L.fmr_enable_loudness(self.h, C.byref(cfg), C.sizeof(LoudnessConfig)))

    def loudness_records(self, stream=0, cap=None):
        """fmr_loudness_read: the oldest unread complete records of `stream` (at most cap; None: all that wait) as
        (records LOUDNESS_RECORD [n], info dict).  Reading drains them."""
        return self._read_records(self._L.fmr_loudness_read, LoudnessInfo, ((LOUDNESS_RECORD, None),), stream, cap)

    def enable_weak_signal(self, act=False, actions=0, attack_ms=0.0, release_ms=0.0, blend_db=(0.0, 0.0),
                           highcut_db=(0.0, 0.0), mute_db=(0.0, 0.0), highcut_hz=0.0, mute_floor_db=0.0,
                           record_intervals=0, max_records=0):
        """fmr_enable_weak_signal: weak-signal handling of every stream / channel (FM chains, once, before the first
        call).  act=False measures and records only; act=True also applies stereo blend, high cut and soft mute (actions:
        WS_BLEND | WS_HIGHCUT | WS_MUTE) to the audio the chain returns.  *_db are (lo, hi) pairs in dB of the smoothed
        ultrasonic noise; 0 = the defaults (all three actions, 10 / 500 ms, 2500 Hz, -20 dB, records of 50 intervals,
        1024 kept)."""
        cfg = WeakSignalConfig(C.sizeof(WeakSignalConfig), WS_ACT if act else WS_MEASURE, int(actions), int(record_intervals),
                               int(max_records), 0, float(attack_ms), float(release_ms), float(blend_db[0]),
                               float(blend_db[1]), float(highcut_db[0]), float(highcut_db[1]), float(mute_db[0]),
                               float(mute_db[1]), float(highcut_hz), float(mute_floor_db))
        self._chk(self._L.fmr_enable_weak_signal(self.h, C.byref(cfg), C.sizeof(WeakSignalConfig)))

    def weak_signal_records(self, stream=0, cap=None):
        """fmr_weak_signal_read: the oldest unread complete records of `stream` (at most cap; None: all that wait) as
        (records WEAK_SIGNAL_RECORD [n], info dict).  Reading drains them."""
        return self._read_records(self._L.fmr_weak_signal_read, WeakSignalInfo, ((WEAK_SIGNAL_RECORD, None),), stream, cap)

    def enable_blanker(self, act=False, threshold_db=0.0, gate_samples=0, max_run_samples=0, average_intervals=0,
                       record_intervals=0, max_records=0):
        """fmr_enable_blanker: the impulse blanker on the input rows, in front of every front end (chains with the IF
        resampler on complex-float input, banks and channelizers included; once, before the first call).  act=False
        measures and records only; act=True zeroes the gated samples in what the front end reads.  0 = the defaults
        (12 dB over the mean of 16 intervals of 4096 samples, a gate of 0.8 us, runs of 8 gates at most, records of 256
        intervals, 1024 kept)."""
        cfg = BlankerConfig(C.sizeof(BlankerConfig), NB_ACT if act else NB_MEASURE, float(threshold_db), int(gate_samples),
                            int(max_run_samples), int(average_intervals), int(record_intervals), int(max_records), 0)
        self._chk(self._L.fmr_enable_blanker(self.h, C.byref(cfg), C.sizeof(BlankerConfig)))

    def blanker_records(self, row=0, cap=None):
        """fmr_blanker_read: the oldest unread complete records of input row `row` (0 for a bank or a channelizer; at most
        cap; None: all that wait) as (records BLANKER_RECORD [n], info dict).  Reading drains them."""
        return self._read_records(self._L.fmr_blanker_read, BlankerInfo, ((BLANKER_RECORD, None),), row, cap)

    def enable_iq_correction(self, act=False, correct=0, average_intervals=0, record_intervals=0, max_records=0):
        """fmr_enable_iq_correction: DC-offset and IQ-imbalance correction of the input rows, in front of the blanker and
        of every front end (chains with the IF resampler on complex-float input, banks and channelizers included; once,
        before the first call).  act=False measures and records only; act=True corrects what the blanker and the front
        end read.  correct: IQC_DC | IQC_BALANCE (0 = both).  0 = the defaults (a window of 64 intervals of 4096
        samples, records of 256 intervals, 1024 kept)."""
        cfg = IqCorrectionConfig(C.sizeof(IqCorrectionConfig), IQC_ACT if act else IQC_MEASURE, int(correct),
                                 int(average_intervals), int(record_intervals), int(max_records), 0)
        self._chk(self._L.fmr_enable_iq_correction(self.h, C.byref(cfg), C.sizeof(IqCorrectionConfig)))

    def iq_correction_records(self, row=0, cap=None):
        """fmr_iq_correction_read: the oldest unread complete records of input row `row` (0 for a bank or a channelizer;
        at most cap; None: all that wait) as (records IQ_CORRECTION_RECORD [n], info dict).  Reading drains them."""
        return self._read_records(self._L.fmr_iq_correction_read, IqCorrectionInfo, ((IQ_CORRECTION_RECORD, None),), row, cap)

    def enable_analyser(self, fft_size=0, interval_samples=0, max_records=0):
        """fmr_enable_analyser: the audio analyser of every stream / channel (any decoder chain, once, before the first
        call); 0 = the defaults (N = 4096, records of 6 N audio frames, 64 records kept)."""
        cfg = AnalyserConfig(C.sizeof(AnalyserConfig), int(fft_size), int(interval_samples), int(max_records))
        self._chk(self._L.fmr_enable_analyser(self.h, C.byref(cfg), C.sizeof(AnalyserConfig)))
        self._an_bins, self._an_ring = (int(fft_size) or 4096) // 2 + 1, int(max_records) or 64

    def analyser_records(self, stream=0, cap=None):
        """fmr_analyser_read: the oldest unread complete records of `stream` (at most cap; None: all that wait) as
        (records ANALYSER_RECORD [n], spectra float64 [n, 3, N / 2 + 1] scaled to power, info dict).  Reading drains them."""
        # one read, sized by the ring (no more than max_records can wait): every read synchronises the chain
        bins = getattr(self, "_an_bins", 1)      # (a chain without the analyser: the library refuses the read)
        cap = getattr(self, "_an_ring", 1) if cap is None else int(cap)
        recs, spectra = np.zeros(cap, dtype=ANALYSER_RECORD), np.empty((cap, 3, bins), dtype=np.float64)
        info = AnalyserInfo()
        n = self._chk(self._L.fmr_analyser_read(self.h, int(stream), recs.ctypes.data if cap else None,
                                                spectra.ctypes.data if cap else None, cap, C.byref(info), C.sizeof(AnalyserInfo)))
        n = n if cap else 0
        return recs[:n], spectra[:n], {k: getattr(info, k) for k, _ in AnalyserInfo._fields_}

    def enable_rf_monitor(self, interval_samples=0, max_records=0):
        """fmr_enable_rf_monitor: the RF monitor of every stream / channel (FM chains, once, before the first call);
        0 = the defaults (records of 38400 IF samples = 100 ms, 64 records kept)."""
        cfg = RfMonitorConfig(C.sizeof(RfMonitorConfig), int(interval_samples), int(max_records))
        self._chk(self._L.fmr_enable_rf_monitor(self.h, C.byref(cfg), C.sizeof(RfMonitorConfig)))

    def rf_monitor_records(self, stream=0, cap=None):
        """fmr_rf_monitor_read: the oldest unread complete records of `stream` (at most cap; None: all that wait) as
        (records RF_MONITOR_RECORD [n], hist uint32 [n, 384], psd float64 [n, 513], info dict).  Reading drains them."""
        return self._read_records(self._L.fmr_rf_monitor_read, RfMonitorInfo, ((RF_MONITOR_RECORD, None), (np.uint32, RF_HIST_BINS),
                                                                                (np.float64, RF_PSD_BINS)), stream, cap)

    def enable_output(self, format="s16", squelch_db=None, gain=0.0, max_frames=0, max_blocks=0, squelch_level=None,
                      rate=None, mono=False):
        """fmr_enable_output: the output stage of every stream / channel (any decoder chain, once, before the first call).
        format "s16" | "f32" (or PCM_S16 / PCM_F32); squelch_db as the reference's -l option (None: never closed), or
        squelch_level, the linear level itself; 0 = the defaults (gain 0.5, 2^18 frames and 4096 records kept).
        rate (Hz) and / or mono: fmr_set_output_rate behind it -- the PCM ring at that rate and / or downmixed."""
        fmt = {"s16": PCM_S16, "f32": PCM_F32}.get(format, format)
        level = 0.0 if squelch_db is None else squelch_level_from_db(squelch_db)
        if squelch_level is not None:
            level = float(squelch_level)
        cfg = OutputConfig(C.sizeof(OutputConfig), int(fmt), level, float(gain), int(max_frames), int(max_blocks))
        self._chk(self._L.fmr_enable_output(self.h, C.byref(cfg), C.sizeof(OutputConfig)))
        if rate is not None or mono:
            self.set_output_rate(0 if rate is None else rate, mono)

    def set_output_rate(self, rate=0, mono=False):
        """fmr_set_output_rate: once, behind enable_output and before the first call."""
        cfg = OutputRateConfig(C.sizeof(OutputRateConfig), int(rate), int(mono), 0)
        self._chk(self._L.fmr_set_output_rate(self.h, C.byref(cfg), C.sizeof(OutputRateConfig)))

    def output_rate_info(self, stream=0):
        """fmr_get_output_rate as a dict: rate, channels, L, M, taps_per_phase, delay_frames, frames_in, pcm_clipped,
        pcm_nonfinite."""
        info = OutputRateInfo()
        self._chk(self._L.fmr_get_output_rate(self.h, int(stream), C.byref(info), C.sizeof(OutputRateInfo)))
        return {k: getattr(info, k) for k, _ in OutputRateInfo._fields_ if k != "struct_size"}

    def output_read(self, stream=0, cap_frames=None, cap_blocks=None):
        """fmr_output_read: the oldest unread PCM frames (at most cap_frames; None: all that wait) and block records (at most
        cap_blocks; None: all) of `stream` as (pcm [n, channels] int16 | float32, blocks OUTPUT_BLOCK [m], info dict).
        Reading drains them."""
        info = OutputInfo()
        tail = (C.byref(info), C.sizeof(OutputInfo))
        self._chk(self._L.fmr_output_read(self.h, int(stream), None, 0, None, 0, None, *tail))
        nf = int(info.frames_waiting if cap_frames is None else cap_frames)
        nb = int(info.blocks_waiting if cap_blocks is None else cap_blocks)
        ch = int(info.channels)
        pcm = np.zeros((nf, ch), dtype=_PCM_DTYPE[int(info.format)])
        blocks = np.zeros(nb, dtype=OUTPUT_BLOCK)
        got = C.c_size_t(0)
        m = self._chk(self._L.fmr_output_read(self.h, int(stream), pcm.ctypes.data if nf else None, nf,
                                              blocks.ctypes.data if nb else None, nb, C.byref(got), *tail))
        return pcm[:got.value], blocks[:m], {k: getattr(info, k) for k, _ in OutputInfo._fields_}

    def enable_mpx_output(self, format="s16", rate=192000, gain=0.0, max_frames=0):
        """fmr_enable_mpx_output: the composite baseband of every stream / channel of an FM chain as mono PCM at `rate`
        (once, before the first call).  format "s16" | "f32" (or PCM_S16 / PCM_F32); rate 0 = 384000, the MPX as it is;
        0 = the defaults (gain 0.5: full scale +-150 kHz; 2^20 frames kept)."""
        fmt = {"s16": PCM_S16, "f32": PCM_F32}.get(format, format)
        cfg = MpxOutputConfig(C.sizeof(MpxOutputConfig), int(fmt), int(rate), float(gain), int(max_frames))
        self._chk(self._L.fmr_enable_mpx_output(self.h, C.byref(cfg), C.sizeof(MpxOutputConfig)))

    def mpx_output_read(self, stream=0, cap_frames=None):
        """fmr_mpx_output_read: the oldest unread frames of `stream` (at most cap_frames; None: all that wait) as
        (pcm [n] int16 | float32, info dict).  Reading drains them."""
        info = MpxOutputInfo()
        tail = (C.byref(info), C.sizeof(MpxOutputInfo))
        self._chk(self._L.fmr_mpx_output_read(self.h, int(stream), None, 0, None, *tail))
        nf = int(info.frames_waiting if cap_frames is None else cap_frames)
        pcm = np.zeros(nf, dtype=_PCM_DTYPE[int(info.format)])
        got = C.c_size_t(0)
        self._chk(self._L.fmr_mpx_output_read(self.h, int(stream), pcm.ctypes.data if nf else None, nf, C.byref(got), *tail))
        return pcm[:got.value], {k: getattr(info, k) for k, _ in MpxOutputInfo._fields_ if k != "struct_size"}

    def pps_events(self, stream=0):
        ev = (PpsEvent * 64)()
        n = self._chk(self._L.fmr_get_pps_events(self.h, stream, ev, 64))
        return [(e.pps_index, e.sample_index, e.block_position, e.block) for e in ev[:min(n, 64)]]

    def multipath_coefficients(self, stream=0):
        buf = np.empty(2 * 1300, dtype=np.float32)
        n = self._chk(self._L.fmr_get_multipath_coefficients(self.h, stream, buf.ctypes.data_as(C.POINTER(C.c_float)), len(buf)))
        return buf[:2 * n].view(np.complex64).copy()

    def debug_read(self, which, stream=0, cap=1 << 24):
        dt = {0: np.complex64, 1: np.float32, 2: np.float64, 3: np.float64, 4: np.float32, 5: np.uint64, 6: np.complex64,
              7: np.complex64}[which]
        buf = np.empty(cap, dtype=dt)
        n = self._chk(self._L.fmr_debug_read(self.h, stream, which, buf.ctypes.data_as(C.c_void_p), buf.nbytes))
        return buf[:n].copy()

    def enable_kernel_timing(self, mode=1):
        """0 off, 1 every kernel of the last call, 2 the dominant kernel only (accumulated over calls)."""
        self._L.fmr_enable_kernel_timing(self.h, int(mode))

    def kernel_trace(self, cap=1 << 16):
        """After enable_kernel_timing(3): [(name, stream, start_ms, end_ms)] of every instrumented kernel since then."""
        names = (C.c_char_p * cap)()
        st = (C.c_int * cap)()
        t0 = (C.c_float * cap)()
        t1 = (C.c_float * cap)()
        L = self._L
        L.fmr_get_kernel_trace.restype = C.c_int
        L.fmr_get_kernel_trace.argtypes = [C.c_void_p, C.POINTER(C.c_char_p), C.POINTER(C.c_int), C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int]
        n = self._chk(L.fmr_get_kernel_trace(self.h, names, st, t0, t1, cap))
        return [(names[i].decode(), st[i], t0[i], t1[i]) for i in range(min(n, cap))]

    def kernel_times(self, cap=4096):
        names = (C.c_char_p * cap)()
        ms = (C.c_float * cap)()
        n = self._chk(self._L.fmr_get_kernel_times(self.h, names, ms, cap))
        return [(names[i].decode(), ms[i]) for i in range(min(n, cap))]


def _mpx_configs(rate, format, gain, n_streams, stereo, deemphasis_us, pilot_shift, rds, max_block_len, max_blocks, device):
    """(fmr_config, fmr_mpx_input_config, keep-alive) of MpxChain's arguments."""
    cfg, keep = _make_config(MODE_FM, 0.0, False, False, False, None, stereo, deemphasis_us, pilot_shift, 0, max_block_len,
                             max_blocks, n_streams, device, 0.0, IQ_CF32, 0.0, RESAMPLER_FAST, False, None)
    cfg.filter_coeff, cfg.n_filter_coeff = None, 0       # (not needed: there is no IF filter)
    fmt = {"s16": PCM_S16, "f32": PCM_F32}.get(format, format)
    return cfg, MpxInputConfig(C.sizeof(MpxInputConfig), int(fmt), int(rate), float(gain), int(bool(rds))), keep


def mpx_chain_shape(rate=192000, format="s16", gain=0.0, n_streams=1, stereo=True, deemphasis_us=50.0, pilot_shift=False,
                    rds=False, max_block_len=65536, max_blocks=1, device=0):
    """fmr_debug_mpx_chain_shape: what creating MpxChain(...) would decide, without a device, as a dict of
    fmr_chain_shape_info's fields; a refusal raises FmrError with .code and .message."""
    L = lib()
    cfg, mi, _keep = _mpx_configs(rate, format, gain, n_streams, stereo, deemphasis_us, pilot_shift, rds, max_block_len,
                                  max_blocks, device)
    o = ChainShapeInfo()
    rc = L.fmr_debug_mpx_chain_shape(C.byref(cfg), C.sizeof(Config), C.byref(mi), C.sizeof(MpxInputConfig), C.byref(o),
                                     C.sizeof(ChainShapeInfo))
    if rc != OK:
        e = FmrError(f"fmr_debug_mpx_chain_shape failed ({rc}): {L.fmr_last_error().decode()}")
        e.code, e.message = rc, L.fmr_last_error().decode()
        raise e
    return {k: int(getattr(o, k)) for k, _ in ChainShapeInfo._fields_ if k != "struct_size"}


class MpxChain(Chain):
    """An FM decoder fed composite baseband (fmr_create_mpx_decoder): n_streams rows of mono PCM at `rate` -- int16
    ("s16") or float32 ("f32") -- instead of IQ.  rate 0 / 384000: the MPX as it is; gain 0 = 2.0.  Everything behind the
    front end is Chain's: status, pps_events, the monitors, the output stage, enable_mpx_output, and with rds=True
    rds_groups / rds_status / set_rds_correction."""

    _CREATE = "fmr_create_mpx_decoder"

    def __init__(self, rate=192000, format="s16", gain=0.0, n_streams=1, stereo=True, deemphasis_us=50.0, pilot_shift=False,
                 rds=False, max_block_len=65536, max_blocks=1, device=0):
        self._L = lib()
        self.enable_rds, self.bank, self.input_format = bool(rds), False, IQ_CF32
        cfg, self._mi, self._keep = _mpx_configs(rate, format, gain, n_streams, stereo, deemphasis_us, pilot_shift, rds,
                                                 max_block_len, max_blocks, device)
        self.format = int(self._mi.format)
        self.n_streams, self.mode, self.stereo = int(n_streams), MODE_FM, bool(stereo)
        self.h = C.c_void_p()
        rc = self._L.fmr_create_mpx_decoder(C.byref(cfg), C.sizeof(Config), C.byref(self._mi), C.sizeof(MpxInputConfig),
                                            C.byref(self.h))
        if rc != OK:
            self.h = None
            e = FmrError(f"{self._CREATE} failed ({rc}): {self._L.fmr_last_error().decode()}")
            e.code, e.message = rc, self._L.fmr_last_error().decode()
            raise e

    def process(self, pcm):
        """One block of one stream: frames in, audio doubles out."""
        pcm = np.ascontiguousarray(pcm, dtype=_PCM_DTYPE[self.format])
        assert pcm.ndim == 1 and self.n_streams == 1
        if len(pcm) == 0:
            return np.zeros(0, dtype=np.float64)
        audio, _ = self.process_blocks(pcm[None, :], [len(pcm)])
        return audio[0]

    def process_blocks(self, pcm, block_len):
        """pcm: (n_streams, N) int16 / float32 frames; block_len: consecutive block lengths in frames.  Returns
        (audio[S][total], audio_len)."""
        pcm = np.atleast_2d(np.asarray(pcm))
        assert pcm.dtype == _PCM_DTYPE[self.format], (pcm.dtype, self.format)
        pcm = np.ascontiguousarray(pcm)
        assert pcm.shape[0] == self.n_streams
        bl = np.ascontiguousarray(block_len, dtype=np.uint32)
        assert int(bl.sum()) <= pcm.shape[1]
        acap = int(bl.sum()) + 64 * len(bl) + 64      # (at most 4 MPX samples per frame, 2 doubles per 8 of them)
        audio = np.zeros((self.n_streams, acap), dtype=np.float64)
        alen = np.zeros(len(bl), dtype=np.uint32)
        u32p = C.POINTER(C.c_uint32)
        self._chk(self._L.fmr_process_mpx_blocks(self.h, pcm.ctypes.data, pcm.shape[1], bl.ctypes.data_as(u32p), len(bl),
                                                 audio.ctypes.data_as(C.POINTER(C.c_double)), acap, alen.ctypes.data_as(u32p)))
        return audio[:, :int(alen.sum())].copy(), alen

    def process_blocks_device(self, d_pcm_ptr, stream_stride, block_len, d_audio_ptr, audio_stride, sync=False):
        """fmr_process_mpx_blocks_device: rows of stream_stride frames at d_pcm_ptr (16-byte aligned rows and stride)."""
        bl = np.ascontiguousarray(block_len, dtype=np.uint32)
        alen = np.zeros(len(bl), dtype=np.uint32)
        u32p = C.POINTER(C.c_uint32)
        self._chk(self._L.fmr_process_mpx_blocks_device(self.h, C.c_void_p(d_pcm_ptr), stream_stride, bl.ctypes.data_as(u32p),
                                                        len(bl), C.c_void_p(d_audio_ptr), audio_stride,
                                                        alen.ctypes.data_as(u32p), int(sync)))
        return alen

    def mpx_input_info(self, stream=0):
        """fmr_get_mpx_input_info as a dict."""
        info = MpxInputInfo()
        self._chk(self._L.fmr_get_mpx_input_info(self.h, int(stream), C.byref(info), C.sizeof(MpxInputInfo)))
        return {k: getattr(info, k) for k, _ in MpxInputInfo._fields_ if k != "struct_size"}


class Channelizer(Chain):
    """Channelizer (fmr_create_channelizer): one wideband capture in, one row of IQ at output_rate per offset out -- row s
    is IfResampler(input_rate, output_rate) of the capture shifted down by offsets_hz[s] (the station at +offsets_hz[s]
    Hz).  output_rate 0 = 384 kHz."""

    _CREATE = "fmr_create_channelizer"

    def __init__(self, input_rate, offsets_hz, output_rate=0.0, resampler_class=RESAMPLER_FAST, max_block_len=65536,
                 max_blocks=1, device=0):
        super().__init__(mode=MODE_NONE, input_rate=input_rate, enable_resampler=True, max_block_len=max_block_len,
                         max_blocks=max_blocks, device=device, output_rate=output_rate, resampler_class=resampler_class,
                         channel_offsets_hz=list(offsets_hz))

    def _create(self, cfg):
        return self._L.fmr_create_channelizer(C.byref(cfg), C.sizeof(Config), C.byref(self.h))

    def resample_blocks_device(self, d_iq_ptr, block_len, d_out_ptr, out_stride, sync=False):
        """The capture (one row) at d_iq_ptr; K rows of out_stride complex samples at d_out_ptr.  Returns out_len."""
        return super().resample_blocks_device(d_iq_ptr, 0, block_len, d_out_ptr, out_stride, sync)


def find_stations(psd, input_rate, raster_hz=100000, raster_offset_hz=0, bandwidth_hz=200000, max_abs_offset_hz=0,
                  threshold_db=10.0, floor_percentile=0.0, cap=None):
    """fmr_find_stations (host only): the stations of a spectrum in fftshift order (Spectrum.psd), as a list of dicts
    {offset_hz, level_db, snr_db, centroid_hz} in ascending offset order.  cap: write at most cap (None: all)."""
    psd = np.ascontiguousarray(psd, dtype=np.float64)
    rule = StationRule(int(raster_hz), int(raster_offset_hz), int(bandwidth_hz), int(max_abs_offset_hz),
                       float(threshold_db), float(floor_percentile))
    L = lib()
    dp = C.POINTER(C.c_double)
    n = L.fmr_find_stations(psd.ctypes.data_as(dp), len(psd), float(input_rate), C.byref(rule), None, 0)
    if n < 0:
        raise FmrError(f"fmr_find_stations failed ({n}): {L.fmr_last_error().decode()}")
    k = n if cap is None else min(n, int(cap))
    out = (Station * max(k, 1))()
    n2 = L.fmr_find_stations(psd.ctypes.data_as(dp), len(psd), float(input_rate), C.byref(rule), out, k)
    assert n2 == n
    return [{"offset_hz": int(st.offset_hz), "level_db": st.level_db, "snr_db": st.snr_db, "centroid_hz": st.centroid_hz}
            for st in out[:k]]


class Spectrum:
    """Welch power spectrum of n_rows IQ rows on the GPU (fmr_spectrum_*): mean PSD and peak hold per row, density-scaled,
    in fftshift order (element k = bin (k - N/2) F / N Hz).  waterfall_segments = R > 0 adds a waterfall (one line per R
    segments, waterfall_lines of them kept per row, read with waterfall()); 0 is the plain object."""

    def __init__(self, input_rate, fft_size=8192, hop=0, window=WINDOW_HANN, n_rows=1, input_format=IQ_CF32,
                 max_call_len=1 << 20, device=0, waterfall_segments=0, waterfall_lines=0, waterfall_which=WATERFALL_MEAN):
        self._L = lib()
        cfg = SpectrumConfig()
        cfg.struct_size = C.sizeof(SpectrumConfig)
        cfg.device, cfg.n_rows, cfg.input_rate, cfg.input_format = int(device), int(n_rows), float(input_rate), int(input_format)
        cfg.fft_size, cfg.hop, cfg.window, cfg.max_call_len = int(fft_size), int(hop), int(window), int(max_call_len)
        self.n_rows, self.fft_size, self.input_rate, self.input_format = int(n_rows), int(fft_size), float(input_rate), int(input_format)
        self.h = C.c_void_p()
        name = "fmr_spectrum_create"
        if waterfall_segments:
            name = "fmr_spectrum_create_waterfall"
            wf = WaterfallConfig(C.sizeof(WaterfallConfig), int(waterfall_segments), int(waterfall_lines), int(waterfall_which))
            rc = self._L.fmr_spectrum_create_waterfall(C.byref(cfg), C.sizeof(SpectrumConfig), C.byref(wf),
                                                       C.sizeof(WaterfallConfig), C.byref(self.h))
        else:
            rc = self._L.fmr_spectrum_create(C.byref(cfg), C.sizeof(SpectrumConfig), C.byref(self.h))
        if rc != OK:
            self.h = None
            raise FmrError(f"{name} failed ({rc}): {self._L.fmr_last_error().decode()}")

    def close(self):
        if getattr(self, "h", None) and getattr(self, "_L", None) is not None:
            self._L.fmr_spectrum_destroy(self.h)
        self.h = None

    def __del__(self):
        self.close()

    def _chk(self, rc):
        if rc < 0:
            raise FmrError(f"fmradion_amd error {rc}: {self._L.fmr_last_error().decode()}")
        return rc

    def process(self, x):
        """x: (n,) or (n_rows, n) complex64 -- or, for a raw input_format, (n, 2) / (n_rows, n, 2) of its integer type."""
        if self.input_format == IQ_CF32:
            x = np.ascontiguousarray(np.atleast_2d(x), dtype=np.complex64)
        else:
            x = np.ascontiguousarray(x, dtype=_IQ_DTYPE[self.input_format])
            if x.ndim == 2:
                x = x[None]
            assert x.ndim == 3 and x.shape[2] == 2
        assert x.shape[0] == self.n_rows, (x.shape, self.n_rows)
        self._chk(self._L.fmr_spectrum_process(self.h, x.ctypes.data, x.shape[1], x.shape[1]))

    def process_device(self, ptr, n, stride=0, sync=True):
        """Rows of `stride` IQ samples (0 = n) at the device address ptr (e.g. a torch tensor's data_ptr())."""
        self._chk(self._L.fmr_spectrum_process_device(self.h, C.c_void_p(int(ptr)), int(stride), int(n), int(sync)))

    def synchronize(self):
        self._chk(self._L.fmr_spectrum_synchronize(self.h))

    def _read(self, row, which):
        out = np.empty(self.fft_size, dtype=np.float64)
        info = SpectrumInfo()
        self._chk(self._L.fmr_spectrum_read(self.h, int(row), which, out.ctypes.data_as(C.POINTER(C.c_double)),
                                            len(out), C.byref(info)))
        return out, info

    def psd(self, row=0):
        return self._read(row, 0)[0]

    def peak_hold(self, row=0):
        return self._read(row, 1)[0]

    def info(self, row=0):
        i = self._read(row, 0)[1]
        return {k: getattr(i, k) for k, _ in SpectrumInfo._fields_}

    def freqs(self):
        return (np.arange(self.fft_size) - self.fft_size // 2) * (self.input_rate / self.fft_size)

    def reset(self):
        self._chk(self._L.fmr_spectrum_reset(self.h))

    def waterfall(self, row=0, cap=None):
        """The oldest unread complete waterfall lines of `row` (at most cap; None: all that are ready): (lines float32
        [n, N] in fftshift order, counted uint32 [n], info dict of fmr_waterfall_info).  Reading drains them."""
        info = WaterfallInfo()
        if cap is None:
            cap = self._chk(self._L.fmr_spectrum_read_waterfall(self.h, int(row), None, None, 0, C.byref(info)))
        lines = np.empty((int(cap), self.fft_size), dtype=np.float32)
        counted = np.empty(int(cap), dtype=np.uint32)
        n = self._chk(self._L.fmr_spectrum_read_waterfall(
            self.h, int(row), lines.ctypes.data_as(C.POINTER(C.c_float)), counted.ctypes.data_as(C.POINTER(C.c_uint32)),
            int(cap), C.byref(info)))
        if int(cap) == 0:
            n = 0
        return lines[:n], counted[:n], {k: getattr(info, k) for k, _ in WaterfallInfo._fields_}
