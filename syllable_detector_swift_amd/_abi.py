"""ctypes declaration of the C ABI in include/syldet.h.

The product path is libsyldet.so (hand-written HIP for gfx950).  There is no Python or
CPU fallback: if the library is missing this module raises at import time.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# SYLDET_LIB: a diagnostic build of the same library (knock-out timing runs); never a different implementation
LIB_PATH = os.environ.get("SYLDET_LIB") or os.path.join(_HERE, "lib", "libsyldet.so")

ABI_VERSION = 1

# status codes (syldet_status_t)
OK = 0
ERR_INVALID_ARGUMENT = -1
ERR_FFT_SIZE = -2
ERR_OVERLAP = -3
ERR_FREQ_RANGE = -4
ERR_INPUT_MISMATCH = -5
ERR_THRESHOLD_MISMATCH = -6
ERR_LAYER_SHAPE = -7
ERR_BUFFER_FULL = -8
ERR_NO_DEVICE = -9
ERR_DEVICE = -10
ERR_OUT_OF_MEMORY = -11
ERR_PARSE_OPEN = -20
ERR_PARSE_MISSING = -21
ERR_PARSE_INVALID = -22
ERR_PARSE_LENGTH = -23
ERR_UNSUPPORTED = -30

WINDOW_NONE, WINDOW_HAMMING, WINDOW_HANNING, WINDOW_BLACKMAN = 0, 1, 2, 3
SCALING_LINEAR, SCALING_LOG, SCALING_DB = 0, 1, 2
SPECTRUM_POWER, SPECTRUM_MAGNITUDE = 0, 1
FN_L2NORMALIZE, FN_NORMALIZE, FN_NORMALIZESTD, FN_MAPMINMAX, FN_MAPSTD = 0, 1, 2, 3, 4
TF_TANSIG, TF_LOGSIG, TF_PURELIN, TF_SATLIN = 0, 1, 2, 3
RULE_FIRST, RULE_ANY = 0, 1
ENGINE_AUTO, ENGINE_GENERIC, ENGINE_FUSED, ENGINE_WIDE_BF16 = 0, 1, 2, 3
PCM_U8, PCM_S16, PCM_S24, PCM_S32, PCM_F32, PCM_F64 = 1, 2, 3, 4, 5, 6     # SYLDET_PCM_*: a file's own sample format

c_float_p = C.POINTER(C.c_float)
c_double_p = C.POINTER(C.c_double)
c_uint8_p = C.POINTER(C.c_uint8)
c_int64_p = C.POINTER(C.c_int64)
c_int32_p = C.POINTER(C.c_int32)
c_int16_p = C.POINTER(C.c_int16)


class Fn(C.Structure):
    _fields_ = [("kind", C.c_int32), ("count", C.c_int32), ("x_offsets", c_float_p),
                ("gains", c_float_p), ("y", C.c_float)]


class Layer(C.Structure):
    _fields_ = [("inputs", C.c_int32), ("outputs", C.c_int32), ("transfer", C.c_int32),
                ("weights", c_float_p), ("biases", c_float_p)]


class Config(C.Structure):
    _fields_ = [("sampling_rate", C.c_double),
                ("fourier_length", C.c_int32), ("window_length", C.c_int32), ("window_overlap", C.c_int32),
                ("freq_lo", C.c_double), ("freq_hi", C.c_double),
                ("time_range", C.c_int32), ("scaling", C.c_int32), ("window", C.c_int32),
                ("spectrum", C.c_int32), ("rule", C.c_int32),
                ("n_input_fns", C.c_int32), ("input_fns", C.POINTER(Fn)),
                ("n_layers", C.c_int32), ("layers", C.POINTER(Layer)),
                ("n_output_fns", C.c_int32), ("output_fns", C.POINTER(Fn)),
                ("n_thresholds", C.c_int32), ("thresholds", c_double_p)]


class Geometry(C.Structure):
    _fields_ = [("gap", C.c_int32), ("overlap", C.c_int32), ("hop", C.c_int32),
                ("f0", C.c_int32), ("f1", C.c_int32), ("bins", C.c_int32),
                ("inputs", C.c_int32), ("outputs", C.c_int32), ("first_index", C.c_int32),
                ("engine", C.c_int32)]


class Slot(C.Structure):
    """syldet_slot_t: where a recording lies in a bank's packed rows."""
    _fields_ = [("row", C.c_int32), ("offset", C.c_int64), ("first_eval", C.c_int64), ("n_evals", C.c_int64),
                ("n_samples", C.c_int64)]


class Shard(C.Structure):
    _fields_ = [("device", C.c_int32), ("first_channel", C.c_int32), ("channels", C.c_int32),
                ("part", C.c_int32), ("parts", C.c_int32)]


EXCHANGE_RCCL, EXCHANGE_PEER_COPY = 0, 1

# columns of a score table row (SYLDET_SCORE_*)
SCORE_DETECTIONS, SCORE_HITS, SCORE_FALSE_POSITIVES, SCORE_REPEATS, SCORE_SUM_OFFSET, SCORE_SUM_OFFSET_SQUARED = 0, 1, 2, 3, 4, 5
SCORE_COLUMNS = 6
SCORE_MAX_THRESHOLDS = 4096
SCORE_MAX_TOLERANCE = 1 << 20

# sources of event-aligned windows (SYLDET_ALIGN_*)
ALIGN_COLUMNS, ALIGN_OUTPUTS, ALIGN_SAMPLES = 0, 1, 2
ALIGN_MAX_WINDOW = 1 << 20
ALIGN_BLOCK = 256

# the trainer's envelope (SYLDET_TRAIN_*)
TRAIN_MAX_HIDDEN, TRAIN_MAX_OUTPUTS = 16, 4

# the matcher's limits (SYLDET_MATCH_*)
MATCH_MAX_TEMPLATE, MATCH_MAX_SEPARATION = 32768, 4096
MATCH_MAX_TEMPLATES, MATCH_MAX_CLASSES = 64, 16

Handle = C.c_void_p
Config_p = C.POINTER(Config)
c_void_pp = C.POINTER(C.c_void_p)

# every symbol include/syldet.h declares: name -> (restype, argtypes)
SIGNATURES = {
    "syldet_abi_version": (C.c_int, []),
    "syldet_strerror": (C.c_char_p, [C.c_int]),
    "syldet_last_error": (C.c_char_p, []),
    "syldet_config_load_text": (C.c_int, [C.c_char_p, C.POINTER(Config_p)]),
    "syldet_config_free": (None, [Config_p]),
    "syldet_config_geometry": (C.c_int, [Config_p, C.POINTER(Geometry)]),
    "syldet_frequency_index_range": (C.c_int, [C.c_int32, C.c_double, C.c_double, C.c_double, c_int32_p, c_int32_p]),
    "syldet_make_window": (C.c_int, [C.c_int32, C.c_int32, c_float_p]),
    "syldet_create": (C.c_int, [Config_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(Handle)]),
    "syldet_create_multi": (C.c_int, [C.POINTER(Config_p), C.c_int32, c_int32_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(Handle)]),
    "syldet_config_compatible": (C.c_int, [Config_p, Config_p, C.POINTER(C.c_char_p)]),
    "syldet_create_mixed": (C.c_int, [C.POINTER(Config_p), C.c_int32, c_int32_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(Handle)]),
    "syldet_config_same_clock": (C.c_int, [Config_p, Config_p, C.POINTER(C.c_char_p)]),
    "syldet_channel_geometry": (C.c_int, [Handle, C.c_int32, C.POINTER(Geometry)]),
    "syldet_destroy": (C.c_int, [Handle]),
    "syldet_get_geometry": (C.c_int, [Handle, C.POINTER(Geometry)]),
    "syldet_channels": (C.c_int32, [Handle]),
    "syldet_count_frames": (C.c_int64, [Handle, C.c_int64]),
    "syldet_count_evals": (C.c_int64, [Handle, C.c_int64]),
    "syldet_run_device": (C.c_int, [Handle, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "syldet_run": (C.c_int, [Handle, c_float_p, C.c_int64, C.c_int64, c_float_p, c_uint8_p]),
    "syldet_run_device_s16": (C.c_int, [Handle, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "syldet_run_s16": (C.c_int, [Handle, c_int16_p, C.c_int64, C.c_int64, c_float_p, c_uint8_p]),
    "syldet_spectrogram_device": (C.c_int, [Handle, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p]),
    "syldet_spectrogram": (C.c_int, [Handle, c_float_p, C.c_int64, C.c_int64, c_float_p]),
    "syldet_detections_device": (C.c_int, [Handle, C.c_void_p, C.c_int64, C.c_double, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "syldet_detections": (C.c_int, [Handle, c_uint8_p, C.c_int64, C.c_double, c_int64_p, C.c_int64, c_int64_p]),
    "syldet_trace_device": (C.c_int, [Handle, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p]),
    "syldet_trace_device_s16": (C.c_int, [Handle, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p]),
    "syldet_trace_interleaved_device_s16": (C.c_int, [Handle, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p]),
    "syldet_trace": (C.c_int, [Handle, c_float_p, C.c_int64, C.c_int32, c_float_p, C.c_int64, C.c_int64]),
    "syldet_trace_s16": (C.c_int, [Handle, c_float_p, C.c_int64, C.c_int32, c_int16_p, C.c_int64, C.c_int64]),
    "syldet_trigger_width": (C.c_int64, [C.c_double, C.c_double]),
    "syldet_trigger_device": (C.c_int, [Handle, C.c_void_p, C.c_int64, C.c_int32, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p]),
    "syldet_trigger_device_s16": (C.c_int, [Handle, C.c_void_p, C.c_int64, C.c_int32, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p]),
    "syldet_trigger_interleaved_device_s16": (C.c_int, [Handle, C.c_void_p, C.c_int64, C.c_int32, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p]),
    "syldet_trigger_mux_device_s16": (C.c_int, [Handle, C.c_void_p, C.c_int64, C.c_int32, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p]),
    "syldet_trigger_onsets_device": (C.c_int, [Handle, C.c_void_p, C.c_int64, C.c_int32, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "syldet_trigger_rehearse_device": (C.c_int, [Handle, C.c_void_p, C.c_int64, C.c_int32, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "syldet_trigger_rehearse_device_s16": (C.c_int, [Handle, C.c_void_p, C.c_int64, C.c_int32, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "syldet_trigger": (C.c_int, [Handle, c_uint8_p, C.c_int64, C.c_int32, C.c_int64, C.c_int64, c_float_p, C.c_int64, C.c_int64]),
    "syldet_trigger_s16": (C.c_int, [Handle, c_uint8_p, C.c_int64, C.c_int32, C.c_int64, C.c_int64, c_int16_p, C.c_int64, C.c_int64]),
    "syldet_trigger_onsets": (C.c_int, [Handle, c_uint8_p, C.c_int64, C.c_int32, C.c_int64, C.c_int64, C.c_int64, c_int64_p, C.c_int64, c_int64_p]),
    "syldet_trigger_arm": (C.c_int, [Handle, C.c_int32, C.c_int64]),
    "syldet_trigger_render": (C.c_int, [Handle, C.c_int32, c_float_p, C.c_int32]),
    "syldet_levels_count": (C.c_int64, [C.c_int64, C.c_int32, C.c_int64]),
    "syldet_sum_squares": (C.c_float, [c_float_p, C.c_int64]),
    "syldet_levels_eval_range": (C.c_int, [Handle, C.c_int64, C.c_int64, C.c_int32, C.c_int64, C.c_int64, c_int64_p, c_int64_p]),
    "syldet_levels_device": (C.c_int, [Handle, C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p]),
    "syldet_levels_device_s16": (C.c_int, [Handle, C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p]),
    "syldet_levels_interleaved_device": (C.c_int, [Handle, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p]),
    "syldet_levels_interleaved_device_s16": (C.c_int, [Handle, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p]),
    "syldet_output_levels_device": (C.c_int, [Handle, C.c_void_p, C.c_int64, C.c_int32, C.c_int64, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p]),
    "syldet_levels": (C.c_int, [Handle, c_float_p, C.c_int64, C.c_int64, C.c_int32, C.c_int64, c_double_p]),
    "syldet_levels_s16": (C.c_int, [Handle, c_int16_p, C.c_int64, C.c_int64, C.c_int32, C.c_int64, c_double_p]),
    "syldet_output_levels": (C.c_int, [Handle, c_float_p, C.c_int64, C.c_int32, C.c_int64, C.c_int32, C.c_int64, c_float_p]),
    "syldet_meters_enable": (C.c_int, [Handle, C.c_int]),
    "syldet_input_level": (C.c_int, [Handle, C.c_int32, c_double_p, c_int32_p]),
    "syldet_output_level": (C.c_int, [Handle, C.c_int32, c_double_p, c_int32_p]),
    "syldet_profile": (C.c_int, [Handle, C.c_int]),
    "syldet_last_timings": (C.c_int, [Handle, c_double_p, C.POINTER(C.c_char_p), C.c_int32, c_int32_p]),
    "syldet_profile_history": (C.c_int, [Handle, C.c_int32]),
    "syldet_timings": (C.c_int, [Handle, C.c_int32, c_double_p, C.POINTER(C.c_char_p), C.c_int32, c_int32_p]),
    "syldet_fixup_stats": (C.c_int, [Handle, c_int64_p, c_int32_p]),
    "syldet_segment_evals": (C.c_int64, [Handle, C.c_int64]),
    "syldet_last_fused_form": (C.c_int, [Handle, c_int32_p, c_int32_p]),
    "syldet_fused_form_of_config": (C.c_int, [C.POINTER(Config_p), C.c_int32, c_int32_p, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_int32,
                                              c_int32_p, c_int32_p]),
    "syldet_fused_dry_run_active": (C.c_int32, []),
    "syldet_append": (C.c_int, [Handle, C.c_int32, c_float_p, C.c_int64]),
    "syldet_append_interleaved": (C.c_int, [Handle, c_float_p, C.c_int64, C.c_int32]),
    "syldet_append_interleaved_channels": (C.c_int, [Handle, c_float_p, C.c_int64, C.c_int32, C.POINTER(C.c_int32)]),
    "syldet_append_s16": (C.c_int, [Handle, C.c_int32, c_int16_p, C.c_int64]),
    "syldet_append_interleaved_s16": (C.c_int, [Handle, c_int16_p, C.c_int64, C.c_int32]),
    "syldet_process_new_value": (C.c_int, [Handle, C.c_int32]),
    "syldet_process_all": (C.c_int, [Handle, c_int64_p]),
    "syldet_pending_evaluations": (C.c_int64, [Handle, C.c_int32]),
    "syldet_last_outputs": (C.c_int, [Handle, C.c_int32, c_float_p]),
    "syldet_last_detected": (C.c_int, [Handle, C.c_int32]),
    "syldet_seen_syllable": (C.c_int, [Handle, C.c_int32]),
    "syldet_deinterleave_device_s16": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p]),
    "syldet_deinterleave_device": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p]),
    "syldet_run_interleaved_device": (C.c_int, [Handle, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "syldet_run_interleaved": (C.c_int, [Handle, c_float_p, C.c_int64, C.c_int32, c_float_p, c_uint8_p]),
    "syldet_run_interleaved_device_s16": (C.c_int, [Handle, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "syldet_run_interleaved_s16": (C.c_int, [Handle, c_int16_p, C.c_int64, C.c_int32, c_float_p, c_uint8_p]),
    "syldet_pack_flags_device": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p]),
    "syldet_unpack_flags_device": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p]),
    "syldet_resampler_create": (C.c_int, [C.c_double, C.c_double, C.c_int32, C.c_int32, C.POINTER(Handle)]),
    "syldet_resampler_destroy": (C.c_int, [Handle]),
    "syldet_resampler_count": (C.c_int64, [Handle, C.c_int64]),
    "syldet_resample_device": (C.c_int, [Handle, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, c_int64_p, C.c_void_p]),
    "syldet_convert_rate_count": (C.c_int64, [C.c_int64, C.c_double, C.c_double]),
    "syldet_convert_rate_device": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_double, C.c_double, C.c_void_p, C.c_int64, c_int64_p, C.c_void_p]),
    "syldet_sinc_defaults": (None, [c_int32_p, c_double_p, c_double_p]),
    "syldet_sinc_coefficient": (C.c_double, [C.c_double, C.c_double, C.c_double, C.c_int32, C.c_double, C.c_double]),
    "syldet_sinc_taps": (C.c_int64, [C.c_double, C.c_double, C.c_int32, C.c_double]),
    "syldet_convert_rate_sinc_device": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_double, C.c_double, C.c_int32, C.c_double, C.c_double,
                                                  C.c_void_p, C.c_int64, c_int64_p, C.c_void_p]),
    "syldet_convert_rate_sinc_device_s16": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_double, C.c_double, C.c_int32, C.c_double, C.c_double,
                                                      C.c_void_p, C.c_int64, c_int64_p, C.c_void_p]),
    "syldet_sinc_ready": (C.c_int64, [C.c_int64, C.c_double, C.c_double, C.c_int32, C.c_double]),
    "syldet_sinc_resampler_create": (C.c_int, [C.c_double, C.c_double, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_double, C.POINTER(Handle)]),
    "syldet_sinc_resampler_destroy": (C.c_int, [Handle]),
    "syldet_sinc_resampler_reset": (C.c_int, [Handle]),
    "syldet_sinc_resampler_position": (C.c_int, [Handle, c_int64_p, c_int64_p, c_int32_p]),
    "syldet_sinc_resampler_count": (C.c_int64, [Handle, C.c_int64]),
    "syldet_sinc_resampler_flush_count": (C.c_int64, [Handle]),
    "syldet_sinc_resample_device": (C.c_int, [Handle, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, c_int64_p, C.c_void_p]),
    "syldet_sinc_resample_device_s16": (C.c_int, [Handle, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, c_int64_p, C.c_void_p]),
    "syldet_sinc_resampler_flush_device": (C.c_int, [Handle, C.c_void_p, C.c_int64, c_int64_p, C.c_void_p]),
    "syldet_sinc_resample": (C.c_int, [Handle, c_float_p, C.c_int64, C.c_int64, c_float_p, C.c_int64, c_int64_p]),
    "syldet_sinc_resampler_flush": (C.c_int, [Handle, c_float_p, C.c_int64, c_int64_p]),
    "syldet_resample": (C.c_int, [Handle, c_float_p, C.c_int64, C.c_int64, c_float_p, C.c_int64, c_int64_p]),
    "syldet_host_alloc": (C.c_int, [C.c_size_t, c_void_pp]),
    "syldet_host_free": (C.c_int, [C.c_void_p]),
    "syldet_shard_table": (C.c_int, [C.c_int32, C.c_int32, C.POINTER(Shard)]),
    "syldet_shard_evaluations": (C.c_int, [C.c_int64, C.c_int32, C.c_int32, c_int64_p, c_int64_p]),
    "syldet_shard_samples": (C.c_int, [Config_p, C.c_int64, C.c_int64, c_int64_p, c_int64_p]),
    "syldet_create_sharded": (C.c_int, [Config_p, C.c_int32, c_int32_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(Handle)]),
    "syldet_sharded_destroy": (C.c_int, [Handle]),
    "syldet_sharded_channels": (C.c_int32, [Handle]),
    "syldet_sharded_shards": (C.c_int32, [Handle]),
    "syldet_sharded_shard": (C.c_int, [Handle, C.c_int32, C.POINTER(Shard)]),
    "syldet_sharded_bank": (Handle, [Handle, C.c_int32]),
    "syldet_sharded_stream": (C.c_void_p, [Handle, C.c_int32]),
    "syldet_sharded_exchange_stream": (C.c_void_p, [Handle, C.c_int32]),
    "syldet_sharded_ranges": (C.c_int, [Handle, C.c_int32, C.c_int64, c_int64_p, c_int64_p, c_int64_p, c_int64_p]),
    "syldet_sharded_run": (C.c_int, [Handle, c_float_p, C.c_int64, C.c_int64, c_float_p, c_uint8_p]),
    "syldet_sharded_run_device": (C.c_int, [Handle, c_void_pp, C.c_int64, c_int64_p, c_void_pp, c_void_pp, c_void_pp]),
    "syldet_sharded_synchronize": (C.c_int, [Handle]),
    "syldet_sharded_rccl_ranks": (C.c_int32, [Handle]),
    "syldet_sharded_connect": (C.c_int, [Handle]),
    "syldet_sharded_launcher_threads": (C.c_int32, [Handle]),
    "syldet_recordings_plan": (C.c_int, [Handle, c_int64_p, c_int32_p, C.c_int32, C.POINTER(Slot), c_int64_p, c_int64_p, c_double_p]),
    "syldet_recordings_plan_of_config": (C.c_int, [Config_p, C.c_int32, c_int32_p, c_int64_p, c_int32_p, C.c_int32, C.POINTER(Slot), c_int64_p, c_int64_p,
                                                   c_double_p]),
    "syldet_recordings_create": (C.c_int, [Handle, c_int64_p, c_int32_p, C.c_int32, C.POINTER(Handle)]),
    "syldet_recordings_destroy": (C.c_int, [Handle]),
    "syldet_recordings_slots": (C.c_int, [Handle, C.POINTER(Slot)]),
    "syldet_recordings_shape": (C.c_int, [Handle, c_int32_p, c_int64_p, c_int64_p, c_double_p]),
    "syldet_recordings_load_device": (C.c_int, [Handle, C.c_void_p, c_int64_p, c_int32_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "syldet_recordings_load_device_s16": (C.c_int, [Handle, C.c_void_p, c_int64_p, c_int32_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "syldet_recordings_load_sinc_device": (C.c_int, [Handle, C.c_void_p, c_int64_p, c_int32_p, c_int64_p, c_double_p, C.c_int32, C.c_double, C.c_double,
                                                     C.c_void_p, C.c_int64, C.c_void_p]),
    "syldet_recordings_load_sinc_device_s16": (C.c_int, [Handle, C.c_void_p, c_int64_p, c_int32_p, c_int64_p, c_double_p, C.c_int32, C.c_double,
                                                         C.c_double, C.c_void_p, C.c_int64, C.c_void_p]),
    "syldet_pcm_sample_bytes": (C.c_int32, [C.c_int32]),
    "syldet_pcm_decode": (C.c_int, [C.c_int32, C.c_void_p, C.c_int64, C.c_int64, c_float_p]),
    "syldet_pcm_check_sources": (C.c_int, [C.c_void_p, C.c_int64, c_int64_p, c_int32_p, c_int32_p, c_int64_p, C.c_int32]),
    "syldet_recordings_load_pcm_device": (C.c_int, [Handle, C.c_void_p, C.c_int64, c_int64_p, c_int32_p, c_int32_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "syldet_recordings_load_sinc_pcm_device": (C.c_int, [Handle, C.c_void_p, C.c_int64, c_int64_p, c_int32_p, c_int32_p, c_int64_p, c_double_p, C.c_int32,
                                                         C.c_double, C.c_double, C.c_void_p, C.c_int64, C.c_void_p]),
    "syldet_recordings_events_device": (C.c_int, [Handle, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                                  C.c_void_p]),
    "syldet_recordings_trace_device": (C.c_int, [Handle, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, c_int64_p, c_int32_p, C.c_void_p]),
    "syldet_recordings_trace_device_s16": (C.c_int, [Handle, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, c_int64_p, c_int32_p, C.c_void_p]),
    "syldet_recordings_trigger_device": (C.c_int, [Handle, C.c_void_p, C.c_int32, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, c_int64_p, c_int32_p,
                                                   C.c_void_p]),
    "syldet_recordings_trigger_device_s16": (C.c_int, [Handle, C.c_void_p, C.c_int32, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, c_int64_p,
                                                       c_int32_p, C.c_void_p]),
    "syldet_recordings_trigger_onsets_device": (C.c_int, [Handle, C.c_void_p, C.c_int32, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p,
                                                          C.c_void_p]),
    "syldet_recordings_levels_layout": (C.c_int, [Handle, C.c_int32, C.c_int64, c_int64_p, c_int64_p]),
    "syldet_recordings_levels_device": (C.c_int, [Handle, C.c_void_p, C.c_int64, C.c_int32, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p]),
    "syldet_recordings_levels_device_s16": (C.c_int, [Handle, C.c_void_p, C.c_int64, C.c_int32, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p]),
    "syldet_recordings_output_levels_device": (C.c_int, [Handle, C.c_void_p, C.c_int32, C.c_int32, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p]),
    "syldet_scorer_create": (C.c_int, [Handle, Handle, c_double_p, C.c_int32, c_int64_p, c_int64_p, C.c_int64, C.c_double, C.POINTER(Handle)]),
    "syldet_scorer_destroy": (C.c_int, [Handle]),
    "syldet_scorer_shape": (C.c_int, [Handle, c_int32_p, c_int32_p, c_int64_p]),
    "syldet_score_device": (C.c_int, [Handle, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p]),
    "syldet_score_host": (C.c_int, [c_float_p, C.c_int64, C.c_int64, c_double_p, C.c_int32, c_int64_p, C.c_int64, C.c_int64, C.c_int64, C.c_int64,
                                    C.c_int64, c_int64_p]),
    "syldet_score_choose": (C.c_int, [c_int64_p, C.c_int32, C.c_int32, c_int64_p, C.c_double, c_int32_p, c_int64_p, c_double_p]),
    "syldet_aligner_create": (C.c_int, [Handle, Handle, C.c_int32, C.c_int64, C.c_int64, C.POINTER(Handle)]),
    "syldet_aligner_destroy": (C.c_int, [Handle]),
    "syldet_aligner_shape": (C.c_int, [Handle, c_int32_p, c_int64_p, c_int32_p]),
    "syldet_align_anchor": (C.c_int, [Handle, C.c_int32, c_int64_p, c_int64_p, c_int32_p]),
    "syldet_align_device": (C.c_int, [Handle, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, c_int64_p, C.c_float, C.c_void_p, C.c_void_p]),
    "syldet_align_stats_device": (C.c_int, [Handle, C.c_void_p, c_int64_p, c_int32_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "syldet_align_host": (C.c_int, [c_float_p, C.c_int64, C.c_int32, C.c_int64, C.c_int64, C.c_int64, C.c_int64, c_int64_p, C.c_int64, C.c_float,
                                    c_float_p, c_int64_p]),
    "syldet_align_stats_host": (C.c_int, [c_float_p, c_int64_p, C.c_int64, C.c_int64, c_int64_p, c_double_p, c_double_p]),
    "syldet_trainer_create": (C.c_int, [Handle, Handle, C.POINTER(Handle)]),
    "syldet_trainer_destroy": (C.c_int, [Handle]),
    "syldet_trainer_shape": (C.c_int, [Handle, c_int32_p, c_int64_p, c_int32_p, c_int32_p]),
    "syldet_train_param_count": (C.c_int, [Config_p, c_int64_p]),
    "syldet_train_targets_device": (C.c_int, [Handle, c_int64_p, c_int64_p, c_int32_p, C.c_int64, C.c_float, C.c_float, C.c_int64, C.c_void_p, C.c_void_p,
                                              C.c_void_p]),
    "syldet_train_targets_host": (C.c_int, [c_int64_p, C.c_int64, c_int32_p, C.c_int32, C.c_int64, C.c_float, C.c_float, C.c_int64, C.c_int64, C.c_int64,
                                            c_float_p, c_float_p]),
    "syldet_train_gradient_device": (C.c_int, [Handle, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                               C.c_void_p, C.c_void_p]),
    "syldet_train_input_range_device": (C.c_int, [Handle, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "syldet_train_input_map_host": (C.c_int, [c_float_p, C.c_int32, c_float_p, c_float_p]),
    "syldet_trainer_set_input_map": (C.c_int, [Handle, c_float_p, c_float_p, C.c_float]),
    "syldet_trainer_input_map": (C.c_int, [Handle, c_int32_p, c_float_p, c_float_p, c_float_p]),
    "syldet_train_adam_device": (C.c_int, [Handle, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_double, C.c_double, C.c_double, C.c_double, C.c_void_p,
                                           C.c_void_p]),
    "syldet_train_adam_host": (C.c_int, [c_float_p, c_float_p, c_float_p, c_float_p, C.c_int64, c_double_p, C.c_int64, C.c_double, C.c_double, C.c_double,
                                         C.c_double, c_double_p]),
    "syldet_train_fit_device": (C.c_int, [Handle, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_double,
                                          C.c_double, C.c_double, C.c_double, C.c_void_p, C.c_void_p]),
    "syldet_train_init_host": (C.c_int, [C.c_uint64, C.c_int32, C.c_int32, C.c_int32, c_float_p]),
    "syldet_train_config_with": (C.c_int, [Config_p, c_float_p, C.c_int64, c_float_p, c_float_p, C.c_float, C.POINTER(Config_p)]),
    "syldet_config_save_text": (C.c_int, [Config_p, C.c_char_p]),
    "syldet_trainer_create_multi": (C.c_int, [Handle, Handle, C.POINTER(Handle)]),
    "syldet_trainer_networks": (C.c_int, [Handle, c_int32_p, c_int32_p]),
    "syldet_trainer_groups": (C.c_int, [Handle, C.c_int64, c_int32_p]),
    "syldet_trainer_set_input_map_of": (C.c_int, [Handle, C.c_int32, c_float_p, c_float_p, C.c_float]),
    "syldet_trainer_input_map_of": (C.c_int, [Handle, C.c_int32, c_int32_p, c_float_p, c_float_p, c_float_p]),
    "syldet_matcher_create": (C.c_int, [Handle, Handle, c_float_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(Handle)]),
    "syldet_matcher_destroy": (C.c_int, [Handle]),
    "syldet_matcher_shape": (C.c_int, [Handle, c_int32_p, c_int32_p, c_int32_p, c_int32_p, c_int32_p]),
    "syldet_matcher_template": (C.c_int, [Handle, c_float_p]),
    "syldet_match_scores_device": (C.c_int, [Handle, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p]),
    "syldet_match_peaks_device": (C.c_int, [Handle, C.c_void_p, C.c_int64, C.c_float, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                            C.c_void_p]),
    "syldet_match_normalize_host": (C.c_int, [c_float_p, C.c_int32, C.c_int32, c_float_p]),
    "syldet_match_scores_host": (C.c_int, [c_float_p, C.c_int32, C.c_int32, c_float_p, C.c_int64, c_float_p]),
    "syldet_match_peaks_host": (C.c_int, [c_float_p, C.c_int64, C.c_float, C.c_int32, C.c_int64, C.c_int64, C.c_int32, c_int64_p, C.c_int64,
                                          c_int64_p, c_float_p]),
    "syldet_matcher_bank_create": (C.c_int, [Handle, Handle, c_float_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, c_int32_p, C.c_int32,
                                             C.POINTER(Handle)]),
    "syldet_matcher_bank_destroy": (C.c_int, [Handle]),
    "syldet_matcher_bank_shape": (C.c_int, [Handle, c_int32_p, c_int32_p, c_int32_p, c_int32_p, c_int32_p, c_int32_p, c_int32_p]),
    "syldet_matcher_bank_templates": (C.c_int, [Handle, c_float_p, c_int32_p]),
    "syldet_match_bank_scores_device": (C.c_int, [Handle, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "syldet_match_bank_peaks_device": (C.c_int, [Handle, C.c_void_p, C.c_void_p, C.c_int64, c_float_p, C.c_int32, C.c_void_p, C.c_int64,
                                                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "syldet_match_classes_host": (C.c_int, [c_float_p, C.c_int64, C.c_int32, c_int32_p, C.c_int32, c_float_p, c_int32_p]),
    "syldet_matcher_bank_create_ragged": (C.c_int, [Handle, Handle, c_float_p, C.c_int32, c_int32_p, C.c_int32, c_int32_p, c_int32_p, C.c_int32,
                                                    C.POINTER(Handle)]),
    "syldet_matcher_bank_lengths": (C.c_int, [Handle, c_int32_p, c_int32_p, c_int32_p]),
    "syldet_match_bank_peaks_each_device": (C.c_int, [Handle, C.c_void_p, C.c_void_p, C.c_int64, c_float_p, c_int32_p, C.c_void_p, C.c_int64,
                                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
}


def _share_hip_runtime_with_torch() -> None:
    """The torch wheel carries its own libamdhip64.so (SONAME libamdhip64.so.7) and asks for it by
    file name.  If libsyldet pulled /opt/rocm's copy in first, a later `import torch` would load a
    second HIP runtime into the process and one of the two would see no device.  Loading torch's
    copy by path first makes both sides resolve to the same runtime, whatever the import order."""
    import importlib.util
    import sys
    if "torch" in sys.modules:
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.origin:
        return
    rt = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
    if os.path.exists(rt):
        C.CDLL(rt, mode=C.RTLD_GLOBAL)


def load(path: str = LIB_PATH) -> C.CDLL:
    _share_hip_runtime_with_torch()
    if not os.path.exists(path):
        raise ImportError(
            f"{path} not found: libsyldet (the HIP/gfx950 engine) has not been built. "
            "Run `python -c 'import __graft_entry__ as g; g.build()'` at the repository root. "
            "There is no CPU fallback.")
    lib = C.CDLL(path)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError if the library lacks a declared symbol
        fn.restype = res
        fn.argtypes = args
    if lib.syldet_abi_version() != ABI_VERSION:
        raise ImportError(f"libsyldet ABI {lib.syldet_abi_version()} != expected {ABI_VERSION}")
    return lib


lib = load()


def last_error() -> str:
    return (lib.syldet_last_error() or b"").decode("utf-8", "replace")


def strerror(status: int) -> str:
    return (lib.syldet_strerror(status) or b"").decode("utf-8", "replace")
