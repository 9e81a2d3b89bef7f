"""ctypes binding of libfmdemod_mi355x.so (see include/fmdemod_mi355x.h)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = os.environ.get("FMD_LIB_PATH") or os.path.join(_HERE, "libfmdemod_mi355x.so")   # override: kernel experiments

MATH_EXACT = 0
MATH_FAST = 1          # the fastest +-1 LSB family of this build for the configuration
MATH_FAST_VALU = 2     # +-1 LSB, vector ALU only
MATH_FAST_MFMA = 3     # +-1 LSB, /8 decimator on the matrix pipe
MATH_FAST_MFMA_F = 7   # ... and every other stage that has a matrix form: 90-tap stereo (pilot / L-R filters at full rate, the composite L+R filter and the second
                       # stage at the emit instants), 128-tap mono (stage D at the emit instants); what MATH_FAST resolves to where it applies
MATH_FAST_MFMA_C, MATH_FAST_MFMA_D, MATH_FAST_MFMA_E = 4, 5, 6   # retired in round 6: accepted, mean MATH_FAST
FAST_MATHS = (MATH_FAST_VALU, MATH_FAST_MFMA, MATH_FAST_MFMA_F)
WINDOW_RECT = 0        # capture spectrum (fmd_batch_spectrum_*): w = 1
WINDOW_HANN = 1        # ... w[n] = 0.5 - 0.5 cos(2 pi n / N)
MAXIMUM_BUF_LENGTH = 16 * 16384


class FmdError(RuntimeError):
    pass


def library_path():
    return _LIB


def build_library(force=False):
    """Compile the HIP kernels and the C host layer for gfx950 (hipcc + gcc)."""
    csrc = os.path.join(_HERE, "csrc")
    cmd = ["make", "-C", csrc]
    if force:
        cmd.append("-B")
    subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL)
    return _LIB


class FmdConfig(C.Structure):
    _fields_ = [
        ("rate_in", C.c_int32), ("rate_out", C.c_int32), ("rate_out2", C.c_int32),
        ("mode", C.c_int32), ("size", C.c_int32), ("deemph", C.c_int32),
        ("offset_tuning", C.c_int32), ("deemph_lambda", C.c_float), ("volume", C.c_float),
        ("block_len", C.c_int32), ("math", C.c_int32),
    ]


class FmdTaps(C.Structure):
    _fields_ = [("fb", C.c_float * 16), ("fm", C.c_float * 128), ("fp", C.c_float * 128),
                ("fs", C.c_float * 128), ("swf", C.c_float), ("cwf", C.c_float)]


class _FmdFilterError(C.Structure):
    _fields_ = [("taps", C.c_int32), ("qf", C.c_int32), ("rms_lsb", C.c_float), ("worst_lsb", C.c_float),
                ("worst_samples_lsb", C.c_float), ("worst_taps_lsb", C.c_float), ("worst_dropped_lsb", C.c_float)]


class FmdErrorEstimate(C.Structure):
    _fields_ = [("family", C.c_int32), ("filters", C.c_int32), ("f", _FmdFilterError * 2), ("limit_rms_lsb", C.c_float)]


class FmdStreamState(C.Structure):
    _fields_ = [("tb", C.c_float * 48), ("pre_r", C.c_float), ("pre_j", C.c_float), ("pp", C.c_float),
                ("deemph_l", C.c_float), ("deemph_r", C.c_float), ("acc", C.c_int32),
                ("reserved", C.c_int32 * 2), ("br", C.c_float * 256), ("bm", C.c_float * 256),
                ("bs", C.c_float * 256)]


class FmdSubcConfig(C.Structure):        # fmd_subc_config
    _fields_ = [("rate_in", C.c_int32), ("fc", C.c_int32), ("bw", C.c_int32), ("n_taps", C.c_int32), ("decim", C.c_int32),
                ("block_samples", C.c_int32)]


class FmdSubcState(C.Structure):         # fmd_subc_state
    _fields_ = [("phase", C.c_int32), ("reserved", C.c_int32 * 3), ("hist", C.c_float * 256)]


class FmdTunerConfig(C.Structure):       # fmd_tuner_config
    _fields_ = [("rate", C.c_int32), ("step_hz", C.c_int32), ("bw", C.c_int32), ("n_taps", C.c_int32), ("block_len", C.c_int32), ("reserved", C.c_int32)]


class FmdTunerChannel(C.Structure):      # fmd_tuner_channel
    _fields_ = [("source", C.c_int32), ("shift", C.c_int32), ("gain", C.c_float), ("reserved", C.c_int32)]


class FmdTunerState(C.Structure):        # fmd_tuner_state
    _fields_ = [("count", C.c_int32), ("valid", C.c_int32), ("reserved", C.c_int32 * 2), ("hist", C.c_uint8 * 128)]


class FmdScanConfig(C.Structure):        # fmd_scan_config
    _fields_ = [("rate", C.c_int32), ("n_bins", C.c_int32), ("raster_hz", C.c_int32), ("bw", C.c_int32), ("min_sep", C.c_int32),
                ("floor_permille", C.c_int32), ("dc_guard", C.c_int32), ("max_stations", C.c_int32), ("threshold", C.c_float), ("reserved", C.c_int32 * 3)]


class FmdScanStation(C.Structure):       # fmd_scan_station
    _fields_ = [("offset_hz", C.c_int32), ("candidate", C.c_int32), ("power", C.c_float), ("snr", C.c_float), ("centroid_hz", C.c_float),
                ("reserved", C.c_int32 * 3)]


STEREO_AUTO, STEREO_FORCE_MONO, STEREO_FORCE_STEREO = 0, 1, 2     # fmd_stereo_set_mode


class FmdStereoConfig(C.Structure):      # fmd_stereo_config
    _fields_ = [("pcm_stride", C.c_int32), ("pilot_per_block", C.c_int32), ("hold_blocks", C.c_int32), ("reserved0", C.c_int32),
                ("pilot_on", C.c_float), ("pilot_off", C.c_float), ("blend_lo", C.c_float), ("blend_hi", C.c_float), ("slew", C.c_float),
                ("reserved", C.c_int32 * 3)]


class FmdStereoState(C.Structure):       # fmd_stereo_state
    _fields_ = [("g", C.c_float), ("stereo", C.c_int32), ("run", C.c_int32), ("reserved", C.c_int32)]


class FmdRdsConfig(C.Structure):         # fmd_rds_config
    _fields_ = [("rate_z", C.c_int32), ("block_z", C.c_int32), ("n_taps", C.c_int32), ("avg_blocks", C.c_int32), ("max_blocks", C.c_int32)]


class FmdRdsState(C.Structure):          # fmd_rds_state
    _fields_ = [("phase", C.c_int32), ("frac", C.c_int32), ("bit", C.c_int64), ("ts", C.c_float * 2), ("reserved", C.c_int32 * 2),
                ("zhist", C.c_float * 128), ("yhist", C.c_float * 136)]


class FmdRdsGroup(C.Structure):          # fmd_rds_group
    _fields_ = [("blk", C.c_uint16 * 4), ("ok_mask", C.c_uint8), ("version", C.c_uint8)]


class FmdRdsDecoder(C.Structure):        # fmd_rds_decoder
    _fields_ = [("reg", C.c_uint32), ("fill", C.c_int32), ("synced", C.c_int32), ("pos", C.c_int32), ("cnt", C.c_int32), ("bad_run", C.c_int32),
                ("hidx", C.c_int32), ("hpos", C.c_int8 * 26), ("ok_mask", C.c_uint8), ("reserved", C.c_uint8), ("hword", C.c_uint16 * 26),
                ("blk", C.c_uint16 * 4), ("consumed", C.c_int32), ("n_sync", C.c_uint32), ("n_loss", C.c_uint32), ("bits", C.c_uint64)]


class FmdRdsInfo(C.Structure):           # fmd_rds_info
    _fields_ = [("have_pi", C.c_int32), ("pi", C.c_uint16), ("pty", C.c_uint8), ("ps_mask", C.c_uint8), ("ps", C.c_uint8 * 9), ("reserved", C.c_uint8 * 3)]


class FmdDebugTaps(C.Structure):
    _fields_ = [("y", C.c_void_p), ("v", C.c_void_p), ("mpx", C.c_void_p), ("prof", C.c_void_p)]


class LpReal(C.Structure):          # struct lp_real
    _fields_ = [("br", C.POINTER(C.c_float)), ("bm", C.POINTER(C.c_float)), ("bs", C.POINTER(C.c_float)),
                ("fm", C.POINTER(C.c_float)), ("fp", C.POINTER(C.c_float)), ("fs", C.POINTER(C.c_float)),
                ("swf", C.c_float), ("cwf", C.c_float), ("pp", C.c_float), ("pos", C.c_int),
                ("size", C.c_int), ("rsize", C.c_int), ("mode", C.c_int)]


class DemodState(C.Structure):      # struct demod_state (x86-64 glibc layout)
    _fields_ = [
        ("exit_flag", C.c_int), ("thread", C.c_ulong),
        ("buf", C.c_uint8 * MAXIMUM_BUF_LENGTH), ("buf_len", C.c_uint32),
        ("lowpassed", C.c_int16 * (MAXIMUM_BUF_LENGTH << 1)), ("lp_len", C.c_int),
        ("lowpass_tb", C.c_float * 48), ("lp_i_hist", C.c_int16 * 60), ("lp_q_hist", C.c_int16 * 60),
        ("result", C.c_int16 * MAXIMUM_BUF_LENGTH), ("result_len", C.c_int),
        ("droop_i_hist", C.c_int16 * 9), ("droop_q_hist", C.c_int16 * 9),
        ("offset_tuning", C.c_int), ("rate_in", C.c_int), ("rate_out", C.c_int), ("rate_out2", C.c_int),
        ("now_r", C.c_int), ("now_j", C.c_int), ("pre_r", C.c_int), ("pre_j", C.c_int),
        ("pre_r_f32", C.c_float), ("pre_j_f32", C.c_float), ("prev_index", C.c_int),
        ("downsample", C.c_int), ("post_downsample", C.c_int), ("output_scale", C.c_int),
        ("squelch_level", C.c_int), ("conseq_squelch", C.c_int), ("squelch_hits", C.c_int),
        ("terminate_on_squelch", C.c_int), ("downsample_passes", C.c_int), ("comp_fir_size", C.c_int),
        ("custom_atan", C.c_int), ("deemph", C.c_double), ("deemph_a", C.c_int), ("deemph_l", C.c_int),
        ("deemph_r", C.c_int), ("deemph_l_f32", C.c_float), ("deemph_r_f32", C.c_float),
        ("deemph_lambda", C.c_float), ("volume", C.c_float), ("now_lpr", C.c_int),
        ("prev_lpr_index", C.c_int), ("lpr", LpReal),
        ("rw", C.c_uint8 * 56), ("ready", C.c_uint8 * 48), ("ready_m", C.c_uint8 * 40),
        ("output_target", C.c_void_p),
    ]


_lib = None

_EXPORTS = [
    "init_u8_f32_table", "init_lp_f32", "init_lp_real_f32", "deinit_lp_real_f32", "demod_init",
    "rotate_90_u8_f32", "u8_f32", "full_demod", "fmd_demod_release", "fmd_dropin_set_math", "fmd_dropin_set_error_handler",
    "fmd_config_error_estimate", "fmd_design_taps", "fmd_deemph_lambda", "fmd_batch_create", "fmd_batch_destroy",
    "fmd_batch_pcm_stride", "fmd_batch_n_streams", "fmd_batch_math", "fmd_config_family", "fmd_batch_set_time_split", "fmd_batch_run_device", "fmd_batch_run_device_debug",
    "fmd_batch_sync", "fmd_batch_wait_stream", "fmd_batch_run_host", "fmd_batch_get_state", "fmd_batch_set_state",
    "fmd_batch_reset", "fmd_batch_last_kernel_ms", "fmd_batch_set_timing", "fmd_batch_kernel_name", "fmd_last_error",
    "fmd_device_count", "fmd_ingest_create", "fmd_ingest_destroy", "fmd_ingest_callback",
    "fmd_ingest_buffered", "fmd_ingest_dropped", "fmd_ingest_mute", "fmd_ingest_set_overflow", "fmd_ingest_pop",
    "fmd_batch_pump",
    "fmd_batch_pump_begin", "fmd_batch_pump_end",
    "fmd_batch_run_device_levels", "fmd_batch_run_host_levels", "fmd_batch_set_squelch", "fmd_batch_get_squelch_hits",
    "fmd_batch_set_squelch_hits",
    "fmd_batch_spectrum_device", "fmd_batch_spectrum_host",
    "fmd_subc_design", "fmd_subc_create", "fmd_batch_subc_create", "fmd_subc_destroy", "fmd_subc_out_per_block", "fmd_subc_run_device",
    "fmd_subc_run_host", "fmd_subc_get_state", "fmd_subc_set_state", "fmd_subc_reset", "fmd_subc_sync",
    "fmd_rds_design", "fmd_rds_create", "fmd_subc_rds_create", "fmd_rds_destroy", "fmd_rds_bits_per_block", "fmd_rds_run_device", "fmd_rds_run_host",
    "fmd_rds_last_y", "fmd_rds_get_state", "fmd_rds_set_state", "fmd_rds_reset", "fmd_rds_sync",
    "fmd_tuner_design", "fmd_tuner_shift", "fmd_tuner_create", "fmd_batch_tuner_create", "fmd_tuner_destroy", "fmd_tuner_set_channel",
    "fmd_tuner_get_channel", "fmd_tuner_run_device", "fmd_tuner_run_host", "fmd_tuner_get_state", "fmd_tuner_set_state", "fmd_tuner_reset",
    "fmd_tuner_sync",
    "fmd_scan_candidates", "fmd_scan_create", "fmd_batch_scan_create", "fmd_scan_destroy", "fmd_scan_run_device", "fmd_scan_run_host", "fmd_scan_sync",
    "fmd_stereo_create", "fmd_batch_stereo_create", "fmd_stereo_destroy", "fmd_stereo_set_mode", "fmd_stereo_run_device", "fmd_stereo_run_host",
    "fmd_stereo_get_state", "fmd_stereo_set_state", "fmd_stereo_reset", "fmd_stereo_sync",
    "fmd_rds_decoder_init", "fmd_rds_decoder_push", "fmd_rds_info_init", "fmd_rds_info_update",
    "fmd_wav_header", "fmd_wav_open", "fmd_wav_write", "fmd_wav_close",
]

INGEST_CB = C.CFUNCTYPE(None, C.POINTER(C.c_ubyte), C.c_uint32, C.c_void_p)
DROPIN_ERROR_CB = C.CFUNCTYPE(None, C.c_char_p, C.c_char_p, C.c_void_p)     # fmd_dropin_error_fn


def exported_symbols():
    return list(_EXPORTS)


def lib():
    """Load libfmdemod_mi355x.so; raises FmdError when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_LIB):
        raise FmdError("%s is missing: run __graft_entry__.build() (there is no CPU fallback)" % _LIB)
    # torch bundles its own libamdhip64.so.7; two HIP runtimes in one process break the
    # second one, so when torch is installed let it load first and share its copy.
    if "torch" not in sys.modules:
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
    L = C.CDLL(_LIB)
    vp = C.c_void_p
    L.fmd_design_taps.argtypes = [C.POINTER(FmdConfig), C.POINTER(FmdTaps)]
    L.fmd_deemph_lambda.restype = C.c_float
    L.fmd_deemph_lambda.argtypes = [C.c_int, C.c_double]
    L.fmd_batch_create.argtypes = [C.POINTER(vp), C.POINTER(FmdConfig), C.POINTER(FmdTaps), C.c_int, C.c_int]
    L.fmd_batch_destroy.argtypes = [vp]
    L.fmd_batch_destroy.restype = None
    L.fmd_batch_pcm_stride.argtypes = [vp]
    L.fmd_batch_n_streams.argtypes = [vp]
    L.fmd_batch_math.argtypes = [vp]
    L.fmd_config_family.argtypes = [C.POINTER(FmdConfig), vp]
    L.fmd_batch_set_time_split.argtypes = [vp, C.c_int]
    L.fmd_batch_run_device.argtypes = [vp, vp, C.c_int, vp, vp, vp]
    L.fmd_batch_run_device_debug.argtypes = [vp, vp, C.c_int, vp, vp, vp, C.POINTER(FmdDebugTaps)]
    L.fmd_batch_sync.argtypes = [vp]
    L.fmd_batch_run_host.argtypes = [vp, vp, C.c_int, vp, vp]
    L.fmd_batch_get_state.argtypes = [vp, C.c_int, C.POINTER(FmdStreamState)]
    L.fmd_batch_set_state.argtypes = [vp, C.c_int, C.POINTER(FmdStreamState)]
    L.fmd_batch_reset.argtypes = [vp]
    L.fmd_batch_last_kernel_ms.argtypes = [vp, C.POINTER(C.c_float)]
    L.fmd_batch_set_timing.argtypes = [vp, C.c_int]
    L.fmd_batch_wait_stream.argtypes = [vp, vp]
    L.fmd_batch_kernel_name.argtypes = [vp]
    L.fmd_batch_kernel_name.restype = C.c_char_p
    L.fmd_last_error.restype = C.c_char_p
    L.fmd_ingest_create.argtypes = [C.POINTER(vp), vp, C.c_int, C.c_uint32]
    L.fmd_ingest_destroy.argtypes = [vp]
    L.fmd_ingest_destroy.restype = None
    L.fmd_ingest_callback.argtypes = [vp, C.c_uint32, vp]
    L.fmd_ingest_callback.restype = None
    L.fmd_ingest_buffered.argtypes = [vp]
    L.fmd_ingest_buffered.restype = C.c_uint32
    L.fmd_ingest_dropped.argtypes = [vp]
    L.fmd_ingest_dropped.restype = C.c_uint64
    L.fmd_ingest_mute.argtypes = [vp, C.c_int]
    L.fmd_ingest_mute.restype = None
    L.fmd_ingest_set_overflow.argtypes = [vp, C.c_int]
    L.fmd_ingest_pop.argtypes = [vp, vp, C.c_uint32]
    L.fmd_ingest_pop.restype = C.c_uint32
    L.fmd_batch_pump.argtypes = [vp, C.c_int, vp, vp]
    L.fmd_batch_pump_begin.argtypes = [vp, C.c_int]
    L.fmd_batch_pump_end.argtypes = [vp, vp, vp]
    L.fmd_batch_run_device_levels.argtypes = [vp, vp, C.c_int, vp, vp, vp, vp, C.POINTER(FmdDebugTaps)]
    L.fmd_batch_run_host_levels.argtypes = [vp, vp, C.c_int, vp, vp, vp]
    L.fmd_batch_set_squelch.argtypes = [vp, vp, C.c_int]
    L.fmd_batch_get_squelch_hits.argtypes = [vp, C.c_int, C.POINTER(C.c_int32)]
    L.fmd_batch_set_squelch_hits.argtypes = [vp, C.c_int, C.c_int32]
    L.fmd_batch_spectrum_device.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, vp, vp]
    L.fmd_batch_spectrum_host.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, vp]
    L.fmd_subc_design.argtypes = [C.POINTER(FmdSubcConfig), vp]
    L.fmd_subc_create.argtypes = [C.POINTER(vp), C.POINTER(FmdSubcConfig), vp, C.c_int, C.c_int]
    L.fmd_batch_subc_create.argtypes = [C.POINTER(vp), vp, C.c_int, C.c_int, C.c_int, C.c_int]
    L.fmd_subc_destroy.argtypes = [vp]
    L.fmd_subc_destroy.restype = None
    L.fmd_subc_out_per_block.argtypes = [vp]
    L.fmd_subc_run_device.argtypes = [vp, vp, C.c_int, vp, vp]
    L.fmd_subc_run_host.argtypes = [vp, vp, C.c_int, vp]
    L.fmd_subc_get_state.argtypes = [vp, C.c_int, C.POINTER(FmdSubcState)]
    L.fmd_subc_set_state.argtypes = [vp, C.c_int, C.POINTER(FmdSubcState)]
    L.fmd_subc_reset.argtypes = [vp]
    L.fmd_subc_sync.argtypes = [vp]
    L.fmd_rds_design.argtypes = [C.POINTER(FmdRdsConfig), vp]
    L.fmd_rds_create.argtypes = [C.POINTER(vp), C.POINTER(FmdRdsConfig), vp, C.c_int, C.c_int]
    L.fmd_subc_rds_create.argtypes = [C.POINTER(vp), vp, C.c_int, C.c_int, C.c_int]
    L.fmd_rds_destroy.argtypes = [vp]
    L.fmd_rds_destroy.restype = None
    L.fmd_rds_bits_per_block.argtypes = [vp]
    L.fmd_rds_run_device.argtypes = [vp, vp, C.c_int, vp, vp, vp, vp, vp]
    L.fmd_rds_run_host.argtypes = [vp, vp, C.c_int, vp, vp, vp, vp]
    L.fmd_rds_last_y.argtypes = [vp, C.c_int, vp, vp]
    L.fmd_rds_get_state.argtypes = [vp, C.c_int, C.POINTER(FmdRdsState)]
    L.fmd_rds_set_state.argtypes = [vp, C.c_int, C.POINTER(FmdRdsState)]
    L.fmd_rds_reset.argtypes = [vp]
    L.fmd_rds_sync.argtypes = [vp]
    L.fmd_tuner_design.argtypes = [C.POINTER(FmdTunerConfig), vp]
    L.fmd_tuner_shift.argtypes = [C.POINTER(FmdTunerConfig), C.c_int, C.c_int, C.POINTER(C.c_int32)]
    L.fmd_tuner_create.argtypes = [C.POINTER(vp), C.POINTER(FmdTunerConfig), vp, C.c_int, C.c_int, C.c_int]
    L.fmd_batch_tuner_create.argtypes = [C.POINTER(vp), vp, C.c_int, C.c_int, C.c_int, C.c_int]
    L.fmd_tuner_destroy.argtypes = [vp]
    L.fmd_tuner_destroy.restype = None
    L.fmd_tuner_set_channel.argtypes = [vp, C.c_int, C.POINTER(FmdTunerChannel)]
    L.fmd_tuner_get_channel.argtypes = [vp, C.c_int, C.POINTER(FmdTunerChannel)]
    L.fmd_tuner_run_device.argtypes = [vp, vp, C.c_int, vp, vp, vp]
    L.fmd_tuner_run_host.argtypes = [vp, vp, C.c_int, vp]
    L.fmd_tuner_get_state.argtypes = [vp, C.c_int, C.POINTER(FmdTunerState)]
    L.fmd_tuner_set_state.argtypes = [vp, C.c_int, C.POINTER(FmdTunerState)]
    L.fmd_tuner_reset.argtypes = [vp]
    L.fmd_tuner_sync.argtypes = [vp]
    L.fmd_scan_candidates.argtypes = [C.POINTER(FmdScanConfig)]
    L.fmd_scan_create.argtypes = [C.POINTER(vp), C.POINTER(FmdScanConfig), C.c_int, C.c_int]
    L.fmd_batch_scan_create.argtypes = [C.POINTER(vp), vp, C.c_int, C.c_int, C.c_int, C.c_int]
    L.fmd_scan_destroy.argtypes = [vp]
    L.fmd_scan_destroy.restype = None
    L.fmd_scan_run_device.argtypes = [vp, vp, C.c_int, vp, vp, vp, vp]
    L.fmd_scan_run_host.argtypes = [vp, vp, C.c_int, vp, vp, vp]
    L.fmd_scan_sync.argtypes = [vp]
    L.fmd_stereo_create.argtypes = [C.POINTER(vp), C.POINTER(FmdStereoConfig), C.c_int, C.c_int]
    L.fmd_batch_stereo_create.argtypes = [C.POINTER(vp), vp, vp, C.POINTER(FmdStereoConfig)]
    L.fmd_stereo_destroy.argtypes = [vp]
    L.fmd_stereo_destroy.restype = None
    L.fmd_stereo_set_mode.argtypes = [vp, C.c_int]
    L.fmd_stereo_run_device.argtypes = [vp, vp, vp, vp, vp, C.c_int, vp, vp, vp, vp]
    L.fmd_stereo_run_host.argtypes = [vp, vp, vp, vp, vp, C.c_int, vp, vp, vp]
    L.fmd_stereo_get_state.argtypes = [vp, C.c_int, C.POINTER(FmdStereoState)]
    L.fmd_stereo_set_state.argtypes = [vp, C.c_int, C.POINTER(FmdStereoState)]
    L.fmd_stereo_reset.argtypes = [vp]
    L.fmd_stereo_sync.argtypes = [vp]
    L.fmd_rds_decoder_init.argtypes = [C.POINTER(FmdRdsDecoder)]
    L.fmd_rds_decoder_init.restype = None
    L.fmd_rds_decoder_push.argtypes = [C.POINTER(FmdRdsDecoder), vp, C.c_int, vp, C.c_int]
    L.fmd_rds_info_init.argtypes = [C.POINTER(FmdRdsInfo)]
    L.fmd_rds_info_init.restype = None
    L.fmd_rds_info_update.argtypes = [C.POINTER(FmdRdsInfo), C.POINTER(FmdRdsGroup)]
    for name in ("init_lp_real_f32", "deinit_lp_real_f32", "demod_init", "rotate_90_u8_f32", "u8_f32",
                 "full_demod", "fmd_demod_release"):
        getattr(L, name).argtypes = [C.POINTER(DemodState)]
        getattr(L, name).restype = None
    _lib = L
    return L


def _check(rc, what):
    if rc < 0:
        raise FmdError("%s failed (%d): %s" % (what, rc, lib().fmd_last_error().decode()))
    return rc


def device_count():
    return int(lib().fmd_device_count())


def wbfm_config(rate_in=300000, rate_out=None, rate_out2=48000, mode=2, size=None, deemph=True,
                deemph_lambda=None, volume=0.4, offset_tuning=False, block_len=262144,
                math=MATH_EXACT, output_rate=None, tau=50e-6):
    """fmd_config with the reference's defaults (demod_init / -X / -Y, src/rtl_fm_player.c:1156-1195)."""
    if size is None:
        size = 128 if mode == 1 else 90
    if rate_out is None:
        rate_out = rate_in
    if output_rate is None:
        output_rate = rate_out2 if rate_out2 > 0 else rate_out
    if deemph_lambda is None:
        deemph_lambda = float(lib().fmd_deemph_lambda(int(output_rate), float(tau)))
    return FmdConfig(rate_in, rate_out, rate_out2, mode, size, int(bool(deemph)), int(bool(offset_tuning)),
                     deemph_lambda, volume, block_len, math)


def design_taps(cfg):
    t = FmdTaps()
    _check(lib().fmd_design_taps(C.byref(cfg), C.byref(t)), "fmd_design_taps")
    return t


def config_family(cfg, taps=None):
    """The kernel family fmd_batch_create would run for this configuration (needs no device); raises FmdError for one it refuses."""
    rc = lib().fmd_config_family(C.byref(cfg), C.byref(taps) if taps is not None else None)
    _check(rc if rc < 0 else 0, "fmd_config_family")
    return rc


def config_error_estimate(cfg, taps=None):
    """fmd_config_error_estimate as a dict: what the fixed-point second stage adds to a PCM value (rms estimate, worst-case bound and its terms, per
    filter) and the family the configuration resolves to.  Needs no device."""
    e = FmdErrorEstimate()
    _check(lib().fmd_config_error_estimate(C.byref(cfg), C.byref(taps) if taps is not None else None, C.byref(e)), "fmd_config_error_estimate")
    return {"family": e.family, "limit_rms_lsb": e.limit_rms_lsb,
            "filters": [{k: getattr(e.f[i], k) for k, _ in _FmdFilterError._fields_} for i in range(e.filters)]}


def _ptr(x):
    """Device pointer of a torch tensor, or a raw integer address."""
    if x is None:
        return None
    if hasattr(x, "data_ptr"):
        return C.c_void_p(x.data_ptr())
    return C.c_void_p(int(x))


def subc_design(cfg):
    """fmd_subc_design: the default taps of a subcarrier configuration, float32 [n_taps] (needs no device)."""
    taps = np.zeros(max(int(cfg.n_taps), 0) if 0 <= cfg.n_taps <= 256 else 256, dtype=np.float32)
    _check(lib().fmd_subc_design(C.byref(cfg), taps.ctypes.data), "fmd_subc_design")
    return taps


class _Object:
    """What the receiver objects beside BatchDemod share: the handle of a C object whose functions are fmd_<_PREFIX>_*, made by its create or
    taken over, its close and its sync."""
    _PREFIX = None

    def _fn(self, name):
        return getattr(lib(), "fmd_%s_%s" % (self._PREFIX, name))

    def _open(self, handle, cfg, *args, taps=False):
        """self._h: `handle`, or what fmd_<prefix>_create(cfg, [taps,] *args) makes (taps: float32 [cfg.n_taps], None for the default ones; False: the
        create takes none)."""
        self.cfg = cfg
        self._h = handle if handle is not None else C.c_void_p()
        if handle is None:
            if taps is not False:
                t = None
                if taps is not None:
                    t = np.ascontiguousarray(taps, dtype=np.float32)
                    assert t.shape == (cfg.n_taps,)
                args = (t.ctypes.data if t is not None else None,) + args
            _check(self._fn("create")(C.byref(self._h), C.byref(cfg), *args), "fmd_%s_create" % self._PREFIX)

    def close(self):
        if getattr(self, "_h", None):
            self._fn("destroy")(self._h)
            self._h = None

    __del__ = close

    def sync(self):
        _check(self._fn("sync")(self._h), "fmd_%s_sync" % self._PREFIX)


class _StatefulObject(_Object):
    """... and, for the ones that carry state from launch to launch (one _STATE struct per stream), its access."""
    _STATE = None

    def get_state(self, stream=0):
        st = self._STATE()
        _check(self._fn("get_state")(self._h, int(stream), C.byref(st)), "fmd_%s_get_state" % self._PREFIX)
        return st

    def set_state(self, stream, st):
        _check(self._fn("set_state")(self._h, int(stream), C.byref(st)), "fmd_%s_set_state" % self._PREFIX)

    def reset(self):
        _check(self._fn("reset")(self._h), "fmd_%s_reset" % self._PREFIX)


class Subcarrier(_StatefulObject):
    """MPX subcarrier receiver (fmd_subc_*): complex down-conversion of the discriminator output at cfg.fc, low-pass, decimation, for n_streams
    independent streams.  taps: float32 [n_taps] of the caller's, or None for fmd_subc_design's."""
    _PREFIX, _STATE = "subc", FmdSubcState

    def __init__(self, cfg, n_streams, taps=None, device=-1, _handle=None):
        self.n_streams = int(n_streams)
        self._open(_handle, cfg, self.n_streams, device, taps=taps)
        self.out_per_block = lib().fmd_subc_out_per_block(self._h)

    def run_device(self, d_v, n_blocks, d_z, hip_stream=None):
        """Asynchronous: d_v float32 [n_streams, n_blocks, block_samples] -> d_z float32 [n_streams, n_blocks, out_per_block, 2] (re, im), both on
        the device (tensors or raw addresses), on `hip_stream` (None: the object's own stream - the buffers must be ready there)."""
        _check(lib().fmd_subc_run_device(self._h, _ptr(d_v), int(n_blocks), _ptr(d_z), _ptr(hip_stream)), "fmd_subc_run_device")

    def run_host(self, v, n_blocks):
        """v: float32 [n_streams, n_blocks, block_samples] -> z complex64 [n_streams, n_blocks, out_per_block] (fmd_subc_run_host)."""
        v = np.ascontiguousarray(v, dtype=np.float32)
        assert v.size == self.n_streams * n_blocks * self.cfg.block_samples
        z = np.zeros((self.n_streams, n_blocks, self.out_per_block), dtype=np.complex64)
        _check(lib().fmd_subc_run_host(self._h, v.ctypes.data, int(n_blocks), z.ctypes.data), "fmd_subc_run_host")
        return z


def tuner_design(cfg):
    """fmd_tuner_design: the default taps of a tuner configuration, float32 [n_taps] (needs no device)."""
    taps = np.zeros(64, dtype=np.float32)
    _check(lib().fmd_tuner_design(C.byref(cfg), taps.ctypes.data), "fmd_tuner_design")
    return taps[:cfg.n_taps].copy()


def tuner_shift(cfg, offset_hz, offset_tuning=False):
    """fmd_tuner_shift: the steps of cfg.step_hz that bring a station at offset_hz from the capture's centre to where the chain looks (-rate / 4, or 0
    with offset_tuning); FmdError when that is not on the grid (needs no device)."""
    sh = C.c_int32()
    _check(lib().fmd_tuner_shift(C.byref(cfg), int(offset_hz), int(bool(offset_tuning)), C.byref(sh)), "fmd_tuner_shift")
    return int(sh.value)


class Tuner(_StatefulObject):
    """Channel tuner (fmd_tuner_*): n_channels stations out of n_sources captures - mix by a channel's shift, low-pass, requantise to u8 IQ in the layout
    BatchDemod.run_device takes.  taps: float32 [n_taps] of the caller's, or None for fmd_tuner_design's."""
    _PREFIX, _STATE = "tuner", FmdTunerState

    def __init__(self, cfg, n_sources, n_channels, taps=None, device=-1, _handle=None):
        self.n_sources, self.n_channels = int(n_sources), int(n_channels)
        self._open(_handle, cfg, self.n_sources, self.n_channels, device, taps=taps)

    def set_channel(self, channel, source=0, shift=0, gain=1.0):
        ch = FmdTunerChannel(int(source), int(shift), float(gain), 0)
        _check(lib().fmd_tuner_set_channel(self._h, int(channel), C.byref(ch)), "fmd_tuner_set_channel")

    def get_channel(self, channel):
        ch = FmdTunerChannel()
        _check(lib().fmd_tuner_get_channel(self._h, int(channel), C.byref(ch)), "fmd_tuner_get_channel")
        return ch

    def run_device(self, d_iq, n_blocks, d_out, d_y=None, hip_stream=None):
        """Asynchronous: d_iq uint8 [n_sources, n_blocks, block_len] -> d_out uint8 [n_channels, n_blocks, block_len] and, where given, d_y float32
        [n_channels, n_blocks, block_len / 2, 2], all on the device (tensors or raw addresses), on `hip_stream` (None: the object's own stream)."""
        _check(lib().fmd_tuner_run_device(self._h, _ptr(d_iq), int(n_blocks), _ptr(d_out), _ptr(d_y), _ptr(hip_stream)), "fmd_tuner_run_device")

    def run_host(self, iq, n_blocks):
        """iq: uint8 [n_sources, n_blocks, block_len] -> uint8 [n_channels, n_blocks, block_len] (fmd_tuner_run_host)."""
        iq = np.ascontiguousarray(iq, dtype=np.uint8)
        assert iq.size == self.n_sources * n_blocks * self.cfg.block_len
        out = np.zeros((self.n_channels, n_blocks, self.cfg.block_len), dtype=np.uint8)
        _check(lib().fmd_tuner_run_host(self._h, iq.ctypes.data, int(n_blocks), out.ctypes.data), "fmd_tuner_run_host")
        return out

    def get_state(self, source=0):               # (the state is per source: the keyword's name differs)
        return super().get_state(source)

    def set_state(self, source, st):
        super().set_state(source, st)


SCAN_STATION_DTYPE = np.dtype([("offset_hz", "<i4"), ("candidate", "<i4"), ("power", "<f4"), ("snr", "<f4"), ("centroid_hz", "<f4"),
                               ("reserved", "<i4", (3,))])     # fmd_scan_station as a numpy record (32 bytes)


def scan_candidates(cfg):
    """fmd_scan_candidates: C = 2 cmax + 1, the candidates of a scan configuration; FmdError outside the supported range (needs no device)."""
    return _check(lib().fmd_scan_candidates(C.byref(cfg)), "fmd_scan_candidates")


class Scan(_Object):
    """Station finder (fmd_scan_*): power spectra in the layout BatchDemod.spectrum_device writes to a ranked list of stations per stream.  Stateless:
    a launch's result depends on its d_power and the configuration alone."""
    _PREFIX = "scan"

    def __init__(self, cfg, n_streams, device=-1, _handle=None):
        self.n_streams = int(n_streams)
        self.n_candidates = scan_candidates(cfg)
        self._open(_handle, cfg, self.n_streams, device)

    def run_device(self, d_power, n_blocks, d_stations, d_counts, d_chan=None, hip_stream=None):
        """Asynchronous: d_power float32 [n_streams, n_blocks, n_bins] -> d_stations [n_streams, max_stations] records of 32 bytes (SCAN_STATION_DTYPE),
        d_counts int32 [n_streams, 2] = {found, written} and, where given, d_chan float32 [n_streams, n_candidates], all on the device (tensors or raw
        addresses), on `hip_stream` (None: the object's own stream - the buffers must be ready there)."""
        _check(lib().fmd_scan_run_device(self._h, _ptr(d_power), int(n_blocks), _ptr(d_stations), _ptr(d_counts), _ptr(d_chan), _ptr(hip_stream)),
               "fmd_scan_run_device")

    def run_host(self, power, n_blocks, chan=True):
        """power: float32 [n_streams, n_blocks, n_bins] -> (stations [n_streams, max_stations] of SCAN_STATION_DTYPE, counts int32 [n_streams, 2],
        chan float32 [n_streams, n_candidates] or None) (fmd_scan_run_host)."""
        power = np.ascontiguousarray(power, dtype=np.float32)
        assert power.size == self.n_streams * n_blocks * self.cfg.n_bins
        st = np.zeros((self.n_streams, self.cfg.max_stations), dtype=SCAN_STATION_DTYPE)
        counts = np.zeros((self.n_streams, 2), dtype=np.int32)
        ch = np.zeros((self.n_streams, self.n_candidates), dtype=np.float32) if chan else None
        _check(lib().fmd_scan_run_host(self._h, power.ctypes.data, int(n_blocks), st.ctypes.data, counts.ctypes.data, ch.ctypes.data if chan else None),
               "fmd_scan_run_host")
        return st, counts, ch


STEREO_INFO_DTYPE = np.dtype([("pilot_ms", "<f4"), ("g_start", "<f4"), ("g_step", "<f4"), ("g_end", "<f4"), ("stereo", "<i4"), ("frames", "<i4"),
                              ("reserved", "<i4", (2,))])      # fmd_stereo_info as a numpy record (32 bytes)
STEREO_METER_DTYPE = np.dtype([("peak_l", "<i4"), ("peak_r", "<i4"), ("full_scale", "<i4"), ("frames", "<i4"), ("sumsq_l", "<u8"),
                               ("sumsq_r", "<u8")])           # fmd_stereo_meter (32 bytes)


class Stereo(_StatefulObject):
    """Stereo control (fmd_stereo_*): the pilot indicator with hysteresis, the blend of the stereo PCM towards mono and the audio meters, for
    n_streams independent streams.  BatchDemod.stereo(pilot, cfg) takes pcm_stride, n_streams and device from a batch and pilot_per_block from a
    Subcarrier at 19 kHz."""
    _PREFIX, _STATE = "stereo", FmdStereoState

    def __init__(self, cfg, n_streams, device=-1, _handle=None):
        self.n_streams = int(n_streams)
        self._open(_handle, cfg, self.n_streams, device)

    def set_mode(self, mode):
        """STEREO_AUTO (the default), STEREO_FORCE_MONO or STEREO_FORCE_STEREO, from the next launch on (a captured launch keeps its own)."""
        _check(lib().fmd_stereo_set_mode(self._h, int(mode)), "fmd_stereo_set_mode")

    def run_device(self, d_pcm, d_lens, d_z, d_quality, n_blocks, d_out, d_info, d_meter=None, hip_stream=None):
        """Asynchronous: d_pcm int16 [n_streams, n_blocks, pcm_stride] and d_lens int32 [n_streams, n_blocks] as BatchDemod.run_device wrote them, d_z
        float32 [n_streams, n_blocks, pilot_per_block, 2] of a Subcarrier at 19 kHz (None: forced modes only), d_quality float32 [n_streams, n_blocks] or
        None -> d_out (may be d_pcm), d_info [n_streams, n_blocks] records of STEREO_INFO_DTYPE and, where given, d_meter of STEREO_METER_DTYPE; all on the
        device (tensors or raw addresses), on `hip_stream` (None: the object's own stream - the buffers must be ready there)."""
        _check(lib().fmd_stereo_run_device(self._h, _ptr(d_pcm), _ptr(d_lens), _ptr(d_z), _ptr(d_quality), int(n_blocks), _ptr(d_out), _ptr(d_info),
                                           _ptr(d_meter), _ptr(hip_stream)), "fmd_stereo_run_device")

    def run_host(self, pcm, lens, z, quality, n_blocks):
        """pcm int16 [n_streams, n_blocks, pcm_stride], lens int32 [S, nb], z complex64 [S, nb, pilot_per_block] or None, quality float32 [S, nb] or
        None -> (out int16 like pcm, info [S, nb] of STEREO_INFO_DTYPE, meter [S, nb] of STEREO_METER_DTYPE) (fmd_stereo_run_host)."""
        S = self.n_streams
        pcm = np.ascontiguousarray(pcm, dtype=np.int16)
        lens = np.ascontiguousarray(lens, dtype=np.int32)
        assert pcm.size == S * n_blocks * self.cfg.pcm_stride and lens.size == S * n_blocks
        if z is not None:
            z = np.ascontiguousarray(z, dtype=np.complex64)
            assert z.size == S * n_blocks * self.cfg.pilot_per_block
        if quality is not None:
            quality = np.ascontiguousarray(quality, dtype=np.float32)
            assert quality.size == S * n_blocks
        out = np.zeros((S, n_blocks, self.cfg.pcm_stride), dtype=np.int16)
        info = np.zeros((S, n_blocks), dtype=STEREO_INFO_DTYPE)
        meter = np.zeros((S, n_blocks), dtype=STEREO_METER_DTYPE)
        _check(lib().fmd_stereo_run_host(self._h, pcm.ctypes.data, lens.ctypes.data, z.ctypes.data if z is not None else None,
                                         quality.ctypes.data if quality is not None else None, int(n_blocks), out.ctypes.data, info.ctypes.data,
                                         meter.ctypes.data), "fmd_stereo_run_host")
        return out, info, meter


def rds_design(cfg):
    """fmd_rds_design: the default matched-filter taps of an RDS configuration, float32 [n_taps] (needs no device)."""
    taps = np.zeros(64, dtype=np.float32)
    _check(lib().fmd_rds_design(C.byref(cfg), taps.ctypes.data), "fmd_rds_design")
    return taps[:cfg.n_taps].copy()


class Rds(_StatefulObject):
    """RDS receiver (fmd_rds_*): the 57 kHz baseband z of a Subcarrier to soft bits, for n_streams independent streams.  taps: float32 [n_taps] of
    the caller's, or None for fmd_rds_design's.  Rds.from_subcarrier(sub) takes rates, block, n_streams and device from a Subcarrier."""
    _PREFIX, _STATE = "rds", FmdRdsState

    def __init__(self, cfg, n_streams, taps=None, device=-1, _handle=None):
        self.n_streams = int(n_streams)
        self._open(_handle, cfg, self.n_streams, device, taps=taps)
        self.bits_per_block = lib().fmd_rds_bits_per_block(self._h)

    @classmethod
    def from_subcarrier(cls, sub, n_taps=64, avg_blocks=8, max_blocks=16):
        h = C.c_void_p()
        _check(lib().fmd_subc_rds_create(C.byref(h), sub._h, int(n_taps), int(avg_blocks), int(max_blocks)), "fmd_subc_rds_create")
        cfg = FmdRdsConfig(sub.cfg.rate_in // sub.cfg.decim, sub.cfg.block_samples // sub.cfg.decim, int(n_taps), int(avg_blocks), int(max_blocks))
        return cls(cfg, sub.n_streams, _handle=h)

    def run_device(self, d_z, n_blocks, d_soft, d_lens, d_first=None, d_est=None, hip_stream=None):
        """Asynchronous: d_z float32 [n_streams, n_blocks, block_z, 2] -> d_soft float32 [n_streams, n_blocks, bits_per_block], d_lens int32
        [n_streams, n_blocks], optionally d_first int64 [n_streams, n_blocks] and d_est float32 [n_streams, n_blocks, 4], all on the device, on
        `hip_stream` (None: the object's own stream - the buffers must be ready there)."""
        _check(lib().fmd_rds_run_device(self._h, _ptr(d_z), int(n_blocks), _ptr(d_soft), _ptr(d_lens), _ptr(d_first), _ptr(d_est), _ptr(hip_stream)),
               "fmd_rds_run_device")

    def run_host(self, z, n_blocks):
        """z: complex64 [n_streams, n_blocks, block_z] -> (soft float32 [S, nb, bits_per_block], lens int32 [S, nb], first int64 [S, nb],
        est float32 [S, nb, 4]) (fmd_rds_run_host)."""
        z = np.ascontiguousarray(z, dtype=np.complex64)
        assert z.size == self.n_streams * n_blocks * self.cfg.block_z
        S = self.n_streams
        soft = np.zeros((S, n_blocks, self.bits_per_block), dtype=np.float32)
        lens = np.zeros((S, n_blocks), dtype=np.int32)
        first = np.zeros((S, n_blocks), dtype=np.int64)
        est = np.zeros((S, n_blocks, 4), dtype=np.float32)
        _check(lib().fmd_rds_run_host(self._h, z.ctypes.data, int(n_blocks), soft.ctypes.data, lens.ctypes.data, first.ctypes.data, est.ctypes.data),
               "fmd_rds_run_host")
        return soft, lens, first, est

    def last_y(self, n_blocks):
        """(y complex64 [S, nb, block_z], Tm complex64 [S, nb]) of the most recent launch (fmd_rds_last_y)."""
        y = np.zeros((self.n_streams, n_blocks, self.cfg.block_z), dtype=np.complex64)
        tm = np.zeros((self.n_streams, n_blocks), dtype=np.complex64)
        _check(lib().fmd_rds_last_y(self._h, int(n_blocks), y.ctypes.data, tm.ctypes.data), "fmd_rds_last_y")
        return y, tm


class RdsDecoder:
    """RDS block / group decoder with the PI / PTY / PS collector (fmd_rds_decoder_*, fmd_rds_info_*: no device).  push(soft) takes soft bits in
    any split and returns the groups completed as (blk0, blk1, blk2, blk3, ok_mask, version) tuples; pi / pty / ps are what the groups so far said."""

    def __init__(self):
        self.dec = FmdRdsDecoder()
        self.info = FmdRdsInfo()
        lib().fmd_rds_decoder_init(C.byref(self.dec))
        lib().fmd_rds_info_init(C.byref(self.info))

    def push(self, soft):
        soft = np.ascontiguousarray(soft, dtype=np.float32).reshape(-1)
        out = (FmdRdsGroup * (soft.size // 104 + 2))()
        n = _check(lib().fmd_rds_decoder_push(C.byref(self.dec), soft.ctypes.data, soft.size, out, len(out)), "fmd_rds_decoder_push")
        assert self.dec.consumed == soft.size
        for i in range(n):
            lib().fmd_rds_info_update(C.byref(self.info), C.byref(out[i]))
        return [(out[i].blk[0], out[i].blk[1], out[i].blk[2], out[i].blk[3], out[i].ok_mask, out[i].version) for i in range(n)]

    @property
    def synced(self):
        return bool(self.dec.synced)

    @property
    def pi(self):
        return self.info.pi if self.info.have_pi else None

    @property
    def pty(self):
        return self.info.pty

    @property
    def ps(self):
        return bytes(self.info.ps[:8]).replace(b"\0", b" ").decode("latin-1") if self.info.ps_mask else ""


class BatchDemod:
    """n_streams independent demodulators; thin wrapper of the fmd_batch_* C API."""

    def __init__(self, cfg, n_streams, taps=None, device=-1):
        self.cfg = cfg
        self.n_streams = int(n_streams)
        self._h = C.c_void_p()
        _check(lib().fmd_batch_create(C.byref(self._h), C.byref(cfg), C.byref(taps) if taps else None,
                                      self.n_streams, device), "fmd_batch_create")
        self.pcm_stride = lib().fmd_batch_pcm_stride(self._h)
        self.channels = 2 if cfg.mode == 2 else 1
        self.math = lib().fmd_batch_math(self._h)      # the kernel family MATH_FAST resolved to

    def close(self):
        if getattr(self, "_h", None):
            lib().fmd_batch_destroy(self._h)
            self._h = None

    __del__ = close

    @staticmethod
    def _debug_taps(debug):
        return FmdDebugTaps(*[(_ptr(debug.get(k)).value if debug.get(k) is not None else None) for k in ("y", "v", "mpx", "prof")])

    def run_device(self, d_iq, n_blocks, d_pcm, d_lens, hip_stream=None, debug=None):
        """Asynchronous device-resident run (tensors or raw device addresses) on `hip_stream` (None: the batch's own stream - the
        buffers must be ready there: torch.cuda.synchronize(), or wait_stream(), after producing them on torch's stream)."""
        if debug is None:
            rc = lib().fmd_batch_run_device(self._h, _ptr(d_iq), n_blocks, _ptr(d_pcm), _ptr(d_lens),
                                            _ptr(hip_stream))
        else:
            dbg = self._debug_taps(debug)
            rc = lib().fmd_batch_run_device_debug(self._h, _ptr(d_iq), n_blocks, _ptr(d_pcm), _ptr(d_lens),
                                                  _ptr(hip_stream), C.byref(dbg))
        _check(rc, "fmd_batch_run_device")

    def sync(self):
        _check(lib().fmd_batch_sync(self._h), "fmd_batch_sync")

    def wait_stream(self, producer_stream=None):
        """Order this batch's own stream behind what is queued on `producer_stream` (a hipStream_t address; None: torch's current
        stream).  run_device() with hip_stream=None launches on the batch's OWN stream: tensors another stream is still filling -
        or memory torch's allocator handed out in its stream's order - are only safe after this or a synchronisation."""
        if producer_stream is None:
            import torch
            producer_stream = torch.cuda.current_stream().cuda_stream
        _check(lib().fmd_batch_wait_stream(self._h, _ptr(producer_stream)), "fmd_batch_wait_stream")

    def run_host(self, iq, n_blocks):
        """iq: uint8 [n_streams, n_blocks, block_len] -> (pcm [S, B, stride] int16, lens [S, B])."""
        iq = np.ascontiguousarray(iq, dtype=np.uint8)
        assert iq.size == self.n_streams * n_blocks * self.cfg.block_len
        pcm = np.zeros((self.n_streams, n_blocks, self.pcm_stride), dtype=np.int16)
        lens = np.zeros((self.n_streams, n_blocks), dtype=np.int32)
        _check(lib().fmd_batch_run_host(self._h, iq.ctypes.data, n_blocks, pcm.ctypes.data, lens.ctypes.data),
               "fmd_batch_run_host")
        return pcm, lens

    def run_device_levels(self, d_iq, n_blocks, d_pcm, d_lens, d_levels, hip_stream=None, debug=None):
        """run_device that also writes each block's channel level to d_levels (float32 [n_streams, n_blocks] on the device, or None: squelch
        alone); see fmd_batch_run_device_levels."""
        dbg = C.byref(self._debug_taps(debug)) if debug is not None else None
        _check(lib().fmd_batch_run_device_levels(self._h, _ptr(d_iq), n_blocks, _ptr(d_pcm), _ptr(d_lens), _ptr(d_levels), _ptr(hip_stream), dbg),
               "fmd_batch_run_device_levels")

    def run_host_levels(self, iq, n_blocks):
        """run_host that also returns each block's channel level: (pcm, lens, levels float32 [S, B])."""
        iq = np.ascontiguousarray(iq, dtype=np.uint8)
        assert iq.size == self.n_streams * n_blocks * self.cfg.block_len
        pcm = np.zeros((self.n_streams, n_blocks, self.pcm_stride), dtype=np.int16)
        lens = np.zeros((self.n_streams, n_blocks), dtype=np.int32)
        levels = np.zeros((self.n_streams, n_blocks), dtype=np.float32)
        _check(lib().fmd_batch_run_host_levels(self._h, iq.ctypes.data, n_blocks, pcm.ctypes.data, lens.ctypes.data, levels.ctypes.data),
               "fmd_batch_run_host_levels")
        return pcm, lens, levels

    def set_squelch(self, thresholds, conseq=10):
        """rtl_fm's power squelch on every run path: thresholds per stream (<= 0: off for that stream; None: squelch off), conseq blocks below
        the threshold before a stream closes (the reference's default 10).  Every stream starts closed (hits = conseq + 1)."""
        if thresholds is None:
            _check(lib().fmd_batch_set_squelch(self._h, None, int(conseq)), "fmd_batch_set_squelch")
            return
        thr = np.ascontiguousarray(thresholds, dtype=np.float32)
        assert thr.shape == (self.n_streams,)
        _check(lib().fmd_batch_set_squelch(self._h, thr.ctypes.data, int(conseq)), "fmd_batch_set_squelch")

    def squelch_hits(self, stream):
        h = C.c_int32()
        _check(lib().fmd_batch_get_squelch_hits(self._h, int(stream), C.byref(h)), "fmd_batch_get_squelch_hits")
        return h.value

    def set_squelch_hits(self, stream, hits):
        _check(lib().fmd_batch_set_squelch_hits(self._h, int(stream), int(hits)), "fmd_batch_set_squelch_hits")

    def spectrum_device(self, d_iq, n_blocks, n_bins, d_power, window=WINDOW_HANN, hip_stream=None):
        """Averaged power spectrum of every block of the capture into d_power (float32 [n_streams, n_blocks, n_bins] on the device); asynchronous,
        touches no demodulator state; see fmd_batch_spectrum_device."""
        _check(lib().fmd_batch_spectrum_device(self._h, _ptr(d_iq), int(n_blocks), int(n_bins), int(window), _ptr(d_power), _ptr(hip_stream)),
               "fmd_batch_spectrum_device")

    def spectrum_host(self, iq, n_blocks, n_bins, window=WINDOW_HANN):
        """iq: uint8 [n_streams, n_blocks, block_len] -> power float32 [S, B, n_bins], natural FFT order (fmd_batch_spectrum_host)."""
        iq = np.ascontiguousarray(iq, dtype=np.uint8)
        assert iq.size == self.n_streams * n_blocks * self.cfg.block_len
        power = np.zeros((self.n_streams, n_blocks, max(int(n_bins), 1)), dtype=np.float32)
        _check(lib().fmd_batch_spectrum_host(self._h, iq.ctypes.data, int(n_blocks), int(n_bins), int(window), power.ctypes.data),
               "fmd_batch_spectrum_host")
        return power

    def subcarrier(self, fc, bw, n_taps=128, decim=16):
        """A Subcarrier over this batch's `v` debug tap (rate_in, block_len / 16 samples per block, n_streams and device from the batch; default
        taps): pass the tap's buffer of a run_device(debug={"v": ...}) straight to its run_device.  fmd_batch_subc_create."""
        h = C.c_void_p()
        _check(lib().fmd_batch_subc_create(C.byref(h), self._h, int(fc), int(bw), int(n_taps), int(decim)), "fmd_batch_subc_create")
        return Subcarrier(FmdSubcConfig(self.cfg.rate_in, int(fc), int(bw), int(n_taps), int(decim), self.cfg.block_len // 16), self.n_streams, _handle=h)

    def tuner(self, step_hz, bw, n_taps=64, n_sources=1):
        """A Tuner whose output feeds this batch: rate = 8 rate_in, block_len, one channel per stream and the device from the batch; default taps.  Its
        run_device's d_out is passed straight to this batch's run_device.  fmd_batch_tuner_create."""
        h = C.c_void_p()
        _check(lib().fmd_batch_tuner_create(C.byref(h), self._h, int(step_hz), int(bw), int(n_taps), int(n_sources)), "fmd_batch_tuner_create")
        return Tuner(FmdTunerConfig(8 * self.cfg.rate_in, int(step_hz), int(bw), int(n_taps), self.cfg.block_len, 0), int(n_sources), self.n_streams,
                     _handle=h)

    def scan(self, n_bins, raster_hz, bw, max_stations=16):
        """A Scan over this batch's spectra: rate = 8 rate_in, one list per stream and the device from the batch; min_sep 1, floor_permille 250,
        dc_guard 0, threshold 4.  Its run_device takes the d_power spectrum_device wrote.  fmd_batch_scan_create."""
        h = C.c_void_p()
        _check(lib().fmd_batch_scan_create(C.byref(h), self._h, int(n_bins), int(raster_hz), int(bw), int(max_stations)), "fmd_batch_scan_create")
        return Scan(FmdScanConfig(8 * self.cfg.rate_in, int(n_bins), int(raster_hz), int(bw), 1, 250, 0, int(max_stations), 4.0), self.n_streams, _handle=h)

    def stereo(self, pilot, cfg):
        """A Stereo over this batch's PCM: pcm_stride, n_streams and the device from the batch, pilot_per_block from `pilot` (a Subcarrier at 19 kHz, or
        None: forced modes only); thresholds, hold, blend range and slew from cfg, an FmdStereoConfig.  fmd_batch_stereo_create."""
        h = C.c_void_p()
        _check(lib().fmd_batch_stereo_create(C.byref(h), self._h, pilot._h if pilot is not None else None, C.byref(cfg)), "fmd_batch_stereo_create")
        full = FmdStereoConfig(self.pcm_stride, pilot.out_per_block if pilot is not None else 0, cfg.hold_blocks, 0, cfg.pilot_on, cfg.pilot_off,
                               cfg.blend_lo, cfg.blend_hi, cfg.slew)
        return Stereo(full, self.n_streams, _handle=h)

    def run_host_concat(self, iq, n_blocks):
        """Like run_host but returns, per stream, the PCM of all blocks concatenated."""
        pcm, lens = self.run_host(iq, n_blocks)
        out = [np.concatenate([pcm[s, b, :lens[s, b]] for b in range(n_blocks)]) for s in range(self.n_streams)]
        return out, lens

    def set_time_split(self, workers_per_cu):
        """Time chunks per launch: > 0 workers per CU to cut for, 0 default, < 0 never cut; see fmd_batch_set_time_split."""
        _check(lib().fmd_batch_set_time_split(self._h, int(workers_per_cu)), "fmd_batch_set_time_split")

    def set_timing(self, on):
        """Bracket every launch with an event pair (default) or not; see fmd_batch_set_timing."""
        _check(lib().fmd_batch_set_timing(self._h, int(bool(on))), "fmd_batch_set_timing")

    def last_kernel_ms(self):
        ms = C.c_float()
        _check(lib().fmd_batch_last_kernel_ms(self._h, C.byref(ms)), "fmd_batch_last_kernel_ms")
        return ms.value

    def kernel_name(self):
        return lib().fmd_batch_kernel_name(self._h).decode()

    def get_state(self, stream=0):
        st = FmdStreamState()
        _check(lib().fmd_batch_get_state(self._h, stream, C.byref(st)), "fmd_batch_get_state")
        return st

    def set_state(self, stream, st):
        _check(lib().fmd_batch_set_state(self._h, stream, C.byref(st)), "fmd_batch_set_state")

    def reset(self):
        _check(lib().fmd_batch_reset(self._h), "fmd_batch_reset")
