"""ctypes binding of libif_fir.so — one Python method per C entry point of include/if_fir.h (same names, same
argument meaning, 1/0 status turned into IfFirError).  No compute happens here.

Two libraries: libif_fir.so is the product (include/if_fir.h); libif_fir_dev.so is the same code with the development
hooks of include/if_fir_debug.h compiled in (diagnostic tuning variants, stamps, the host-only table / schedule / plan
dumps, if_fir_time_device).  `IfFir(..., dev=True)` / `IfFirMc(..., dev=True)` and the module-level debug_* helpers use
the development library; everything else uses the product."""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libif_fir.so")
DEV_LIB_PATH = os.path.join(_HERE, "libif_fir_dev.so")

INPUT_F32, INPUT_I16 = 0, 1
OUTPUT_F32, OUTPUT_I16 = 0, 1
BACKEND_AUTO, BACKEND_HIP_DIRECT, BACKEND_HIP_TAPSPLIT, BACKEND_HIP_GENERIC, BACKEND_HIP_FFT = range(5)
WINDOW_RECT, WINDOW_HAMMING, WINDOW_HANN, WINDOW_BLACKMAN = range(4)

# every symbol include/if_fir.h declares (tests check the library exports all of them)
EXPORTS = [
    "if_bpf_design", "if_bpf_design_complex", "if_fir_init", "if_fir_init_complex", "if_fir_destroy", "if_fir_reset", "if_fir_set_backend", "if_fir_get_backend",
    "if_fir_set_tuning", "if_fir_set_input_format", "if_fir_set_stream", "if_fir_synchronize", "if_fir_last_error", "if_fir_out_count",
    "if_fir_process", "if_fir_process_device", "if_fir_synth_device", "if_fir_dev_alloc",
    "if_fir_dev_free", "if_fir_dev_upload", "if_fir_dev_download", "if_fir_device_info",
    "if_fir_set_nco", "if_fir_get_nco", "if_fir_channelizer_process_device", "if_fir_channelizer_process_device_freq", "if_fir_host_alloc", "if_fir_host_free",
    "if_fir_power_device",
    "if_fir_mc_owner", "if_fir_mc_unique_id", "if_fir_mc_init", "if_fir_mc_destroy", "if_fir_mc_reset",
    "if_fir_mc_set_input_format", "if_fir_mc_process_device", "if_fir_mc_channel_ctx", "if_fir_mc_last_error",
    "if_fir_mc_set_chunk_samples", "if_fir_mc_get_chunk_samples",
    "if_fir_interp_init", "if_fir_interp_init_complex", "if_fir_interp_destroy", "if_fir_interp_reset", "if_fir_interp_set_backend",
    "if_fir_interp_get_backend", "if_fir_interp_set_input_format", "if_fir_interp_set_nco", "if_fir_interp_get_nco",
    "if_fir_interp_set_stream", "if_fir_interp_synchronize", "if_fir_interp_last_error", "if_fir_interp_out_count",
    "if_fir_interp_process", "if_fir_interp_process_device",
    "if_fir_resamp_init", "if_fir_resamp_init_complex", "if_fir_resamp_destroy", "if_fir_resamp_reset", "if_fir_resamp_set_input_format",
    "if_fir_resamp_set_stream", "if_fir_resamp_synchronize", "if_fir_resamp_last_error", "if_fir_resamp_out_count",
    "if_fir_resamp_process", "if_fir_resamp_process_device",
    "if_fir_psd_init", "if_fir_psd_destroy", "if_fir_psd_reset", "if_fir_psd_set_input_format", "if_fir_psd_set_stream",
    "if_fir_psd_synchronize", "if_fir_psd_last_error", "if_fir_psd_frame_count", "if_fir_psd_process", "if_fir_psd_process_device",
    "if_fir_combiner_init", "if_fir_combiner_init_complex", "if_fir_combiner_destroy", "if_fir_combiner_reset", "if_fir_combiner_set_backend",
    "if_fir_combiner_get_backend", "if_fir_combiner_set_input_format", "if_fir_combiner_set_centres", "if_fir_combiner_get_centres",
    "if_fir_combiner_set_stream", "if_fir_combiner_synchronize", "if_fir_combiner_last_error", "if_fir_combiner_out_count",
    "if_fir_combiner_process", "if_fir_combiner_process_device",
    "if_fir_ddc_init", "if_fir_ddc_init_complex", "if_fir_ddc_destroy", "if_fir_ddc_reset", "if_fir_ddc_set_input_format",
    "if_fir_ddc_set_nco", "if_fir_ddc_get_nco", "if_fir_ddc_set_stream", "if_fir_ddc_synchronize", "if_fir_ddc_last_error",
    "if_fir_ddc_out_count", "if_fir_ddc_process", "if_fir_ddc_process_device",
    "if_fir_duc_init", "if_fir_duc_init_complex", "if_fir_duc_destroy", "if_fir_duc_reset", "if_fir_duc_set_input_format",
    "if_fir_duc_set_output_format", "if_fir_duc_set_nco", "if_fir_duc_get_nco", "if_fir_duc_set_stream", "if_fir_duc_synchronize",
    "if_fir_duc_last_error", "if_fir_duc_out_count", "if_fir_duc_process", "if_fir_duc_process_device",
    "if_fir_arb_init", "if_fir_arb_destroy", "if_fir_arb_reset", "if_fir_arb_set_step", "if_fir_arb_set_input_format",
    "if_fir_arb_set_stream", "if_fir_arb_synchronize", "if_fir_arb_last_error", "if_fir_arb_out_count", "if_fir_arb_process",
    "if_fir_arb_process_device", "if_fir_arb_step_from_rates",
    "if_fir_pfb_init", "if_fir_pfb_destroy", "if_fir_pfb_reset", "if_fir_pfb_set_input_format", "if_fir_pfb_set_stream",
    "if_fir_pfb_synchronize", "if_fir_pfb_last_error", "if_fir_pfb_frame_count", "if_fir_pfb_process", "if_fir_pfb_process_device",
    "if_fir_synth_init", "if_fir_synth_destroy", "if_fir_synth_reset", "if_fir_synth_set_input_format", "if_fir_synth_set_stream",
    "if_fir_synth_synchronize", "if_fir_synth_last_error", "if_fir_synth_sample_count", "if_fir_synth_process",
    "if_fir_synth_process_device",
    "if_fir_sub_init", "if_fir_sub_destroy", "if_fir_sub_reset", "if_fir_sub_set_input_format", "if_fir_sub_set_nco", "if_fir_sub_get_nco",
    "if_fir_sub_set_stream", "if_fir_sub_synchronize", "if_fir_sub_last_error", "if_fir_sub_frame_count", "if_fir_sub_process",
    "if_fir_sub_process_device",
    "if_fir_subup_init", "if_fir_subup_destroy", "if_fir_subup_reset", "if_fir_subup_set_input_format", "if_fir_subup_set_nco",
    "if_fir_subup_get_nco", "if_fir_subup_set_stream", "if_fir_subup_synchronize", "if_fir_subup_last_error", "if_fir_subup_frame_count",
    "if_fir_subup_process", "if_fir_subup_process_device",
    "if_fir_rpfb_init", "if_fir_rpfb_destroy", "if_fir_rpfb_reset", "if_fir_rpfb_set_input_format", "if_fir_rpfb_set_stream",
    "if_fir_rpfb_synchronize", "if_fir_rpfb_last_error", "if_fir_rpfb_frame_count", "if_fir_rpfb_process", "if_fir_rpfb_process_device",
    "if_fir_rsynth_init", "if_fir_rsynth_destroy", "if_fir_rsynth_reset", "if_fir_rsynth_set_input_format", "if_fir_rsynth_set_output_format",
    "if_fir_rsynth_set_stream", "if_fir_rsynth_synchronize", "if_fir_rsynth_last_error", "if_fir_rsynth_sample_count", "if_fir_rsynth_process",
    "if_fir_rsynth_process_device",
    "if_fir_fpow_init", "if_fir_fpow_destroy", "if_fir_fpow_reset", "if_fir_fpow_set_input_format", "if_fir_fpow_set_stream",
    "if_fir_fpow_synchronize", "if_fir_fpow_last_error", "if_fir_fpow_frame_count", "if_fir_fpow_process", "if_fir_fpow_process_device",
    "if_fir_turn_init", "if_fir_turn_destroy", "if_fir_turn_set_input_format", "if_fir_turn_set_output_format", "if_fir_turn_set_stream",
    "if_fir_turn_synchronize", "if_fir_turn_last_error", "if_fir_turn_process", "if_fir_turn_process_device",
]
# every symbol include/if_fir_debug.h declares: exported by libif_fir_dev.so only
DEV_EXPORTS = ["if_fir_time_device", "if_fir_debug_stamps", "if_fir_debug_fft_tables", "if_fir_debug_fft_tables_odd", "if_fir_debug_fft_tables_bank",
               "if_fir_debug_bank_plan", "if_fir_debug_bank_tail", "if_fir_debug_fft_schedule",
               "if_fir_mc_debug_plan", "if_fir_debug_queue_faults",
               "if_fir_debug_interp_config", "if_fir_debug_interp_seek", "if_fir_debug_interp_tables", "if_fir_debug_interp_plan",
               "if_fir_debug_resamp_config", "if_fir_debug_psd_plan", "if_fir_debug_psd_config",
               "if_fir_debug_combiner_config", "if_fir_debug_combiner_seek", "if_fir_debug_combiner_tables",
               "if_fir_debug_ddc_config", "if_fir_debug_duc_config", "if_fir_debug_arb_config",
               "if_fir_debug_pfb_config", "if_fir_debug_synth_config", "if_fir_debug_synth_workspace",
               "if_fir_debug_sub_config", "if_fir_debug_subup_config", "if_fir_debug_rpfb_config",
               "if_fir_debug_rsynth_config", "if_fir_debug_rsynth_workspace", "if_fir_debug_fpow_config",
               "if_fir_debug_turn_config"]
MC_ID_BYTES = 128


class PsdConfig(ctypes.Structure):
    """if_fir_psd_config_t"""
    _fields_ = [("ulSize", ctypes.c_uint32), ("ulHop", ctypes.c_uint32), ("ulSegments", ctypes.c_uint32), ("lFirstBin", ctypes.c_int32),
                ("ulBins", ctypes.c_uint32), ("fRefPower", ctypes.c_float), ("ulInputFormat", ctypes.c_uint32)]


class PfbConfig(ctypes.Structure):
    """if_fir_pfb_config_t"""
    _fields_ = [("ulChannels", ctypes.c_uint32), ("ulHop", ctypes.c_uint32), ("lFirstBin", ctypes.c_int32), ("ulBins", ctypes.c_uint32)]


class RpfbConfig(ctypes.Structure):
    """if_fir_rpfb_config_t"""
    _fields_ = [("ulChannels", ctypes.c_uint32), ("ulHop", ctypes.c_uint32), ("ulFirstBin", ctypes.c_uint32), ("ulBins", ctypes.c_uint32)]


class RsynthConfig(ctypes.Structure):
    """if_fir_rsynth_config_t"""
    _fields_ = [("ulChannels", ctypes.c_uint32), ("ulHop", ctypes.c_uint32), ("ulFirstBin", ctypes.c_uint32), ("ulBins", ctypes.c_uint32)]


class SynthConfig(ctypes.Structure):
    """if_fir_synth_config_t"""
    _fields_ = [("ulChannels", ctypes.c_uint32), ("ulHop", ctypes.c_uint32), ("lFirstBin", ctypes.c_int32), ("ulBins", ctypes.c_uint32)]


class SubConfig(ctypes.Structure):
    """if_fir_sub_config_t"""
    _fields_ = [("ulBins", ctypes.c_uint32), ("ulTaps", ctypes.c_uint32), ("ulTapRows", ctypes.c_uint32), ("ulDecimation", ctypes.c_uint32)]


class SubUpConfig(ctypes.Structure):
    """if_fir_subup_config_t"""
    _fields_ = [("ulBins", ctypes.c_uint32), ("ulTaps", ctypes.c_uint32), ("ulTapRows", ctypes.c_uint32), ("ulInterpolation", ctypes.c_uint32)]


class FpowConfig(ctypes.Structure):
    """if_fir_fpow_config_t"""
    _fields_ = [("ulBins", ctypes.c_uint32), ("ulFirst", ctypes.c_uint32), ("ulGroup", ctypes.c_uint32), ("ulOutBins", ctypes.c_uint32),
                ("ulFrames", ctypes.c_uint32), ("fNorm", ctypes.c_float), ("fRefPower", ctypes.c_float), ("ulInputFormat", ctypes.c_uint32)]


class TurnConfig(ctypes.Structure):
    """if_fir_turn_config_t"""
    _fields_ = [("ulDirection", ctypes.c_uint32), ("ulBins", ctypes.c_uint32), ("ulChannels", ctypes.c_uint32), ("ulFirst", ctypes.c_uint32),
                ("ulInputFormat", ctypes.c_uint32), ("ulOutputFormat", ctypes.c_uint32)]


class IfFirError(RuntimeError):
    pass


_libs = {}


def lib():
    """Load libif_fir.so, the product (raises if it has not been built: there is no fallback)."""
    return _load(LIB_PATH, False)


def dev_lib():
    """Load libif_fir_dev.so: the product's code plus the development hooks of include/if_fir_debug.h."""
    return _load(DEV_LIB_PATH, True)


def _load(path, dev):
    if path in _libs:
        return _libs[path]
    if not os.path.exists(path):
        raise IfFirError("%s is not built (%s); run `python -c 'import __graft_entry__ as g; g.build()'`"
                         % (os.path.basename(path), path))
    L = ctypes.CDLL(path)
    u8, u32, u64, i32, vp = ctypes.c_uint8, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int32, ctypes.c_void_p
    f32p = ctypes.POINTER(ctypes.c_float)
    L.if_bpf_design.argtypes = [f32p, u32, ctypes.c_double, ctypes.c_double, u32]
    L.if_bpf_design.restype = u8
    L.if_fir_init.argtypes = [ctypes.POINTER(vp), f32p, u32, u32, u64, i32]
    L.if_fir_init.restype = u8
    L.if_fir_init_complex.argtypes = [ctypes.POINTER(vp), f32p, u32, u32, u64, i32]
    L.if_fir_init_complex.restype = u8
    L.if_bpf_design_complex.argtypes = [f32p, u32, ctypes.c_double, ctypes.c_double, u32]
    L.if_bpf_design_complex.restype = u8
    L.if_fir_destroy.argtypes = [vp]
    L.if_fir_destroy.restype = None
    L.if_fir_reset.argtypes = [vp]
    L.if_fir_reset.restype = u8
    L.if_fir_set_backend.argtypes = [vp, u32]
    L.if_fir_set_backend.restype = u8
    L.if_fir_get_backend.argtypes = [vp]
    L.if_fir_get_backend.restype = u32
    L.if_fir_set_input_format.argtypes = [vp, u32]
    L.if_fir_set_input_format.restype = u8
    L.if_fir_set_tuning.argtypes = [vp, u32]
    L.if_fir_set_tuning.restype = u8
    L.if_fir_set_stream.argtypes = [vp, vp]
    L.if_fir_set_stream.restype = u8
    L.if_fir_synchronize.argtypes = [vp]
    L.if_fir_synchronize.restype = u8
    L.if_fir_last_error.argtypes = [vp]
    L.if_fir_last_error.restype = ctypes.c_char_p
    L.if_fir_out_count.argtypes = [vp, u64]
    L.if_fir_out_count.restype = u64
    L.if_fir_process.argtypes = [vp, f32p, f32p, u64, ctypes.POINTER(u64)]
    L.if_fir_process.restype = u8
    L.if_fir_process_device.argtypes = [vp, vp, vp, u64, ctypes.POINTER(u64)]
    L.if_fir_process_device.restype = u8
    L.if_fir_synth_device.argtypes = [vp, vp, u64, u64, u32]
    L.if_fir_synth_device.restype = u8
    L.if_fir_dev_alloc.argtypes = [vp, ctypes.POINTER(vp), u64]
    L.if_fir_dev_alloc.restype = u8
    L.if_fir_dev_free.argtypes = [vp, vp]
    L.if_fir_dev_free.restype = u8
    L.if_fir_dev_upload.argtypes = [vp, vp, vp, u64]
    L.if_fir_dev_upload.restype = u8
    L.if_fir_dev_download.argtypes = [vp, vp, vp, u64]
    L.if_fir_dev_download.restype = u8
    L.if_fir_device_info.argtypes = [vp, ctypes.c_char_p, u32]
    L.if_fir_device_info.restype = u8
    L.if_fir_set_nco.argtypes = [vp, ctypes.c_double]
    L.if_fir_set_nco.restype = u8
    L.if_fir_get_nco.argtypes = [vp, ctypes.POINTER(ctypes.c_double)]
    L.if_fir_get_nco.restype = u8
    L.if_fir_channelizer_process_device.argtypes = [vp, u32, ctypes.POINTER(u32), vp, ctypes.POINTER(vp), u64,
                                                    ctypes.POINTER(u64)]
    L.if_fir_channelizer_process_device.restype = u8
    L.if_fir_channelizer_process_device_freq.argtypes = [vp, u32, ctypes.POINTER(ctypes.c_double), vp, ctypes.POINTER(vp), u64,
                                                         ctypes.POINTER(u64)]
    L.if_fir_channelizer_process_device_freq.restype = u8
    L.if_fir_host_alloc.argtypes = [vp, ctypes.POINTER(vp), u64]
    L.if_fir_host_alloc.restype = u8
    L.if_fir_host_free.argtypes = [vp, vp]
    L.if_fir_host_free.restype = u8
    L.if_fir_power_device.argtypes = [vp, vp, u64, ctypes.POINTER(ctypes.c_double)]
    L.if_fir_power_device.restype = u8
    u8p = ctypes.POINTER(ctypes.c_uint8)
    L.if_fir_mc_owner.argtypes = [u32, u32]
    L.if_fir_mc_owner.restype = u32
    L.if_fir_mc_unique_id.argtypes = [u8p]
    L.if_fir_mc_unique_id.restype = u8
    L.if_fir_mc_init.argtypes = [ctypes.POINTER(vp), u32, f32p, u32, u32, u64, i32, u32, u32, u8p]
    L.if_fir_mc_init.restype = u8
    L.if_fir_mc_destroy.argtypes = [vp]
    L.if_fir_mc_destroy.restype = None
    L.if_fir_mc_reset.argtypes = [vp]
    L.if_fir_mc_reset.restype = u8
    L.if_fir_mc_set_input_format.argtypes = [vp, u32]
    L.if_fir_mc_set_input_format.restype = u8
    L.if_fir_mc_process_device.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(vp), u64, ctypes.POINTER(u64)]
    L.if_fir_mc_process_device.restype = u8
    L.if_fir_mc_channel_ctx.argtypes = [vp, u32]
    L.if_fir_mc_channel_ctx.restype = vp
    L.if_fir_mc_last_error.argtypes = [vp]
    L.if_fir_mc_last_error.restype = ctypes.c_char_p
    L.if_fir_mc_set_chunk_samples.argtypes = [vp, u64]
    L.if_fir_mc_set_chunk_samples.restype = u8
    L.if_fir_mc_get_chunk_samples.argtypes = [vp, ctypes.POINTER(u64), ctypes.POINTER(u64)]
    L.if_fir_mc_get_chunk_samples.restype = u8
    # the streaming contexts (_StreamCtx): what the families declare alike, then what each has of its own
    for prefix in ("if_fir_interp_", "if_fir_resamp_", "if_fir_psd_", "if_fir_combiner_", "if_fir_ddc_", "if_fir_duc_", "if_fir_arb_",
                   "if_fir_pfb_", "if_fir_synth_", "if_fir_sub_", "if_fir_subup_", "if_fir_rpfb_", "if_fir_rsynth_", "if_fir_fpow_"):
        for name, args, res in (("destroy", [vp], None), ("reset", [vp], u8), ("synchronize", [vp], u8), ("set_input_format", [vp, u32], u8),
                                ("set_stream", [vp, vp], u8), ("last_error", [vp], ctypes.c_char_p)):
            getattr(L, prefix + name).argtypes = args
            getattr(L, prefix + name).restype = res
    for prefix, init_args in (("if_fir_interp_", [ctypes.POINTER(vp), f32p, u32, u32, u64, i32]),
                              ("if_fir_resamp_", [ctypes.POINTER(vp), f32p, u32, u32, u32, u64, i32]),
                              ("if_fir_ddc_", [ctypes.POINTER(vp), f32p, u32, u32, u64, i32])):
        for name, args, res in (("init", init_args, u8), ("init_complex", init_args, u8), ("out_count", [vp, u64], u64),
                                ("process", [vp, vp, f32p, u64, ctypes.POINTER(u64)], u8),
                                ("process_device", [vp, vp, vp, u64, ctypes.POINTER(u64)], u8)):
            getattr(L, prefix + name).argtypes = args
            getattr(L, prefix + name).restype = res
    L.if_fir_interp_set_backend.argtypes = [vp, u32]
    L.if_fir_interp_set_backend.restype = u8
    L.if_fir_interp_get_backend.argtypes = [vp]
    L.if_fir_interp_get_backend.restype = u32
    L.if_fir_interp_set_nco.argtypes = [vp, ctypes.c_double]
    L.if_fir_interp_set_nco.restype = u8
    L.if_fir_interp_get_nco.argtypes = [vp, ctypes.POINTER(ctypes.c_double)]
    L.if_fir_interp_get_nco.restype = u8
    L.if_fir_ddc_set_nco.argtypes = [vp, ctypes.c_double]
    L.if_fir_ddc_set_nco.restype = u8
    L.if_fir_ddc_get_nco.argtypes = [vp, ctypes.POINTER(ctypes.c_double)]
    L.if_fir_ddc_get_nco.restype = u8
    for name, args, res in (("init", [ctypes.POINTER(vp), f32p, u32, u32, u64, i32], u8),
                            ("init_complex", [ctypes.POINTER(vp), f32p, u32, u32, u64, i32], u8), ("out_count", [vp, u64], u64),
                            ("process", [vp, vp, vp, u64, ctypes.POINTER(u64)], u8),
                            ("process_device", [vp, vp, vp, u64, ctypes.POINTER(u64)], u8), ("set_output_format", [vp, u32], u8),
                            ("set_nco", [vp, ctypes.c_double], u8), ("get_nco", [vp, ctypes.POINTER(ctypes.c_double)], u8)):
        getattr(L, "if_fir_duc_" + name).argtypes = args
        getattr(L, "if_fir_duc_" + name).restype = res
    for name, args, res in (("init", [ctypes.POINTER(vp), f32p, u32, u32, u64, u64, i32], u8), ("set_step", [vp, u64], u8),
                            ("out_count", [vp, u64], u64), ("process", [vp, vp, f32p, u64, ctypes.POINTER(u64)], u8),
                            ("process_device", [vp, vp, vp, u64, ctypes.POINTER(u64)], u8),
                            ("step_from_rates", [ctypes.c_double, ctypes.c_double], u64)):
        getattr(L, "if_fir_arb_" + name).argtypes = args
        getattr(L, "if_fir_arb_" + name).restype = res
    f64p = ctypes.POINTER(ctypes.c_double)
    for name in ("init", "init_complex"):
        getattr(L, "if_fir_combiner_" + name).argtypes = [ctypes.POINTER(vp), f32p, u32, u32, u32, f64p, u64, i32]
        getattr(L, "if_fir_combiner_" + name).restype = u8
    L.if_fir_combiner_set_backend.argtypes = [vp, u32]
    L.if_fir_combiner_set_backend.restype = u8
    L.if_fir_combiner_get_backend.argtypes = [vp]
    L.if_fir_combiner_get_backend.restype = u32
    L.if_fir_combiner_set_centres.argtypes = [vp, f64p]
    L.if_fir_combiner_set_centres.restype = u8
    L.if_fir_combiner_get_centres.argtypes = [vp, f64p]
    L.if_fir_combiner_get_centres.restype = u8
    L.if_fir_combiner_out_count.argtypes = [vp, u64]
    L.if_fir_combiner_out_count.restype = u64
    L.if_fir_combiner_process.argtypes = [vp, ctypes.POINTER(vp), f32p, u64, ctypes.POINTER(u64)]
    L.if_fir_combiner_process.restype = u8
    L.if_fir_combiner_process_device.argtypes = [vp, ctypes.POINTER(vp), vp, u64, ctypes.POINTER(u64)]
    L.if_fir_combiner_process_device.restype = u8
    u16p = ctypes.POINTER(ctypes.c_uint16)
    L.if_fir_psd_init.argtypes = [ctypes.POINTER(vp), ctypes.POINTER(PsdConfig), f32p, u64, i32]
    L.if_fir_psd_init.restype = u8
    L.if_fir_psd_frame_count.argtypes = [vp, u64]
    L.if_fir_psd_frame_count.restype = u64
    L.if_fir_psd_process.argtypes = [vp, vp, u64, u16p, f32p, ctypes.POINTER(u32)]
    L.if_fir_psd_process.restype = u8
    L.if_fir_psd_process_device.argtypes = [vp, vp, u64, vp, vp, ctypes.POINTER(u32)]
    L.if_fir_psd_process_device.restype = u8
    L.if_fir_pfb_init.argtypes = [ctypes.POINTER(vp), ctypes.POINTER(PfbConfig), f32p, u32, u64, i32]
    L.if_fir_pfb_init.restype = u8
    L.if_fir_pfb_frame_count.argtypes = [vp, u64]
    L.if_fir_pfb_frame_count.restype = u64
    L.if_fir_pfb_process.argtypes = [vp, vp, f32p, u64, ctypes.POINTER(u64)]
    L.if_fir_pfb_process.restype = u8
    L.if_fir_pfb_process_device.argtypes = [vp, vp, vp, u64, ctypes.POINTER(u64)]
    L.if_fir_pfb_process_device.restype = u8
    L.if_fir_synth_init.argtypes = [ctypes.POINTER(vp), ctypes.POINTER(SynthConfig), f32p, u32, u64, i32]
    L.if_fir_synth_init.restype = u8
    L.if_fir_synth_sample_count.argtypes = [vp, u64]
    L.if_fir_synth_sample_count.restype = u64
    L.if_fir_synth_process.argtypes = [vp, vp, f32p, u64, ctypes.POINTER(u64)]
    L.if_fir_synth_process.restype = u8
    L.if_fir_synth_process_device.argtypes = [vp, vp, vp, u64, ctypes.POINTER(u64)]
    L.if_fir_synth_process_device.restype = u8
    L.if_fir_fpow_init.argtypes = [ctypes.POINTER(vp), ctypes.POINTER(FpowConfig), u64, i32]
    L.if_fir_fpow_init.restype = u8
    L.if_fir_fpow_frame_count.argtypes = [vp, u64]
    L.if_fir_fpow_frame_count.restype = u64
    L.if_fir_fpow_process.argtypes = [vp, vp, u64, u16p, f32p, ctypes.POINTER(u32)]
    L.if_fir_fpow_process.restype = u8
    L.if_fir_fpow_process_device.argtypes = [vp, vp, u64, vp, vp, ctypes.POINTER(u32)]
    L.if_fir_fpow_process_device.restype = u8
    if dev:
        L.if_fir_debug_fpow_config.argtypes = [vp, u32, u64]
        L.if_fir_debug_fpow_config.restype = u8
    # the corner turn carries no state: the common calls but no reset
    for name, args, res in (("destroy", [vp], None), ("synchronize", [vp], u8), ("set_input_format", [vp, u32], u8),
                            ("set_output_format", [vp, u32], u8), ("set_stream", [vp, vp], u8), ("last_error", [vp], ctypes.c_char_p),
                            ("init", [ctypes.POINTER(vp), ctypes.POINTER(TurnConfig), ctypes.POINTER(u32), u64, i32], u8),
                            ("process", [vp, vp, vp, u64, u64], u8), ("process_device", [vp, vp, vp, u64, u64], u8)):
        getattr(L, "if_fir_turn_" + name).argtypes = args
        getattr(L, "if_fir_turn_" + name).restype = res
    if dev:
        L.if_fir_debug_turn_config.argtypes = [vp, u32]
        L.if_fir_debug_turn_config.restype = u8
    L.if_fir_sub_init.argtypes = [ctypes.POINTER(vp), ctypes.POINTER(SubConfig), f32p, u64, i32]
    L.if_fir_sub_init.restype = u8
    L.if_fir_sub_set_nco.argtypes = [vp, f64p]
    L.if_fir_sub_set_nco.restype = u8
    L.if_fir_sub_get_nco.argtypes = [vp, f64p]
    L.if_fir_sub_get_nco.restype = u8
    L.if_fir_sub_frame_count.argtypes = [vp, u64]
    L.if_fir_sub_frame_count.restype = u64
    L.if_fir_sub_process.argtypes = [vp, vp, f32p, u64, ctypes.POINTER(u64)]
    L.if_fir_sub_process.restype = u8
    L.if_fir_sub_process_device.argtypes = [vp, vp, vp, u64, ctypes.POINTER(u64)]
    L.if_fir_sub_process_device.restype = u8
    if dev:
        L.if_fir_debug_sub_config.argtypes = [vp, u32, ctypes.POINTER(u32), u64]
        L.if_fir_debug_sub_config.restype = u8
    L.if_fir_subup_init.argtypes = [ctypes.POINTER(vp), ctypes.POINTER(SubUpConfig), f32p, u64, i32]
    L.if_fir_subup_init.restype = u8
    L.if_fir_subup_set_nco.argtypes = [vp, f64p]
    L.if_fir_subup_set_nco.restype = u8
    L.if_fir_subup_get_nco.argtypes = [vp, f64p]
    L.if_fir_subup_get_nco.restype = u8
    L.if_fir_subup_frame_count.argtypes = [vp, u64]
    L.if_fir_subup_frame_count.restype = u64
    L.if_fir_subup_process.argtypes = [vp, vp, f32p, u64, ctypes.POINTER(u64)]
    L.if_fir_subup_process.restype = u8
    L.if_fir_subup_process_device.argtypes = [vp, vp, vp, u64, ctypes.POINTER(u64)]
    L.if_fir_subup_process_device.restype = u8
    L.if_fir_rpfb_init.argtypes = [ctypes.POINTER(vp), ctypes.POINTER(RpfbConfig), f32p, u32, u64, i32]
    L.if_fir_rpfb_init.restype = u8
    L.if_fir_rpfb_frame_count.argtypes = [vp, u64]
    L.if_fir_rpfb_frame_count.restype = u64
    L.if_fir_rpfb_process.argtypes = [vp, vp, f32p, u64, ctypes.POINTER(u64)]
    L.if_fir_rpfb_process.restype = u8
    L.if_fir_rpfb_process_device.argtypes = [vp, vp, vp, u64, ctypes.POINTER(u64)]
    L.if_fir_rpfb_process_device.restype = u8
    L.if_fir_rsynth_init.argtypes = [ctypes.POINTER(vp), ctypes.POINTER(RsynthConfig), f32p, u32, u64, i32]
    L.if_fir_rsynth_init.restype = u8
    L.if_fir_rsynth_set_output_format.argtypes = [vp, u32]
    L.if_fir_rsynth_set_output_format.restype = u8
    L.if_fir_rsynth_sample_count.argtypes = [vp, u64]
    L.if_fir_rsynth_sample_count.restype = u64
    L.if_fir_rsynth_process.argtypes = [vp, vp, vp, u64, ctypes.POINTER(u64)]
    L.if_fir_rsynth_process.restype = u8
    L.if_fir_rsynth_process_device.argtypes = [vp, vp, vp, u64, ctypes.POINTER(u64)]
    L.if_fir_rsynth_process_device.restype = u8
    if dev:
        L.if_fir_debug_rsynth_config.argtypes = [vp, u32, u64]
        L.if_fir_debug_rsynth_config.restype = u8
        L.if_fir_debug_rsynth_workspace.argtypes = [vp, u64, ctypes.POINTER(u64)]
        L.if_fir_debug_rsynth_workspace.restype = u8
        L.if_fir_debug_rpfb_config.argtypes = [vp, u32, ctypes.POINTER(u32), u64]
        L.if_fir_debug_rpfb_config.restype = u8
        L.if_fir_debug_subup_config.argtypes = [vp, u32, ctypes.POINTER(u32), u64]
        L.if_fir_debug_subup_config.restype = u8
        L.if_fir_debug_synth_config.argtypes = [vp, u32, u32, ctypes.POINTER(u32), u64]
        L.if_fir_debug_synth_config.restype = u8
        L.if_fir_debug_synth_workspace.argtypes = [vp, u64, ctypes.POINTER(u64)]
        L.if_fir_debug_synth_workspace.restype = u8
        L.if_fir_debug_pfb_config.argtypes = [vp, u32, ctypes.POINTER(u32), u64]
        L.if_fir_debug_pfb_config.restype = u8
        L.if_fir_debug_combiner_config.argtypes = [vp, u32]
        L.if_fir_debug_combiner_config.restype = u8
        L.if_fir_debug_combiner_seek.argtypes = [vp, u64]
        L.if_fir_debug_combiner_seek.restype = u8
        L.if_fir_debug_combiner_tables.argtypes = [f32p, u32, u32, ctypes.c_double, ctypes.POINTER(u32), ctypes.POINTER(i32), f32p, u32]
        L.if_fir_debug_combiner_tables.restype = u32
        L.if_fir_debug_psd_plan.argtypes = [vp, u64, ctypes.POINTER(u64)]
        L.if_fir_debug_psd_plan.restype = u8
        L.if_fir_debug_psd_config.argtypes = [vp, u32, u64]
        L.if_fir_debug_psd_config.restype = u8
        L.if_fir_debug_resamp_config.argtypes = [vp, u32, ctypes.POINTER(u32)]
        L.if_fir_debug_resamp_config.restype = u8
        L.if_fir_debug_ddc_config.argtypes = [vp, u32, ctypes.POINTER(u32), u64]
        L.if_fir_debug_ddc_config.restype = u8
        L.if_fir_debug_duc_config.argtypes = [vp, u32, ctypes.POINTER(u32), u64]
        L.if_fir_debug_duc_config.restype = u8
        L.if_fir_debug_arb_config.argtypes = [vp, u32, ctypes.POINTER(u32), u64, u64]
        L.if_fir_debug_arb_config.restype = u8
        L.if_fir_debug_interp_config.argtypes = [vp, u32, u32]
        L.if_fir_debug_interp_config.restype = u8
        L.if_fir_debug_interp_seek.argtypes = [vp, u64]
        L.if_fir_debug_interp_seek.restype = u8
        L.if_fir_debug_interp_tables.argtypes = [f32p, u32, u32, f32p, u32]
        L.if_fir_debug_interp_tables.restype = u32
        L.if_fir_debug_interp_plan.argtypes = [u32, u32, ctypes.POINTER(u32), ctypes.POINTER(u32), ctypes.POINTER(u32)]
        L.if_fir_debug_interp_plan.restype = u8
        L.if_fir_time_device.argtypes = [vp, vp, vp, u64, u32, u32, f32p]
        L.if_fir_time_device.restype = u8
        L.if_fir_debug_stamps.argtypes = [vp, ctypes.POINTER(u64), u32]
        L.if_fir_debug_stamps.restype = u32
        L.if_fir_debug_fft_tables.argtypes = [f32p, u32, u32, u32, u32, f32p, u32]
        L.if_fir_debug_fft_tables.restype = u32
        L.if_fir_debug_fft_schedule.argtypes = [u64, u32, u32, ctypes.POINTER(ctypes.c_int64)]
        L.if_fir_debug_fft_schedule.restype = u8
        L.if_fir_mc_debug_plan.argtypes = [u32, u32, u32, u64, u32, u32, u32, u64, u64, ctypes.POINTER(u64), u32]
        L.if_fir_mc_debug_plan.restype = u32
        L.if_fir_debug_queue_faults.argtypes = [vp, ctypes.POINTER(u32)]
        L.if_fir_debug_queue_faults.restype = u8
    _libs[path] = L
    return L


def _f32p(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def _taps_arg(taps, complex_taps):
    """(contiguous float32 array -- complex taps interleaved (re, im) --, tap count, complex flag) of a constructor's taps"""
    taps = np.asarray(taps)
    if np.iscomplexobj(taps):
        taps = np.ascontiguousarray(taps.astype(np.complex64)).view(np.float32)
        complex_taps = True
    taps = np.ascontiguousarray(taps, dtype=np.float32)
    return taps, (taps.size // 2 if complex_taps else taps.size), bool(complex_taps)


def bpf_design(taps, f_low=0.15, f_high=0.25, window=WINDOW_BLACKMAN):
    """if_bpf_design(): windowed-sinc band-pass taps (float32)."""
    h = np.zeros(max(int(taps), 0), dtype=np.float32)
    if not lib().if_bpf_design(_f32p(h), int(taps), float(f_low), float(f_high), int(window)):
        raise IfFirError("if_bpf_design rejected taps=%r band=[%r,%r] window=%r" % (taps, f_low, f_high, window))
    return h


def bpf_design_complex(taps, centre=0.2, bandwidth=0.1, window=WINDOW_BLACKMAN):
    """if_bpf_design_complex(): channel-selection taps, interleaved (re, im) float32."""
    g = np.zeros(2 * max(int(taps), 0), dtype=np.float32)
    if not lib().if_bpf_design_complex(_f32p(g), int(taps), float(centre), float(bandwidth), int(window)):
        raise IfFirError("if_bpf_design_complex rejected taps=%r centre=%r bandwidth=%r" % (taps, centre, bandwidth))
    return g


class IfFir:
    """One if_fir_ctx_t.  Methods mirror the C entry points."""

    def __init__(self, taps, decimation=1, max_samples=1 << 20, device=0, backend=None, complex_taps=False, dev=False,
                 lib_path=None):
        # lib_path (development tools only, tools/ab_inproc.py): another build of the development library, loaded beside the
        # default one so that two builds can be timed alternately in one process
        self._L = _load(os.path.abspath(lib_path), True) if lib_path else dev_lib() if dev else lib()
        taps, count, complex_taps = _taps_arg(taps, complex_taps)
        self._ctx = ctypes.c_void_p()
        self.taps = taps
        self.decimation = int(decimation)
        init = self._L.if_fir_init_complex if complex_taps else self._L.if_fir_init
        if not init(ctypes.byref(self._ctx), _f32p(taps), count, self.decimation, int(max_samples), int(device)):
            self._ctx = ctypes.c_void_p()
            raise IfFirError(self._L.if_fir_last_error(None).decode())
        if backend is not None:
            self.set_backend(backend)

    def _check(self, ok):
        if not ok:
            raise IfFirError(self._L.if_fir_last_error(self._ctx).decode())

    def close(self):
        if self._ctx:
            self._L.if_fir_destroy(self._ctx)
            self._ctx = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def reset(self):
        self._check(self._L.if_fir_reset(self._ctx))

    def set_backend(self, backend):
        self._check(self._L.if_fir_set_backend(self._ctx, int(backend)))

    def get_backend(self):
        return int(self._L.if_fir_get_backend(self._ctx))

    def set_input_format(self, fmt):
        self._check(self._L.if_fir_set_input_format(self._ctx, int(fmt)))
        self._i16 = (int(fmt) == INPUT_I16)

    def set_nco(self, freq):
        """if_fir_set_nco(): mix the input with exp(-j 2 pi f a) ahead of the filter (SPEC §3.2); 0 = off."""
        self._check(self._L.if_fir_set_nco(self._ctx, float(freq)))

    def get_nco(self):
        f = ctypes.c_double(0.0)
        self._check(self._L.if_fir_get_nco(self._ctx, ctypes.byref(f)))
        return float(f.value)

    def power_device(self, dev_iq, samples):
        """if_fir_power_device(): mean(|y|^2) of a device IQ buffer."""
        p = ctypes.c_double(0.0)
        self._check(self._L.if_fir_power_device(self._ctx, ctypes.c_void_p(int(dev_iq)), int(samples), ctypes.byref(p)))
        return float(p.value)

    def host_alloc(self, count, dtype=np.float32):
        """if_fir_host_alloc(): a page-locked numpy array of `count` elements (free it with host_free(array))."""
        dtype = np.dtype(dtype)
        p = ctypes.c_void_p(None)
        self._check(self._L.if_fir_host_alloc(self._ctx, ctypes.byref(p), int(count) * dtype.itemsize))
        buf = (ctypes.c_char * (int(count) * dtype.itemsize)).from_address(p.value)
        arr = np.frombuffer(buf, dtype=dtype, count=int(count))
        self._pinned = getattr(self, "_pinned", {})
        self._pinned[arr.ctypes.data] = p.value
        return arr

    def host_free(self, arr):
        p = self._pinned.pop(arr.ctypes.data)
        self._check(self._L.if_fir_host_free(self._ctx, ctypes.c_void_p(p)))

    def process_into(self, iq, out):
        """if_fir_process() with caller-provided host arrays (e.g. from host_alloc); returns the output sample count."""
        n = iq.size // 2
        m = ctypes.c_uint64(0)
        self._check(self._L.if_fir_process(self._ctx, ctypes.cast(iq.ctypes.data, ctypes.POINTER(ctypes.c_float)),
                                         _f32p(out), n, ctypes.byref(m)))
        return int(m.value)

    def channelizer_process_device_freq(self, centres, dev_in, dev_outs, samples):
        """if_fir_channelizer_process_device_freq(): channel c centred at centres[c] cycles/sample (decimation 4, 8, 12, ..., 64)."""
        k = len(centres)
        fc = (ctypes.c_double * k)(*[float(v) for v in centres])
        po = (ctypes.c_void_p * k)(*[ctypes.c_void_p(int(p)) for p in dev_outs])
        m = ctypes.c_uint64(0)
        self._check(self._L.if_fir_channelizer_process_device_freq(self._ctx, k, fc, ctypes.c_void_p(int(dev_in)), po,
                                                                   int(samples), ctypes.byref(m)))
        return int(m.value)

    def channelizer_process_device(self, slots, dev_in, dev_outs, samples):
        """if_fir_channelizer_process_device(): uniform filter bank, channel c mixed down by slots[c]/16."""
        k = len(slots)
        sl = (ctypes.c_uint32 * k)(*[int(v) for v in slots])
        po = (ctypes.c_void_p * k)(*[ctypes.c_void_p(int(p)) for p in dev_outs])
        m = ctypes.c_uint64(0)
        self._check(self._L.if_fir_channelizer_process_device(self._ctx, k, sl, ctypes.c_void_p(int(dev_in)), po,
                                                            int(samples), ctypes.byref(m)))
        return int(m.value)

    def set_tuning(self, variant):
        self._check(self._L.if_fir_set_tuning(self._ctx, int(variant)))

    def set_stream(self, stream_handle):
        self._check(self._L.if_fir_set_stream(self._ctx, ctypes.c_void_p(stream_handle or None)))

    def synchronize(self):
        self._check(self._L.if_fir_synchronize(self._ctx))

    def out_count(self, samples):
        return int(self._L.if_fir_out_count(self._ctx, int(samples)))

    def device_info(self):
        buf = ctypes.create_string_buffer(256)
        self._check(self._L.if_fir_device_info(self._ctx, buf, 256))
        return buf.value.decode()

    def process(self, iq):
        """if_fir_process(): host interleaved float32 (or complex64) in, interleaved float32 out."""
        iq = np.asarray(iq)
        if getattr(self, "_i16", False):
            iq = np.ascontiguousarray(iq, dtype=np.int16).reshape(-1)
        else:
            if np.iscomplexobj(iq):
                iq = np.ascontiguousarray(iq.astype(np.complex64)).view(np.float32)
            iq = np.ascontiguousarray(iq, dtype=np.float32).reshape(-1)
        n = iq.size // 2
        out = np.empty(2 * self.out_count(n), dtype=np.float32)
        m = ctypes.c_uint64(0)
        dummy = np.zeros(2, dtype=np.float32)
        src = iq if n else dummy
        self._check(self._L.if_fir_process(self._ctx, ctypes.cast(src.ctypes.data, ctypes.POINTER(ctypes.c_float)),
                                         _f32p(out if out.size else dummy), n, ctypes.byref(m)))
        assert m.value * 2 == out.size
        return out

    def process_device(self, dev_in, dev_out, samples):
        """if_fir_process_device(): raw device pointers (ints), asynchronous. Returns the output sample count."""
        m = ctypes.c_uint64(0)
        self._check(self._L.if_fir_process_device(self._ctx, ctypes.c_void_p(dev_in), ctypes.c_void_p(dev_out),
                                                int(samples), ctypes.byref(m)))
        return int(m.value)

    def synth_device(self, dev_iq, first, samples, channel=0):
        self._check(self._L.if_fir_synth_device(self._ctx, ctypes.c_void_p(dev_iq), int(first), int(samples),
                                              int(channel)))

    def time_device(self, dev_in, dev_out, samples, warmup=3, reps=10):
        """if_fir_time_device() (development library: construct with dev=True)."""
        ms = ctypes.c_float(0)
        self._check(self._L.if_fir_time_device(self._ctx, ctypes.c_void_p(dev_in), ctypes.c_void_p(dev_out),
                                             int(samples), int(warmup), int(reps), ctypes.byref(ms)))
        return float(ms.value)

    def debug_queue_faults(self):
        """if_fir_debug_queue_faults() (development library): expired bounded waits of the block queue, 0 when healthy."""
        n = ctypes.c_uint32(0)
        self._check(self._L.if_fir_debug_queue_faults(self._ctx, ctypes.byref(n)))
        return int(n.value)

    def debug_stamps(self, waves=None):
        """Arm (waves=None) or fetch the per-wave diagnostic stamps of the last persistent-kernel launch."""
        if waves is None:
            self._L.if_fir_debug_stamps(self._ctx, None, 0)
            return None
        buf = np.zeros(4 * waves, dtype=np.uint64)
        n = self._L.if_fir_debug_stamps(self._ctx, buf.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), buf.size)
        return buf[:n].reshape(-1, 4)

    # device memory helpers (pure C hosts use these instead of HIP headers)
    def dev_alloc(self, nbytes):
        p = ctypes.c_void_p()
        self._check(self._L.if_fir_dev_alloc(self._ctx, ctypes.byref(p), int(nbytes)))
        return p.value

    def dev_free(self, ptr):
        self._check(self._L.if_fir_dev_free(self._ctx, ctypes.c_void_p(ptr)))

    def dev_upload(self, ptr, host):
        host = np.ascontiguousarray(host)
        self._check(self._L.if_fir_dev_upload(self._ctx, ctypes.c_void_p(ptr), host.ctypes.data_as(ctypes.c_void_p),
                                            host.nbytes))

    def dev_download(self, ptr, nbytes, dtype=np.float32):
        host = np.empty(nbytes // np.dtype(dtype).itemsize, dtype=dtype)
        self._check(self._L.if_fir_dev_download(self._ctx, host.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(ptr),
                                              host.nbytes))
        return host


class _StreamCtx:
    """What IfFirInterp, IfFirResamp, IfFirPsd, IfFirCombiner, IfFirDdc, IfFirDuc, IfFirArb, IfFirPfb, IfFirSynth, IfFirSub, IfFirSubUp, IfFirRpfb, IfFirRsynth, IfFirFpow and IfFirTurn share (csrc/if_fir_stream_ctx.h is the C side of it): the context's lifetime, the
    calls the fifteen families have under one name, and the host array a process() sends.  A subclass sets _PREFIX and, in its
    __init__, self._L, self._ctx and self._i16."""
    _PREFIX = None   # the family's C name prefix: "if_fir_interp_" and so on

    def _c(self, name):
        return getattr(self._L, self._PREFIX + name)

    def _check(self, ok):
        if not ok:
            raise IfFirError(self._c("last_error")(self._ctx).decode())

    def close(self):
        if self._ctx:
            self._c("destroy")(self._ctx)
            self._ctx = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def reset(self):
        self._check(self._c("reset")(self._ctx))

    def set_input_format(self, fmt):
        self._check(self._c("set_input_format")(self._ctx, int(fmt)))
        self._i16 = (int(fmt) == INPUT_I16)

    def set_stream(self, stream_handle):
        self._check(self._c("set_stream")(self._ctx, ctypes.c_void_p(stream_handle or None)))

    def synchronize(self):
        self._check(self._c("synchronize")(self._ctx))

    def _host_input(self, iq):
        """(contiguous interleaved float32 -- or int16 after set_input_format(INPUT_I16) -- array, sample count) of a host array"""
        iq = np.asarray(iq)
        if self._i16:
            iq = np.ascontiguousarray(iq, dtype=np.int16).reshape(-1)
        else:
            if np.iscomplexobj(iq):
                iq = np.ascontiguousarray(iq.astype(np.complex64)).view(np.float32)
            iq = np.ascontiguousarray(iq, dtype=np.float32).reshape(-1)
        return iq, iq.size // 2

    def _process(self, iq):
        """<prefix>process() of a family with one input and one output stream: host array in, interleaved float32 out"""
        iq, n = self._host_input(iq)
        out = np.empty(2 * self.out_count(n), dtype=np.float32)
        m = ctypes.c_uint64(0)
        dummy = np.zeros(2, dtype=np.float32)
        self._check(self._c("process")(self._ctx, ctypes.c_void_p(iq.ctypes.data if n else dummy.ctypes.data),
                                       _f32p(out if out.size else dummy), n, ctypes.byref(m)))
        assert m.value * 2 == out.size
        return out

    def _process_device(self, dev_in, dev_out, samples):
        """<prefix>process_device() of such a family: raw device pointers (ints), asynchronous; the output sample count"""
        m = ctypes.c_uint64(0)
        self._check(self._c("process_device")(self._ctx, ctypes.c_void_p(dev_in), ctypes.c_void_p(dev_out), int(samples),
                                              ctypes.byref(m)))
        return int(m.value)


class IfFirInterp(_StreamCtx):
    """One if_fir_interp_t: upsample by `interpolation`, filter, optionally mix up (docs/SPEC.md §6).  Methods mirror the C
    entry points; N input samples give N * interpolation outputs."""
    _PREFIX = "if_fir_interp_"

    def __init__(self, taps, interpolation, max_samples=1 << 20, device=0, backend=None, complex_taps=False, dev=False):
        self._L = dev_lib() if dev else lib()
        taps, count, complex_taps = _taps_arg(taps, complex_taps)
        self._ctx = ctypes.c_void_p()
        self.taps = taps
        self.interpolation = int(interpolation)
        self._i16 = False
        init = self._L.if_fir_interp_init_complex if complex_taps else self._L.if_fir_interp_init
        if not init(ctypes.byref(self._ctx), _f32p(taps), count, self.interpolation,
                    int(max_samples), int(device)):
            self._ctx = ctypes.c_void_p()
            raise IfFirError(self._c("last_error")(None).decode())
        if backend is not None:
            self.set_backend(backend)

    def set_backend(self, backend):
        self._check(self._L.if_fir_interp_set_backend(self._ctx, int(backend)))

    def get_backend(self):
        return int(self._L.if_fir_interp_get_backend(self._ctx))

    def set_nco(self, freq):
        """if_fir_interp_set_nco(): mix the OUTPUT up by exp(+j 2 pi f n), n = absolute output index; 0 = off."""
        self._check(self._L.if_fir_interp_set_nco(self._ctx, float(freq)))

    def get_nco(self):
        f = ctypes.c_double(0.0)
        self._check(self._L.if_fir_interp_get_nco(self._ctx, ctypes.byref(f)))
        return float(f.value)

    def out_count(self, samples):
        return int(self._L.if_fir_interp_out_count(self._ctx, int(samples)))

    def process(self, iq):
        """if_fir_interp_process(): host interleaved float32 / complex64 (or int16 pairs after set_input_format(INPUT_I16)) in,
        interleaved float32 out."""
        return self._process(iq)

    def process_device(self, dev_in, dev_out, samples):
        """if_fir_interp_process_device(): raw device pointers (ints), asynchronous.  Returns the output sample count."""
        return self._process_device(dev_in, dev_out, samples)

    def debug_config(self, force_full=False, grid_limit=0):
        """if_fir_debug_interp_config() (development library: construct with dev=True)."""
        self._check(self._L.if_fir_debug_interp_config(self._ctx, 1 if force_full else 0, int(grid_limit)))

    def debug_seek(self, samples):
        """if_fir_debug_interp_seek() (development library): the next call's first output index becomes samples * L."""
        self._check(self._L.if_fir_debug_interp_seek(self._ctx, int(samples)))


def debug_interp_tables(taps, complex_taps=False):
    """if_fir_debug_interp_tables(): the interpolator's multiply table FFT_4096(taps) / 4096 as complex64 (host-only, no GPU)."""
    taps = np.ascontiguousarray(taps, dtype=np.float32)
    t = taps.size // 2 if complex_taps else taps.size
    out = np.zeros(2 * 4096, dtype=np.float32)
    if dev_lib().if_fir_debug_interp_tables(_f32p(taps), t, 1 if complex_taps else 0, _f32p(out), out.size) != out.size:
        raise IfFirError("if_fir_debug_interp_tables: %d taps are not served by the overlap-save kernel" % t)
    return out.view(np.complex64)


def debug_interp_plan(taps, interpolation):
    """if_fir_debug_interp_plan(): (overlap rows, history length in input samples, overlap-save backend serves the pair) for a
    tap count and an interpolation (host-only, no GPU)."""
    rows, hist, ok = ctypes.c_uint32(0), ctypes.c_uint32(0), ctypes.c_uint32(0)
    if not dev_lib().if_fir_debug_interp_plan(int(taps), int(interpolation), ctypes.byref(rows), ctypes.byref(hist), ctypes.byref(ok)):
        raise IfFirError("if_fir_debug_interp_plan: %d taps, interpolation %d are outside if_fir_interp_init's range"
                         % (int(taps), int(interpolation)))
    return int(rows.value), int(hist.value), bool(ok.value)


class IfFirCombiner(_StreamCtx):
    """One if_fir_combiner_t: C baseband streams, each interpolated by `interpolation` with one prototype filter and mixed up to
    its own centre, summed into one stream in one pass (docs/SPEC.md §9).  Methods mirror the C entry points; N input samples per
    channel give N * interpolation outputs."""
    _PREFIX = "if_fir_combiner_"

    def __init__(self, taps, interpolation, centres, max_samples=1 << 20, device=0, backend=None, complex_taps=False, dev=False):
        self._L = dev_lib() if dev else lib()
        taps, count, complex_taps = _taps_arg(taps, complex_taps)
        centres = np.ascontiguousarray(centres, dtype=np.float64).reshape(-1)
        self._ctx = ctypes.c_void_p()
        self.taps = taps
        self.interpolation = int(interpolation)
        self.channels = int(centres.size)
        self._i16 = False
        init = self._L.if_fir_combiner_init_complex if complex_taps else self._L.if_fir_combiner_init
        if not init(ctypes.byref(self._ctx), _f32p(taps), count, self.interpolation,
                    self.channels, centres.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), int(max_samples), int(device)):
            self._ctx = ctypes.c_void_p()
            raise IfFirError(self._c("last_error")(None).decode())
        if backend is not None:
            self.set_backend(backend)

    def set_backend(self, backend):
        self._check(self._L.if_fir_combiner_set_backend(self._ctx, int(backend)))

    def get_backend(self):
        return int(self._L.if_fir_combiner_get_backend(self._ctx))

    def set_centres(self, centres):
        """if_fir_combiner_set_centres(): all centres at once, from the next call, as if set since the last reset."""
        centres = np.ascontiguousarray(centres, dtype=np.float64).reshape(-1)
        if centres.size != self.channels:
            raise IfFirError("if_fir_combiner_set_centres takes %d centres (got %d)" % (self.channels, centres.size))
        self._check(self._L.if_fir_combiner_set_centres(self._ctx, centres.ctypes.data_as(ctypes.POINTER(ctypes.c_double))))

    def get_centres(self):
        f = np.zeros(self.channels, dtype=np.float64)
        self._check(self._L.if_fir_combiner_get_centres(self._ctx, f.ctypes.data_as(ctypes.POINTER(ctypes.c_double))))
        return f

    def out_count(self, samples):
        return int(self._L.if_fir_combiner_out_count(self._ctx, int(samples)))

    def process(self, iqs):
        """if_fir_combiner_process(): one host array per channel (interleaved float32 / complex64, or int16 pairs after
        set_input_format(INPUT_I16)), all of one length, in; interleaved float32 out."""
        if len(iqs) != self.channels:
            raise IfFirError("if_fir_combiner_process takes %d channels (got %d)" % (self.channels, len(iqs)))
        arrs = [self._host_input(iq) for iq in iqs]
        n = arrs[0][1]
        if any(a[1] != n for a in arrs):
            raise IfFirError("if_fir_combiner_process: every channel brings the same number of samples")
        out = np.empty(2 * self.out_count(n), dtype=np.float32)
        m = ctypes.c_uint64(0)
        dummy = np.zeros(2, dtype=np.float32)
        ptrs = (ctypes.c_void_p * self.channels)(*[a[0].ctypes.data if n else dummy.ctypes.data for a in arrs])
        self._check(self._L.if_fir_combiner_process(self._ctx, ptrs, _f32p(out if out.size else dummy), n, ctypes.byref(m)))
        assert m.value * 2 == out.size
        return out

    def process_device(self, dev_ins, dev_out, samples):
        """if_fir_combiner_process_device(): raw device pointers (ints), one per channel, asynchronous.  Returns the output
        sample count."""
        if len(dev_ins) != self.channels:
            raise IfFirError("if_fir_combiner_process_device takes %d channels (got %d)" % (self.channels, len(dev_ins)))
        m = ctypes.c_uint64(0)
        ptrs = (ctypes.c_void_p * self.channels)(*[int(p) for p in dev_ins])
        self._check(self._L.if_fir_combiner_process_device(self._ctx, ptrs, ctypes.c_void_p(dev_out), int(samples), ctypes.byref(m)))
        return int(m.value)

    def debug_config(self, grid_limit=0):
        """if_fir_debug_combiner_config() (development library: construct with dev=True)."""
        self._check(self._L.if_fir_debug_combiner_config(self._ctx, int(grid_limit)))

    def debug_seek(self, samples):
        """if_fir_debug_combiner_seek() (development library): the next call's first output index becomes samples * L."""
        self._check(self._L.if_fir_debug_combiner_seek(self._ctx, int(samples)))


def debug_combiner_tables(taps, centre, complex_taps=False):
    """if_fir_debug_combiner_tables(): (G, r, the combiner's multiply table for the residual r as complex64) of a centre
    (host-only, no GPU)."""
    taps = np.ascontiguousarray(taps, dtype=np.float32)
    t = taps.size // 2 if complex_taps else taps.size
    out = np.zeros(2 * 4096, dtype=np.float32)
    grid, res = ctypes.c_uint32(0), ctypes.c_int32(0)
    if dev_lib().if_fir_debug_combiner_tables(_f32p(taps), t, 1 if complex_taps else 0, float(centre), ctypes.byref(grid),
                                              ctypes.byref(res), _f32p(out), out.size) != out.size:
        raise IfFirError("if_fir_debug_combiner_tables: %d taps at centre %r are not served by the overlap-save kernel" % (t, centre))
    return int(grid.value), int(res.value), out.view(np.complex64)


class IfFirResamp(_StreamCtx):
    """One if_fir_resamp_t: change the rate by interpolation / decimation in one polyphase pass (docs/SPEC.md §7).  Methods
    mirror the C entry points; how many outputs a call emits depends on the stream position (out_count)."""
    _PREFIX = "if_fir_resamp_"

    def __init__(self, taps, interpolation, decimation, max_samples=1 << 20, device=0, complex_taps=False, dev=False):
        self._L = dev_lib() if dev else lib()
        taps, count, complex_taps = _taps_arg(taps, complex_taps)
        self._ctx = ctypes.c_void_p()
        self.taps = taps
        self.interpolation, self.decimation = int(interpolation), int(decimation)
        self._i16 = False
        self._dev, self._grid_limit = bool(dev), 0
        init = self._L.if_fir_resamp_init_complex if complex_taps else self._L.if_fir_resamp_init
        if not init(ctypes.byref(self._ctx), _f32p(taps), count, self.interpolation,
                    self.decimation, int(max_samples), int(device)):
            self._ctx = ctypes.c_void_p()
            raise IfFirError(self._c("last_error")(None).decode())

    def out_count(self, samples):
        """if_fir_resamp_out_count(): outputs of a call with `samples` inputs at the current stream position."""
        return int(self._L.if_fir_resamp_out_count(self._ctx, int(samples)))

    def process(self, iq):
        """if_fir_resamp_process(): host interleaved float32 / complex64 (or int16 pairs after set_input_format(INPUT_I16)) in,
        interleaved float32 out."""
        return self._process(iq)

    def process_device(self, dev_in, dev_out, samples):
        """if_fir_resamp_process_device(): raw device pointers (ints), asynchronous.  Returns the output sample count."""
        return self._process_device(dev_in, dev_out, samples)

    def debug_config(self, grid_limit=0):
        """if_fir_debug_resamp_config() (development library: construct with dev=True): at most grid_limit workgroups (0 = the
        launcher's choice).  Returns the outputs of one tile of this context."""
        if not self._dev:
            raise IfFirError("if_fir_debug_resamp_config is in the development library only: construct with dev=True")
        tile = ctypes.c_uint32(0)
        self._check(self._L.if_fir_debug_resamp_config(self._ctx, int(grid_limit), ctypes.byref(tile)))
        self._grid_limit = int(grid_limit)
        return int(tile.value)

    def tile_outputs(self):
        """outputs one workgroup computes per tile (development library); the grid limit stays as it is"""
        return self.debug_config(self._grid_limit)


def step_from_rates(rate_in, rate_out):
    """if_fir_arb_step_from_rates(): the IfFirArb step for a pair of rates, rint(rate_in / rate_out * 2^32); 0 when that is
    outside 2^26 .. 2^34.  No context, no GPU."""
    return int(lib().if_fir_arb_step_from_rates(float(rate_in), float(rate_out)))


class IfFirArb(_StreamCtx):
    """One if_fir_arb_t: change the rate by any ratio 1/64 .. 4 with a step that can be retuned between calls (docs/SPEC.md
    §12).  `taps` is the real prototype designed at 2^phase_bits times the input rate; `step` is input samples per output
    sample times 2^32.  Methods mirror the C entry points; how many outputs a call emits depends on the position (out_count)."""
    _PREFIX = "if_fir_arb_"

    def __init__(self, taps, phase_bits, step, max_samples=1 << 20, device=0, dev=False):
        self._L = dev_lib() if dev else lib()
        taps = np.ascontiguousarray(taps, dtype=np.float32).reshape(-1)
        self._ctx = ctypes.c_void_p()
        self.taps = taps
        self.phase_bits, self._step = int(phase_bits), int(step)
        self._i16 = False
        self._dev, self._grid_limit = bool(dev), 0
        if not (0 <= self.phase_bits < 1 << 32 and 0 <= self._step < 1 << 64):
            raise IfFirError("if_fir_arb_init: phase bits and step must be unsigned (got %d, %d)" % (self.phase_bits, self._step))
        if not self._L.if_fir_arb_init(ctypes.byref(self._ctx), _f32p(taps), taps.size, self.phase_bits, self._step,
                                       int(max_samples), int(device)):
            self._ctx = ctypes.c_void_p()
            raise IfFirError(self._c("last_error")(None).decode())

    @property
    def step(self):
        """the step in force: input samples per output sample times 2^32"""
        return self._step

    def set_step(self, step):
        """if_fir_arb_set_step(): retune between calls; the position, the time of the next output and the history stay."""
        if not 0 <= int(step) < 1 << 64:
            raise IfFirError("if_fir_arb_set_step: step must be 2^26..2^34 (got %d)" % int(step))
        self._check(self._L.if_fir_arb_set_step(self._ctx, int(step)))
        self._step = int(step)

    def out_count(self, samples):
        """if_fir_arb_out_count(): outputs of a call with `samples` inputs at the current position and step."""
        return int(self._L.if_fir_arb_out_count(self._ctx, int(samples)))

    def process(self, iq):
        """if_fir_arb_process(): host interleaved float32 / complex64 (or int16 pairs after set_input_format(INPUT_I16)) in,
        interleaved float32 out."""
        return self._process(iq)

    def process_device(self, dev_in, dev_out, samples):
        """if_fir_arb_process_device(): raw device pointers (ints), asynchronous.  Returns the output sample count."""
        return self._process_device(dev_in, dev_out, samples)

    def debug_config(self, grid_limit=0, position=None, time_offset=0):
        """if_fir_debug_arb_config() (development library: construct with dev=True): at most grid_limit workgroups (0 = the
        launcher's choice); with `position`, on a freshly reset context, the next input has that absolute index and the next
        output comes time_offset / 2^32 samples after it.  Returns the outputs of one tile of this context."""
        if not self._dev:
            raise IfFirError("if_fir_debug_arb_config is in the development library only: construct with dev=True")
        tile = ctypes.c_uint32(0)
        pos = (1 << 64) - 1 if position is None else int(position)
        self._check(self._L.if_fir_debug_arb_config(self._ctx, int(grid_limit), ctypes.byref(tile), pos, int(time_offset)))
        self._grid_limit = int(grid_limit)
        return int(tile.value)

    def tile_outputs(self):
        """outputs one workgroup computes per tile (development library); the grid limit and the position stay as they are"""
        return self.debug_config(self._grid_limit)


class IfFirDdc(_StreamCtx):
    """One if_fir_ddc_t: REAL IF samples to decimated complex baseband in one pass -- NCO down-mix, filter, keep every
    decimation-th (docs/SPEC.md §10).  Methods mirror the C entry points; how many outputs a call emits depends on the stream
    position (out_count)."""
    _PREFIX = "if_fir_ddc_"
    NO_POSITION = (1 << 64) - 1

    def __init__(self, taps, decimation, max_samples=1 << 20, device=0, complex_taps=False, dev=False):
        self._L = dev_lib() if dev else lib()
        taps, count, complex_taps = _taps_arg(taps, complex_taps)
        self._ctx = ctypes.c_void_p()
        self.taps = taps
        self.decimation = int(decimation)
        self._i16 = False
        self._dev, self._grid_limit = bool(dev), 0
        init = self._L.if_fir_ddc_init_complex if complex_taps else self._L.if_fir_ddc_init
        if not init(ctypes.byref(self._ctx), _f32p(taps), count, self.decimation, int(max_samples), int(device)):
            self._ctx = ctypes.c_void_p()
            raise IfFirError(self._c("last_error")(None).decode())

    def set_nco(self, freq):
        """if_fir_ddc_set_nco(): mix the input down by exp(-j 2 pi f a), a = absolute sample index; 0 = off."""
        self._check(self._L.if_fir_ddc_set_nco(self._ctx, float(freq)))

    def get_nco(self):
        f = ctypes.c_double(0.0)
        self._check(self._L.if_fir_ddc_get_nco(self._ctx, ctypes.byref(f)))
        return float(f.value)

    def out_count(self, samples):
        """if_fir_ddc_out_count(): outputs of a call with `samples` inputs at the current stream position."""
        return int(self._L.if_fir_ddc_out_count(self._ctx, int(samples)))

    def _host_input(self, r):
        """(contiguous float32 -- or int16 after set_input_format(INPUT_I16) -- array of REAL samples, sample count)"""
        r = np.ascontiguousarray(r, dtype=np.int16 if self._i16 else np.float32).reshape(-1)
        return r, r.size

    def process(self, r):
        """if_fir_ddc_process(): host float32 (or int16 after set_input_format(INPUT_I16)) real samples in, interleaved
        float32 I, Q out."""
        return self._process(r)

    def process_device(self, dev_in, dev_out, samples):
        """if_fir_ddc_process_device(): raw device pointers (ints), asynchronous.  Returns the output sample count."""
        return self._process_device(dev_in, dev_out, samples)

    def debug_config(self, grid_limit=0, position=None):
        """if_fir_debug_ddc_config() (development library: construct with dev=True): at most grid_limit workgroups (0 = the
        launcher's choice); position (optional) = the absolute index of the next call's first sample, with the history zeroed.
        Returns the outputs of one tile of this context."""
        if not self._dev:
            raise IfFirError("if_fir_debug_ddc_config is in the development library only: construct with dev=True")
        tile = ctypes.c_uint32(0)
        self._check(self._L.if_fir_debug_ddc_config(self._ctx, int(grid_limit), ctypes.byref(tile),
                                                    self.NO_POSITION if position is None else int(position)))
        self._grid_limit = int(grid_limit)
        return int(tile.value)

    def tile_outputs(self):
        """outputs one workgroup computes per tile (development library); the grid limit stays as it is"""
        return self.debug_config(self._grid_limit)


class IfFirDuc(_StreamCtx):
    """One if_fir_duc_t: complex baseband to a REAL IF stream at `interpolation` times the rate in one pass -- upsample, filter,
    NCO up-mix, real part, optionally int16 (docs/SPEC.md §11).  Methods mirror the C entry points; N input samples give
    N * interpolation real outputs, float32 or (after set_output_format(OUTPUT_I16)) int16."""
    _PREFIX = "if_fir_duc_"
    NO_POSITION = (1 << 64) - 1

    def __init__(self, taps, interpolation, max_samples=1 << 20, device=0, complex_taps=False, dev=False):
        self._L = dev_lib() if dev else lib()
        taps, count, complex_taps = _taps_arg(taps, complex_taps)
        self._ctx = ctypes.c_void_p()
        self.taps = taps
        self.interpolation = int(interpolation)
        self._i16 = self._o16 = False
        self._dev, self._grid_limit = bool(dev), 0
        init = self._L.if_fir_duc_init_complex if complex_taps else self._L.if_fir_duc_init
        if not init(ctypes.byref(self._ctx), _f32p(taps), count, self.interpolation, int(max_samples), int(device)):
            self._ctx = ctypes.c_void_p()
            raise IfFirError(self._c("last_error")(None).decode())

    def set_output_format(self, fmt):
        """if_fir_duc_set_output_format(): OUTPUT_F32 or OUTPUT_I16 (the float32 result times 2^15, to nearest even, saturated)."""
        self._check(self._L.if_fir_duc_set_output_format(self._ctx, int(fmt)))
        self._o16 = (int(fmt) == OUTPUT_I16)

    def set_nco(self, freq):
        """if_fir_duc_set_nco(): mix the output up by exp(+j 2 pi f m), m = absolute output index, before the real part; 0 = off."""
        self._check(self._L.if_fir_duc_set_nco(self._ctx, float(freq)))

    def get_nco(self):
        f = ctypes.c_double(0.0)
        self._check(self._L.if_fir_duc_get_nco(self._ctx, ctypes.byref(f)))
        return float(f.value)

    def out_count(self, samples):
        """if_fir_duc_out_count(): samples * interpolation."""
        return int(self._L.if_fir_duc_out_count(self._ctx, int(samples)))

    def process(self, iq):
        """if_fir_duc_process(): host interleaved float32 / complex64 (or int16 pairs after set_input_format(INPUT_I16)) in, real
        float32 (or int16 after set_output_format(OUTPUT_I16)) out."""
        iq, n = self._host_input(iq)
        out = np.empty(self.out_count(n), dtype=np.int16 if self._o16 else np.float32)
        m = ctypes.c_uint64(0)
        dummy = np.zeros(2, dtype=np.float32)
        self._check(self._L.if_fir_duc_process(self._ctx, ctypes.c_void_p(iq.ctypes.data if n else dummy.ctypes.data),
                                               ctypes.c_void_p(out.ctypes.data if out.size else dummy.ctypes.data), n, ctypes.byref(m)))
        assert m.value == out.size
        return out

    def process_device(self, dev_in, dev_out, samples):
        """if_fir_duc_process_device(): raw device pointers (ints), asynchronous.  Returns the output sample count."""
        return self._process_device(dev_in, dev_out, samples)

    def debug_config(self, grid_limit=0, position=None):
        """if_fir_debug_duc_config() (development library: construct with dev=True): at most grid_limit workgroups (0 = the
        launcher's choice); position (optional) = the count of input samples before the next call, with the history zeroed.
        Returns the INPUT samples of one tile of this context."""
        if not self._dev:
            raise IfFirError("if_fir_debug_duc_config is in the development library only: construct with dev=True")
        tile = ctypes.c_uint32(0)
        self._check(self._L.if_fir_debug_duc_config(self._ctx, int(grid_limit), ctypes.byref(tile),
                                                    self.NO_POSITION if position is None else int(position)))
        self._grid_limit = int(grid_limit)
        return int(tile.value)

    def tile_inputs(self):
        """input samples one workgroup takes per tile (development library); the grid limit stays as it is"""
        return self.debug_config(self._grid_limit)


class IfFirPsd(_StreamCtx):
    """One if_fir_psd_t: averaged periodogram of an IQ stream as frames of uint16 spectrum codes, the layout wb_detect reads
    (docs/SPEC.md §8).  Methods mirror the C entry points; how many frames a call emits depends on the stream position
    (frame_count)."""
    _PREFIX = "if_fir_psd_"
    NO_POSITION = (1 << 64) - 1

    def __init__(self, size, hop, segments, first_bin, bins, ref_power=1.0, window=None, input_format=INPUT_F32,
                 max_samples=1 << 20, device=0, dev=False):
        self._L = dev_lib() if dev else lib()
        self._ctx = ctypes.c_void_p()
        self._dev = bool(dev)
        self.size, self.hop, self.segments, self.first_bin, self.bins = int(size), int(hop), int(segments), int(first_bin), int(bins)
        cfg = PsdConfig(self.size, self.hop, self.segments, self.first_bin, self.bins, float(ref_power), int(input_format))
        self._i16 = (int(input_format) == INPUT_I16)
        wp = None
        if window is not None:
            window = np.ascontiguousarray(window, dtype=np.float32)
            if window.size != self.size:
                raise IfFirError("IfFirPsd: the window must have size = %d values (got %d)" % (self.size, window.size))
            wp = _f32p(window)
        if not self._L.if_fir_psd_init(ctypes.byref(self._ctx), ctypes.byref(cfg), wp, int(max_samples), int(device)):
            self._ctx = ctypes.c_void_p()
            raise IfFirError(self._c("last_error")(None).decode())

    def frame_count(self, samples):
        """if_fir_psd_frame_count(): frames of a call with `samples` samples at the current stream position."""
        return int(self._L.if_fir_psd_frame_count(self._ctx, int(samples)))

    def process(self, iq, want_power=True):
        """if_fir_psd_process(): host interleaved float32 / complex64 (or int16 pairs after set_input_format(INPUT_I16)) in;
        returns ((frames, bins) uint16 codes, (frames, bins) float32 power or None)."""
        iq, n = self._host_input(iq)
        frames = self.frame_count(n)
        codes = np.empty((frames, self.bins), dtype=np.uint16)
        power = np.empty((frames, self.bins), dtype=np.float32) if want_power else None
        m = ctypes.c_uint32(0)
        dummy = np.zeros(2, dtype=np.float32)
        self._check(self._L.if_fir_psd_process(
            self._ctx, ctypes.c_void_p(iq.ctypes.data if n else dummy.ctypes.data), n,
            codes.ctypes.data_as(ctypes.POINTER(ctypes.c_uint16)) if frames else None,
            _f32p(power) if want_power and frames else None, ctypes.byref(m)))
        assert m.value == frames
        return codes, power

    def process_device(self, dev_in, samples, dev_bins, dev_power=0):
        """if_fir_psd_process_device(): raw device pointers (ints; dev_power may be 0), asynchronous.  Returns the frames emitted."""
        m = ctypes.c_uint32(0)
        self._check(self._L.if_fir_psd_process_device(self._ctx, ctypes.c_void_p(dev_in or None), int(samples),
                                                      ctypes.c_void_p(dev_bins or None), ctypes.c_void_p(dev_power or None),
                                                      ctypes.byref(m)))
        return int(m.value)

    def debug_plan(self, samples):
        """if_fir_debug_psd_plan() (development library: construct with dev=True): (segments, chunks, frames, carried samples)
        of the next call of `samples` samples."""
        if not self._dev:
            raise IfFirError("if_fir_debug_psd_plan is in the development library only: construct with dev=True")
        out = (ctypes.c_uint64 * 4)()
        self._check(self._L.if_fir_debug_psd_plan(self._ctx, int(samples), out))
        return tuple(int(v) for v in out)

    def debug_config(self, grid_limit=0, position=None):
        """if_fir_debug_psd_config() (development library: construct with dev=True): at most grid_limit workgroups of the chunk
        kernel (0 = the launcher's choice); position (optional) = the stream position of the next call's first sample, the first
        sample of a chunk, with nothing carried and the open frame's accumulator at +0."""
        if not self._dev:
            raise IfFirError("if_fir_debug_psd_config is in the development library only: construct with dev=True")
        self._check(self._L.if_fir_debug_psd_config(self._ctx, int(grid_limit),
                                                    self.NO_POSITION if position is None else int(position)))


class IfFirPfb(_StreamCtx):
    """One if_fir_pfb_t: all `channels` channels of a uniform grid out of one IQ stream in one pass, a frame of `bins` complex64
    values every `hop` input samples (docs/SPEC.md §13).  Methods mirror the C entry points; how many frames a call emits
    depends on the stream position (frame_count)."""
    _PREFIX = "if_fir_pfb_"
    NO_POSITION = (1 << 64) - 1

    def __init__(self, taps, channels, hop=None, first_bin=0, bins=None, max_samples=1 << 20, device=0, dev=False):
        self._L = dev_lib() if dev else lib()
        self._ctx = ctypes.c_void_p()
        self._dev, self._grid_limit = bool(dev), 0
        taps = np.ascontiguousarray(taps, dtype=np.float32).reshape(-1)
        self.taps = taps
        self.channels = int(channels)
        self.hop = self.channels if hop is None else int(hop)
        self.first_bin = int(first_bin)
        self.bins = self.channels if bins is None else int(bins)
        self._i16 = False
        if not all(0 <= v < 1 << 32 for v in (self.channels, self.hop, self.bins)) or not -(1 << 31) <= self.first_bin < 1 << 31:
            raise IfFirError("if_fir_pfb_init: channels, hop and bins must be unsigned, first_bin a 32-bit integer")
        cfg = PfbConfig(self.channels, self.hop, self.first_bin, self.bins)
        if not self._L.if_fir_pfb_init(ctypes.byref(self._ctx), ctypes.byref(cfg), _f32p(taps) if taps.size else None, taps.size,
                                       int(max_samples), int(device)):
            self._ctx = ctypes.c_void_p()
            raise IfFirError(self._c("last_error")(None).decode())

    def frame_count(self, samples):
        """if_fir_pfb_frame_count(): frames of a call with `samples` samples at the current stream position."""
        return int(self._L.if_fir_pfb_frame_count(self._ctx, int(samples)))

    def process(self, iq):
        """if_fir_pfb_process(): host interleaved float32 / complex64 (or int16 pairs after set_input_format(INPUT_I16)) in;
        returns the (frames, bins) complex64 array."""
        iq, n = self._host_input(iq)
        frames = self.frame_count(n)
        out = np.empty((frames, self.bins), dtype=np.complex64)
        m = ctypes.c_uint64(0)
        dummy = np.zeros(2, dtype=np.float32)
        self._check(self._L.if_fir_pfb_process(self._ctx, ctypes.c_void_p(iq.ctypes.data if n else dummy.ctypes.data),
                                               _f32p(out.view(np.float32) if out.size else dummy), n, ctypes.byref(m)))
        assert m.value == frames
        return out

    def process_device(self, dev_in, dev_out, samples):
        """if_fir_pfb_process_device(): raw device pointers (ints), asynchronous.  Returns the frames emitted."""
        m = ctypes.c_uint64(0)
        self._check(self._L.if_fir_pfb_process_device(self._ctx, ctypes.c_void_p(dev_in or None), ctypes.c_void_p(dev_out or None),
                                                      int(samples), ctypes.byref(m)))
        return int(m.value)

    def debug_config(self, grid_limit=0, position=None):
        """if_fir_debug_pfb_config() (development library: construct with dev=True): at most grid_limit workgroups (0 = the
        launcher's choice); position (optional) = the absolute index of the next call's first sample, with the history zeroed.
        Returns the consecutive frames one workgroup owns."""
        if not self._dev:
            raise IfFirError("if_fir_debug_pfb_config is in the development library only: construct with dev=True")
        group = ctypes.c_uint32(0)
        self._check(self._L.if_fir_debug_pfb_config(self._ctx, int(grid_limit), ctypes.byref(group),
                                                    self.NO_POSITION if position is None else int(position)))
        self._grid_limit = int(grid_limit)
        return int(group.value)


class IfFirRpfb(_StreamCtx):
    """One if_fir_rpfb_t: the `channels` / 2 + 1 distinct channels of a uniform grid out of one REAL sample stream in one pass, a
    frame of `bins` complex64 values every `hop` input samples (docs/SPEC.md §17).  Methods mirror the C entry points; how many
    frames a call emits depends on the stream position (frame_count)."""
    _PREFIX = "if_fir_rpfb_"
    NO_POSITION = (1 << 64) - 1

    def __init__(self, taps, channels, hop=None, first_bin=0, bins=None, max_samples=1 << 20, device=0, dev=False):
        self._L = dev_lib() if dev else lib()
        self._ctx = ctypes.c_void_p()
        self._dev, self._grid_limit = bool(dev), 0
        taps = np.ascontiguousarray(taps, dtype=np.float32).reshape(-1)
        self.taps = taps
        self.channels = int(channels)
        self.hop = self.channels if hop is None else int(hop)
        self.first_bin = int(first_bin)
        self.bins = self.channels // 2 + 1 - self.first_bin if bins is None else int(bins)
        self._i16 = False
        if not all(0 <= v < 1 << 32 for v in (self.channels, self.hop, self.first_bin, self.bins)):
            raise IfFirError("if_fir_rpfb_init: channels, hop, first_bin and bins must be unsigned 32-bit integers")
        cfg = RpfbConfig(self.channels, self.hop, self.first_bin, self.bins)
        if not self._L.if_fir_rpfb_init(ctypes.byref(self._ctx), ctypes.byref(cfg), _f32p(taps) if taps.size else None, taps.size,
                                        int(max_samples), int(device)):
            self._ctx = ctypes.c_void_p()
            raise IfFirError(self._c("last_error")(None).decode())

    def frame_count(self, samples):
        """if_fir_rpfb_frame_count(): frames of a call with `samples` samples at the current stream position."""
        return int(self._L.if_fir_rpfb_frame_count(self._ctx, int(samples)))

    def _host_input(self, r):
        """(contiguous float32 -- or int16 after set_input_format(INPUT_I16) -- array of REAL samples, sample count)"""
        r = np.ascontiguousarray(r, dtype=np.int16 if self._i16 else np.float32).reshape(-1)
        return r, r.size

    def process(self, r):
        """if_fir_rpfb_process(): host float32 (or int16 after set_input_format(INPUT_I16)) real samples in; returns the
        (frames, bins) complex64 array."""
        r, n = self._host_input(r)
        frames = self.frame_count(n)
        out = np.empty((frames, self.bins), dtype=np.complex64)
        m = ctypes.c_uint64(0)
        dummy = np.zeros(2, dtype=np.float32)
        self._check(self._L.if_fir_rpfb_process(self._ctx, ctypes.c_void_p(r.ctypes.data if n else dummy.ctypes.data),
                                                _f32p(out.view(np.float32) if out.size else dummy), n, ctypes.byref(m)))
        assert m.value == frames
        return out

    def process_device(self, dev_in, dev_out, samples):
        """if_fir_rpfb_process_device(): raw device pointers (ints), asynchronous.  Returns the frames emitted."""
        m = ctypes.c_uint64(0)
        self._check(self._L.if_fir_rpfb_process_device(self._ctx, ctypes.c_void_p(dev_in or None), ctypes.c_void_p(dev_out or None),
                                                       int(samples), ctypes.byref(m)))
        return int(m.value)

    def debug_config(self, grid_limit=0, position=None):
        """if_fir_debug_rpfb_config() (development library: construct with dev=True): at most grid_limit workgroups (0 = the
        launcher's choice); position (optional) = the absolute index of the next call's first sample, with the history zeroed.
        Returns the consecutive frames one workgroup owns."""
        if not self._dev:
            raise IfFirError("if_fir_debug_rpfb_config is in the development library only: construct with dev=True")
        group = ctypes.c_uint32(0)
        self._check(self._L.if_fir_debug_rpfb_config(self._ctx, int(grid_limit), ctypes.byref(group),
                                                     self.NO_POSITION if position is None else int(position)))
        self._grid_limit = int(grid_limit)
        return int(group.value)


class IfFirSynth(_StreamCtx):
    """One if_fir_synth_t: `channels` channel streams on a uniform grid to one IQ stream in one pass, `hop` output samples per
    frame of `bins` values (docs/SPEC.md §14).  Methods mirror the C entry points; its input is what IfFirPfb.process returns."""
    _PREFIX = "if_fir_synth_"
    NO_POSITION = (1 << 64) - 1
    ROUTE_PLAN, ROUTE_WORKSPACE, ROUTE_LDS = 0, 1, 2

    def __init__(self, taps, channels, hop=None, first_bin=0, bins=None, max_frames=1 << 12, device=0, dev=False):
        self._L = dev_lib() if dev else lib()
        self._ctx = ctypes.c_void_p()
        self._dev = bool(dev)
        taps = np.ascontiguousarray(taps, dtype=np.float32).reshape(-1)
        self.taps = taps
        self.channels = int(channels)
        self.hop = self.channels if hop is None else int(hop)
        self.first_bin = int(first_bin)
        self.bins = self.channels if bins is None else int(bins)
        self._i16 = False
        if not all(0 <= v < 1 << 32 for v in (self.channels, self.hop, self.bins)) or not -(1 << 31) <= self.first_bin < 1 << 31:
            raise IfFirError("if_fir_synth_init: channels, hop and bins must be unsigned, first_bin a 32-bit integer")
        cfg = SynthConfig(self.channels, self.hop, self.first_bin, self.bins)
        if not self._L.if_fir_synth_init(ctypes.byref(self._ctx), ctypes.byref(cfg), _f32p(taps) if taps.size else None, taps.size,
                                         int(max_frames), int(device)):
            self._ctx = ctypes.c_void_p()
            raise IfFirError(self._c("last_error")(None).decode())

    def sample_count(self, frames):
        """if_fir_synth_sample_count(): output samples of a call with `frames` frames at the current stream position."""
        return int(self._L.if_fir_synth_sample_count(self._ctx, int(frames)))

    def _frames_input(self, frames):
        """(contiguous array, frame count) of a host (frames, bins) array: complex64 / interleaved float32, or int16 pairs after
        set_input_format(INPUT_I16)"""
        x, n = self._host_input(frames)
        if n % self.bins:
            raise IfFirError("if_fir_synth_process: %d elements are not whole frames of %d bins" % (n, self.bins))
        return x, n // self.bins

    def process(self, frames):
        """if_fir_synth_process(): a host (frames, bins) array in (what IfFirPfb.process returns); interleaved float32 out."""
        x, f = self._frames_input(frames)
        out = np.empty(2 * f * self.hop, dtype=np.float32)
        m = ctypes.c_uint64(0)
        dummy = np.zeros(2, dtype=np.float32)
        self._check(self._L.if_fir_synth_process(self._ctx, ctypes.c_void_p(x.ctypes.data if f else dummy.ctypes.data),
                                                 _f32p(out if out.size else dummy), f, ctypes.byref(m)))
        assert m.value * 2 == out.size
        return out

    def process_device(self, dev_in, dev_out, frames):
        """if_fir_synth_process_device(): raw device pointers (ints), asynchronous.  Returns the samples emitted."""
        m = ctypes.c_uint64(0)
        self._check(self._L.if_fir_synth_process_device(self._ctx, ctypes.c_void_p(dev_in or None), ctypes.c_void_p(dev_out or None),
                                                        int(frames), ctypes.byref(m)))
        return int(m.value)

    def _need_dev(self, name):
        if not self._dev:
            raise IfFirError("%s is in the development library only: construct with dev=True" % name)

    def debug_config(self, grid_limit=0, route=0, position=None):
        """if_fir_debug_synth_config() (development library: construct with dev=True): at most grid_limit workgroups per kernel
        (0 = the launcher's choice); route 0 = the plan's choice, 1 = workspace, 2 = LDS (refused where it does not fit);
        position (optional) = the absolute index of the next call's first FRAME, with the history zeroed.  Returns the route in
        use."""
        self._need_dev("if_fir_debug_synth_config")
        got = ctypes.c_uint32(0)
        self._check(self._L.if_fir_debug_synth_config(self._ctx, int(grid_limit), int(route), ctypes.byref(got),
                                                      self.NO_POSITION if position is None else int(position)))
        return int(got.value)

    def debug_workspace(self, nbytes=0):
        """if_fir_debug_synth_workspace() (development library): nbytes > 0 replaces the workspace by one of that budget.
        Returns the frames of a call one chunk emits the outputs of."""
        self._need_dev("if_fir_debug_synth_workspace")
        got = ctypes.c_uint64(0)
        self._check(self._L.if_fir_debug_synth_workspace(self._ctx, int(nbytes), ctypes.byref(got)))
        return int(got.value)


class IfFirRsynth(_StreamCtx):
    """One if_fir_rsynth_t: the `channels` / 2 + 1 distinct channels of a uniform grid to one REAL stream in one pass, `hop` real
    output samples per frame of `bins` values (docs/SPEC.md §18).  Methods mirror the C entry points; its input is what
    IfFirRpfb.process returns, its output float32 or (after set_output_format(OUTPUT_I16)) int16."""
    _PREFIX = "if_fir_rsynth_"
    NO_POSITION = (1 << 64) - 1

    def __init__(self, taps, channels, hop=None, first_bin=0, bins=None, max_frames=1 << 12, device=0, dev=False):
        self._L = dev_lib() if dev else lib()
        self._ctx = ctypes.c_void_p()
        self._dev = bool(dev)
        taps = np.ascontiguousarray(taps, dtype=np.float32).reshape(-1)
        self.taps = taps
        self.channels = int(channels)
        self.hop = self.channels if hop is None else int(hop)
        self.first_bin = int(first_bin)
        self.bins = self.channels // 2 + 1 - self.first_bin if bins is None else int(bins)
        self._i16 = self._o16 = False
        if not all(0 <= v < 1 << 32 for v in (self.channels, self.hop, self.first_bin, self.bins)):
            raise IfFirError("if_fir_rsynth_init: channels, hop, first_bin and bins must be unsigned 32-bit integers")
        cfg = RsynthConfig(self.channels, self.hop, self.first_bin, self.bins)
        if not self._L.if_fir_rsynth_init(ctypes.byref(self._ctx), ctypes.byref(cfg), _f32p(taps) if taps.size else None, taps.size,
                                          int(max_frames), int(device)):
            self._ctx = ctypes.c_void_p()
            raise IfFirError(self._c("last_error")(None).decode())

    def set_output_format(self, fmt):
        """if_fir_rsynth_set_output_format(): OUTPUT_F32 or OUTPUT_I16 (the float32 result times 2^15, to nearest even, saturated)."""
        self._check(self._L.if_fir_rsynth_set_output_format(self._ctx, int(fmt)))
        self._o16 = (int(fmt) == OUTPUT_I16)

    def sample_count(self, frames):
        """if_fir_rsynth_sample_count(): output samples of a call with `frames` frames at the current stream position."""
        return int(self._L.if_fir_rsynth_sample_count(self._ctx, int(frames)))

    def _frames_input(self, frames):
        """(contiguous array, frame count) of a host (frames, bins) array: complex64 / interleaved float32, or int16 pairs after
        set_input_format(INPUT_I16)"""
        x, n = self._host_input(frames)
        if n % self.bins:
            raise IfFirError("if_fir_rsynth_process: %d elements are not whole frames of %d bins" % (n, self.bins))
        return x, n // self.bins

    def process(self, frames):
        """if_fir_rsynth_process(): a host (frames, bins) array in (what IfFirRpfb.process returns); real float32 (or int16 after
        set_output_format(OUTPUT_I16)) out."""
        x, f = self._frames_input(frames)
        out = np.empty(f * self.hop, dtype=np.int16 if self._o16 else np.float32)
        m = ctypes.c_uint64(0)
        dummy = np.zeros(2, dtype=np.float32)
        self._check(self._L.if_fir_rsynth_process(self._ctx, ctypes.c_void_p(x.ctypes.data if f else dummy.ctypes.data),
                                                  ctypes.c_void_p(out.ctypes.data if out.size else dummy.ctypes.data), f, ctypes.byref(m)))
        assert m.value == out.size
        return out

    def process_device(self, dev_in, dev_out, frames):
        """if_fir_rsynth_process_device(): raw device pointers (ints), asynchronous.  Returns the samples emitted."""
        m = ctypes.c_uint64(0)
        self._check(self._L.if_fir_rsynth_process_device(self._ctx, ctypes.c_void_p(dev_in or None), ctypes.c_void_p(dev_out or None),
                                                         int(frames), ctypes.byref(m)))
        return int(m.value)

    def _need_dev(self, name):
        if not self._dev:
            raise IfFirError("%s is in the development library only: construct with dev=True" % name)

    def debug_config(self, grid_limit=0, position=None):
        """if_fir_debug_rsynth_config() (development library: construct with dev=True): at most grid_limit workgroups per kernel
        (0 = the launcher's choice); position (optional) = the absolute index of the next call's first FRAME, with the history
        zeroed."""
        self._need_dev("if_fir_debug_rsynth_config")
        self._check(self._L.if_fir_debug_rsynth_config(self._ctx, int(grid_limit), self.NO_POSITION if position is None else int(position)))

    def debug_workspace(self, nbytes=0):
        """if_fir_debug_rsynth_workspace() (development library): nbytes > 0 replaces the workspace by one of that budget.
        Returns the frames of a call one chunk emits the outputs of."""
        self._need_dev("if_fir_debug_rsynth_workspace")
        got = ctypes.c_uint64(0)
        self._check(self._L.if_fir_debug_rsynth_workspace(self._ctx, int(nbytes), ctypes.byref(got)))
        return int(got.value)


class IfFirSub(_StreamCtx):
    """One if_fir_sub_t: the second stage of a two-stage channelizer over frames of `bins` elements (what IfFirPfb.process
    returns and IfFirSynth.process takes): every bin filtered by its own row of `taps` (one row for all bins, or a (bins, T)
    array), decimated by `decimation` and mixed by its own NCO in one pass (docs/SPEC.md §15).  Methods mirror the C entry
    points; how many frames a call emits depends on the stream position (frame_count)."""
    _PREFIX = "if_fir_sub_"
    NO_POSITION = (1 << 64) - 1

    def __init__(self, taps, bins, decimation=1, max_frames=1 << 12, device=0, dev=False, tap_rows=None):
        self._L = dev_lib() if dev else lib()
        self._ctx = ctypes.c_void_p()
        self._dev = bool(dev)
        taps = np.ascontiguousarray(taps, dtype=np.float32)
        self.bins = int(bins)
        self.decimation = int(decimation)
        self.tap_rows = int(tap_rows) if tap_rows is not None else (taps.shape[0] if taps.ndim == 2 else 1)
        self.taps = taps.reshape(-1)
        self.ntaps = self.taps.size // self.tap_rows if self.tap_rows > 0 else 0
        self._i16 = False
        if not all(0 <= v < 1 << 32 for v in (self.bins, self.ntaps, self.tap_rows, self.decimation)):
            raise IfFirError("if_fir_sub_init: bins, taps, tap rows and decimation must be unsigned 32-bit integers")
        cfg = SubConfig(self.bins, self.ntaps, self.tap_rows, self.decimation)
        if not self._L.if_fir_sub_init(ctypes.byref(self._ctx), ctypes.byref(cfg), _f32p(self.taps) if self.taps.size else None,
                                       int(max_frames), int(device)):
            self._ctx = ctypes.c_void_p()
            raise IfFirError(self._c("last_error")(None).decode())

    def set_nco(self, freqs):
        """if_fir_sub_set_nco(): `bins` frequencies in cycles per input frame, |f| <= 0.5; None sets every word to 0."""
        if freqs is None:
            self._check(self._L.if_fir_sub_set_nco(self._ctx, None))
            return
        f = np.ascontiguousarray(freqs, dtype=np.float64).reshape(-1)
        if f.size != self.bins:
            raise IfFirError("if_fir_sub_set_nco: %d frequencies for %d bins" % (f.size, self.bins))
        self._check(self._L.if_fir_sub_set_nco(self._ctx, f.ctypes.data_as(ctypes.POINTER(ctypes.c_double))))

    def get_nco(self):
        """if_fir_sub_get_nco(): the quantised frequencies in force, one per bin."""
        f = np.zeros(self.bins, dtype=np.float64)
        self._check(self._L.if_fir_sub_get_nco(self._ctx, f.ctypes.data_as(ctypes.POINTER(ctypes.c_double))))
        return f

    def frame_count(self, frames):
        """if_fir_sub_frame_count(): output frames of a call with `frames` frames at the current stream position."""
        return int(self._L.if_fir_sub_frame_count(self._ctx, int(frames)))

    def process(self, frames):
        """if_fir_sub_process(): a host (frames, bins) array in (complex64 / interleaved float32, or int16 pairs after
        set_input_format(INPUT_I16)); returns the (output frames, bins) complex64 array."""
        x, n = self._host_input(frames)
        if n % self.bins:
            raise IfFirError("if_fir_sub_process: %d elements are not whole frames of %d bins" % (n, self.bins))
        f = n // self.bins
        out = np.empty((self.frame_count(f), self.bins), dtype=np.complex64)
        m = ctypes.c_uint64(0)
        dummy = np.zeros(2, dtype=np.float32)
        self._check(self._L.if_fir_sub_process(self._ctx, ctypes.c_void_p(x.ctypes.data if f else dummy.ctypes.data),
                                               _f32p(out.view(np.float32) if out.size else dummy), f, ctypes.byref(m)))
        assert m.value == out.shape[0]
        return out

    def process_device(self, dev_in, dev_out, frames):
        """if_fir_sub_process_device(): raw device pointers (ints), asynchronous.  Returns the frames emitted."""
        m = ctypes.c_uint64(0)
        self._check(self._L.if_fir_sub_process_device(self._ctx, ctypes.c_void_p(dev_in or None), ctypes.c_void_p(dev_out or None),
                                                      int(frames), ctypes.byref(m)))
        return int(m.value)

    def debug_config(self, grid_limit=0, position=None):
        """if_fir_debug_sub_config() (development library: construct with dev=True): at most grid_limit workgroups per kernel
        (0 = the launcher's choice); position (optional) = the absolute index of the next call's first FRAME, with the history
        zeroed.  Returns the (output, bin) values one tile holds."""
        if not self._dev:
            raise IfFirError("if_fir_debug_sub_config is in the development library only: construct with dev=True")
        tile = ctypes.c_uint32(0)
        self._check(self._L.if_fir_debug_sub_config(self._ctx, int(grid_limit), ctypes.byref(tile),
                                                    self.NO_POSITION if position is None else int(position)))
        return int(tile.value)


class IfFirSubUp(_StreamCtx):
    """One if_fir_subup_t: the transmit mirror of IfFirSub over frames of `bins` elements (what IfFirSynth.process takes): every
    bin interpolated by `interpolation` through its own row of `taps` (one row for all bins, or a (bins, T) array) and mixed up
    by its own NCO in one pass (docs/SPEC.md §16).  Methods mirror the C entry points; F frames in give F * interpolation out."""
    _PREFIX = "if_fir_subup_"
    NO_POSITION = (1 << 64) - 1

    def __init__(self, taps, bins, interpolation=1, max_frames=1 << 12, device=0, dev=False, tap_rows=None):
        self._L = dev_lib() if dev else lib()
        self._ctx = ctypes.c_void_p()
        self._dev = bool(dev)
        taps = np.ascontiguousarray(taps, dtype=np.float32)
        self.bins = int(bins)
        self.interpolation = int(interpolation)
        self.tap_rows = int(tap_rows) if tap_rows is not None else (taps.shape[0] if taps.ndim == 2 else 1)
        self.taps = taps.reshape(-1)
        self.ntaps = self.taps.size // self.tap_rows if self.tap_rows > 0 else 0
        self._i16 = False
        if not all(0 <= v < 1 << 32 for v in (self.bins, self.ntaps, self.tap_rows, self.interpolation)):
            raise IfFirError("if_fir_subup_init: bins, taps, tap rows and interpolation must be unsigned 32-bit integers")
        cfg = SubUpConfig(self.bins, self.ntaps, self.tap_rows, self.interpolation)
        if not self._L.if_fir_subup_init(ctypes.byref(self._ctx), ctypes.byref(cfg), _f32p(self.taps) if self.taps.size else None,
                                         int(max_frames), int(device)):
            self._ctx = ctypes.c_void_p()
            raise IfFirError(self._c("last_error")(None).decode())

    def set_nco(self, freqs):
        """if_fir_subup_set_nco(): `bins` frequencies in cycles per OUTPUT frame, |f| <= 0.5; None sets every word to 0."""
        if freqs is None:
            self._check(self._L.if_fir_subup_set_nco(self._ctx, None))
            return
        f = np.ascontiguousarray(freqs, dtype=np.float64).reshape(-1)
        if f.size != self.bins:
            raise IfFirError("if_fir_subup_set_nco: %d frequencies for %d bins" % (f.size, self.bins))
        self._check(self._L.if_fir_subup_set_nco(self._ctx, f.ctypes.data_as(ctypes.POINTER(ctypes.c_double))))

    def get_nco(self):
        """if_fir_subup_get_nco(): the quantised frequencies in force, one per bin."""
        f = np.zeros(self.bins, dtype=np.float64)
        self._check(self._L.if_fir_subup_get_nco(self._ctx, f.ctypes.data_as(ctypes.POINTER(ctypes.c_double))))
        return f

    def frame_count(self, frames):
        """if_fir_subup_frame_count(): output frames of a call with `frames` frames (0 where the call would be refused)."""
        return int(self._L.if_fir_subup_frame_count(self._ctx, int(frames)))

    def process(self, frames):
        """if_fir_subup_process(): a host (frames, bins) array in (complex64 / interleaved float32, or int16 pairs after
        set_input_format(INPUT_I16)); returns the (frames * interpolation, bins) complex64 array."""
        x, n = self._host_input(frames)
        if n % self.bins:
            raise IfFirError("if_fir_subup_process: %d elements are not whole frames of %d bins" % (n, self.bins))
        f = n // self.bins
        out = np.empty((self.frame_count(f), self.bins), dtype=np.complex64)
        m = ctypes.c_uint64(0)
        dummy = np.zeros(2, dtype=np.float32)
        self._check(self._L.if_fir_subup_process(self._ctx, ctypes.c_void_p(x.ctypes.data if f else dummy.ctypes.data),
                                                 _f32p(out.view(np.float32) if out.size else dummy), f, ctypes.byref(m)))
        assert m.value == out.shape[0]
        return out

    def process_device(self, dev_in, dev_out, frames):
        """if_fir_subup_process_device(): raw device pointers (ints), asynchronous.  Returns the frames emitted."""
        m = ctypes.c_uint64(0)
        self._check(self._L.if_fir_subup_process_device(self._ctx, ctypes.c_void_p(dev_in or None), ctypes.c_void_p(dev_out or None),
                                                        int(frames), ctypes.byref(m)))
        return int(m.value)

    def debug_config(self, grid_limit=0, position=None):
        """if_fir_debug_subup_config() (development library: construct with dev=True): at most grid_limit workgroups per
        kernel (0 = the launcher's choice); position (optional) = the absolute index of the next call's first INPUT frame, with
        the history zeroed.  Returns the (output, bin) values one tile holds."""
        if not self._dev:
            raise IfFirError("if_fir_debug_subup_config is in the development library only: construct with dev=True")
        tile = ctypes.c_uint32(0)
        self._check(self._L.if_fir_debug_subup_config(self._ctx, int(grid_limit), ctypes.byref(tile),
                                                      self.NO_POSITION if position is None else int(position)))
        return int(tile.value)


FFT_TABLE_FLOATS = 2 * (4096 + 4096 + 256 + 1024 + 1024 + 64 + 256)


class IfFirFpow(_StreamCtx):
    """One if_fir_fpow_t: the power stage over frames of `bins` elements (what IfFirPfb, IfFirRpfb and IfFirSub emit): every
    output bin sums `group` adjacent elements from `first` on, every output frame averages `frames` input frames, and the result
    comes as the uint16 spectrum codes wb_detect reads and, optionally, as float32 powers (docs/SPEC.md §19).  Methods mirror
    the C entry points; how many frames a call emits depends on the stream position (frame_count)."""
    _PREFIX = "if_fir_fpow_"
    NO_POSITION = (1 << 64) - 1

    def __init__(self, bins, frames, norm=1.0, first=0, group=1, out_bins=None, ref_power=1.0, input_format=INPUT_F32,
                 max_frames=1 << 12, device=0, dev=False):
        self._L = dev_lib() if dev else lib()
        self._ctx = ctypes.c_void_p()
        self._dev = bool(dev)
        self.bins, self.first, self.group, self.frames = int(bins), int(first), int(group), int(frames)
        self.out_bins = int(out_bins) if out_bins is not None else (max(self.bins - self.first, 0) // self.group if self.group > 0 else 0)
        self._i16 = (int(input_format) == INPUT_I16)
        if not all(0 <= v < 1 << 32 for v in (self.bins, self.first, self.group, self.out_bins, self.frames, int(input_format))):
            raise IfFirError("if_fir_fpow_init: bins, first, group, output bins, frames and format must be unsigned 32-bit integers")
        cfg = FpowConfig(self.bins, self.first, self.group, self.out_bins, self.frames, float(norm), float(ref_power), int(input_format))
        if not self._L.if_fir_fpow_init(ctypes.byref(self._ctx), ctypes.byref(cfg), int(max_frames), int(device)):
            self._ctx = ctypes.c_void_p()
            raise IfFirError(self._c("last_error")(None).decode())

    def frame_count(self, frames):
        """if_fir_fpow_frame_count(): output frames of a call with `frames` input frames at the current stream position."""
        return int(self._L.if_fir_fpow_frame_count(self._ctx, int(frames)))

    def process(self, frames, want_power=True):
        """if_fir_fpow_process(): a host (frames, bins) array in (complex64 / interleaved float32, or int16 pairs after
        set_input_format(INPUT_I16)); returns ((output frames, out_bins) uint16 codes, float32 powers of that shape or None)."""
        x, n = self._host_input(frames)
        if n % self.bins:
            raise IfFirError("if_fir_fpow_process: %d elements are not whole frames of %d bins" % (n, self.bins))
        f = n // self.bins
        m_want = self.frame_count(f)
        codes = np.empty((m_want, self.out_bins), dtype=np.uint16)
        power = np.empty((m_want, self.out_bins), dtype=np.float32) if want_power else None
        m = ctypes.c_uint32(0)
        dummy = np.zeros(2, dtype=np.float32)
        self._check(self._L.if_fir_fpow_process(
            self._ctx, ctypes.c_void_p(x.ctypes.data if f else dummy.ctypes.data), f,
            codes.ctypes.data_as(ctypes.POINTER(ctypes.c_uint16)) if m_want else None,
            _f32p(power) if want_power and m_want else None, ctypes.byref(m)))
        assert m.value == m_want
        return codes, power

    def process_device(self, dev_in, frames, dev_bins, dev_power=0):
        """if_fir_fpow_process_device(): raw device pointers (ints; dev_power may be 0), asynchronous.  Returns the frames emitted."""
        m = ctypes.c_uint32(0)
        self._check(self._L.if_fir_fpow_process_device(self._ctx, ctypes.c_void_p(dev_in or None), int(frames),
                                                       ctypes.c_void_p(dev_bins or None), ctypes.c_void_p(dev_power or None),
                                                       ctypes.byref(m)))
        return int(m.value)

    def debug_config(self, grid_limit=0, position=None):
        """if_fir_debug_fpow_config() (development library: construct with dev=True): at most grid_limit workgroups per kernel
        (0 = the launcher's choice); position (optional) = the absolute index of the next call's first input FRAME, with the
        carried sums cleared."""
        if not self._dev:
            raise IfFirError("if_fir_debug_fpow_config is in the development library only: construct with dev=True")
        self._check(self._L.if_fir_debug_fpow_config(self._ctx, int(grid_limit),
                                                     self.NO_POSITION if position is None else int(position)))


TURN_TO_STREAMS, TURN_TO_FRAMES = 0, 1


class IfFirTurn(_StreamCtx):
    """One if_fir_turn_t: the corner turn between frames of `bins` elements (the layout of IfFirPfb, IfFirRpfb, IfFirSub, IfFirSubUp,
    IfFirSynth, IfFirRsynth and IfFirFpow) and one contiguous row per listed bin (what the stream families read and write), with
    the format conversion fused (docs/SPEC.md §20).  `sel` is a list of distinct bins in any order, or None for the span
    first .. first + channels - 1.  The stage carries no state: there is no reset.  Methods mirror the C entry points."""
    _PREFIX = "if_fir_turn_"

    def __init__(self, direction, bins, sel=None, channels=None, first=0, input_format=INPUT_F32, output_format=OUTPUT_F32,
                 max_frames=1 << 12, device=0, dev=False):
        self._L = dev_lib() if dev else lib()
        self._ctx = ctypes.c_void_p()
        self._dev = bool(dev)
        self.direction, self.bins, self.first = int(direction), int(bins), int(first)
        if sel is not None:
            sel = [int(v) for v in np.asarray(sel).reshape(-1)]
            if not all(0 <= v < 1 << 32 for v in sel):
                raise IfFirError("if_fir_turn_init: listed bins must be unsigned 32-bit integers")
        self.channels = int(channels) if channels is not None else (len(sel) if sel is not None else self.bins - self.first)
        self._i16 = (int(input_format) == INPUT_I16)
        self._o16 = (int(output_format) == OUTPUT_I16)
        if not all(0 <= v < 1 << 32 for v in (self.direction, self.bins, self.channels, self.first, int(input_format), int(output_format))):
            raise IfFirError("if_fir_turn_init: direction, bins, channels, first and the formats must be unsigned 32-bit integers")
        if sel is not None and len(sel) != self.channels:
            raise IfFirError("if_fir_turn_init: %d listed bins for %d channels" % (len(sel), self.channels))
        cfg = TurnConfig(self.direction, self.bins, self.channels, self.first, int(input_format), int(output_format))
        arr = (ctypes.c_uint32 * max(len(sel), 1))(*sel) if sel is not None else None
        if not self._L.if_fir_turn_init(ctypes.byref(self._ctx), ctypes.byref(cfg), arr, int(max_frames), int(device)):
            self._ctx = ctypes.c_void_p()
            raise IfFirError(self._c("last_error")(None).decode())
        self.sel = list(sel) if sel is not None else list(range(self.first, self.first + self.channels))

    def reset(self):
        raise IfFirError("if_fir_turn_t carries no state: there is no reset")

    def set_output_format(self, fmt):
        """if_fir_turn_set_output_format(): OUTPUT_F32 or OUTPUT_I16 (times 2^15, to nearest even, saturated; NaN gives 0)."""
        self._check(self._L.if_fir_turn_set_output_format(self._ctx, int(fmt)))
        self._o16 = (int(fmt) == OUTPUT_I16)

    def process(self, data, pitch=None, frames=None):
        """if_fir_turn_process(): host arrays.  TO_STREAMS: a (frames, bins) array in (complex64 / interleaved float32, or int16
        pairs after set_input_format(INPUT_I16)), a (channels, pitch, 2) float32 or int16 array out (pitch: default frames), of
        which [:, :frames] is written and the rest is zero.  TO_FRAMES: a (channels, pitch) array of elements in, of which the
        first `frames` (default: pitch) of every row are used, a (frames, bins, 2) array out."""
        x, n = self._host_input(data)
        odt = np.int16 if self._o16 else np.float32
        if self.direction == TURN_TO_FRAMES:
            if n % self.channels:
                raise IfFirError("if_fir_turn_process: %d elements are not %d rows" % (n, self.channels))
            p = n // self.channels
            f = p if frames is None else int(frames)
            out = np.zeros((max(f, 0), self.bins, 2), dtype=odt)
        else:
            if n % self.bins:
                raise IfFirError("if_fir_turn_process: %d elements are not whole frames of %d bins" % (n, self.bins))
            f = n // self.bins
            p = f if pitch is None else int(pitch)
            out = np.zeros((self.channels, p, 2), dtype=odt)
        dummy = np.zeros(2, dtype=np.float32)
        self._check(self._L.if_fir_turn_process(self._ctx, ctypes.c_void_p(x.ctypes.data if x.size else dummy.ctypes.data),
                                                ctypes.c_void_p(out.ctypes.data if out.size else dummy.ctypes.data), f, p))
        return out

    def process_device(self, dev_in, dev_out, frames, pitch=None):
        """if_fir_turn_process_device(): raw device pointers (ints), asynchronous; pitch in elements (default: frames)."""
        self._check(self._L.if_fir_turn_process_device(self._ctx, ctypes.c_void_p(dev_in or None), ctypes.c_void_p(dev_out or None),
                                                       int(frames), int(frames if pitch is None else pitch)))

    def debug_config(self, grid_limit=0):
        """if_fir_debug_turn_config() (development library: construct with dev=True): at most grid_limit workgroups (0 = the
        launcher's choice)."""
        if not self._dev:
            raise IfFirError("if_fir_debug_turn_config is in the development library only: construct with dev=True")
        self._check(self._L.if_fir_debug_turn_config(self._ctx, int(grid_limit)))


def debug_fft_tables(taps, decimation, complex_taps=False, nco_delta=0):
    """if_fir_debug_fft_tables(): the overlap-save kernel's table image as complex64 sections (host-only, no GPU)."""
    taps = np.ascontiguousarray(taps, dtype=np.float32)
    t = taps.size // 2 if complex_taps else taps.size
    out = np.zeros(FFT_TABLE_FLOATS, dtype=np.float32)
    n = dev_lib().if_fir_debug_fft_tables(_f32p(taps), t, 1 if complex_taps else 0, int(decimation), int(nco_delta) & 0xFFFFFFFF,
                                      _f32p(out), out.size)
    if n != FFT_TABLE_FLOATS:
        raise IfFirError("if_fir_debug_fft_tables: (taps=%d, decimation=%d) is not served by the overlap-save kernel" % (t, decimation))
    c = out.view(np.complex64)
    return {"tw1": c[0:4096], "hp": c[4096:8192], "tw2": c[8192:8448], "twd": c[8448:9472], "twe": c[9472:10496],
            "ncob": c[10496:10560], "twf": c[10560:10816]}


def debug_fft_tables_bank(taps, bank, parity=0, complex_taps=False):
    """if_fir_debug_fft_tables_bank(): a filter bank's table image (bank 8 or 16) as complex64 sections (host-only)."""
    taps = np.ascontiguousarray(taps, dtype=np.float32)
    t = taps.size // 2 if complex_taps else taps.size
    out = np.zeros(FFT_TABLE_FLOATS, dtype=np.float32)
    L = dev_lib()
    L.if_fir_debug_fft_tables_bank.restype = ctypes.c_uint32
    n = L.if_fir_debug_fft_tables_bank(_f32p(taps), ctypes.c_uint32(t), ctypes.c_uint32(1 if complex_taps else 0), ctypes.c_uint32(int(bank)),
                                       ctypes.c_uint32(int(parity)), _f32p(out), ctypes.c_uint32(out.size))
    if n != FFT_TABLE_FLOATS:
        raise IfFirError("if_fir_debug_fft_tables_bank: (taps=%d, bank=%d) is not served" % (t, bank))
    c = out.view(np.complex64)
    return {"tw1": c[0:4096], "hp": c[4096:8192], "tw2": c[8192:8448], "twd": c[8448:9472], "twe": c[9472:10496], "ncob": c[10496:10560]}


def debug_bank_tail(decimation, own_centres=False):
    """if_fir_debug_bank_tail(): the bank's tail (4, 8, 16) for a decimation, 0 if the bank does not serve it."""
    L = dev_lib()
    L.if_fir_debug_bank_tail.restype = ctypes.c_uint32
    return int(L.if_fir_debug_bank_tail(ctypes.c_uint32(int(decimation)), ctypes.c_uint32(1 if own_centres else 0)))


def debug_bank8_plan(slots):
    """if_fir_debug_bank_plan(): (mask of the even slots' all-slots launch, mask of the odd slots', channels left per channel)."""
    k = len(slots)
    arr = (ctypes.c_uint32 * k)(*[int(v) for v in slots])
    out = (ctypes.c_uint32 * 3)()
    L = dev_lib()
    L.if_fir_debug_bank_plan.restype = ctypes.c_uint8
    if not L.if_fir_debug_bank_plan(arr, ctypes.c_uint32(k), out):
        raise IfFirError("if_fir_debug_bank_plan: 1..16 channels")
    return int(out[0]), int(out[1]), [c for c in range(k) if (out[2] >> c) & 1]


def debug_fft_tables_odd(taps, decimation, complex_taps=False, nco_delta=0):
    """if_fir_debug_fft_tables_odd(): the odd-decimation kernel's table image (decimation 3, 9, 15, ...) as complex64 sections."""
    taps = np.ascontiguousarray(taps, dtype=np.float32)
    t = taps.size // 2 if complex_taps else taps.size
    nfl = 10496 + 512
    out = np.zeros(nfl, dtype=np.float32)
    L = dev_lib()
    L.if_fir_debug_fft_tables_odd.restype = ctypes.c_uint32
    n = L.if_fir_debug_fft_tables_odd(_f32p(taps), ctypes.c_uint32(t), ctypes.c_uint32(1 if complex_taps else 0),
                                      ctypes.c_uint32(int(decimation)), ctypes.c_uint32(int(nco_delta) & 0xFFFFFFFF), _f32p(out),
                                      ctypes.c_uint32(out.size))
    if n != nfl:
        raise IfFirError("if_fir_debug_fft_tables_odd: (taps=%d, decimation=%d) is not served by the odd-decimation kernel" % (t, decimation))
    c = out.view(np.complex64)
    return {"g": c[0:3072], "tb": c[3072:3328], "tc": c[3328:4096], "twd": c[4096:5120], "twe": c[5120:5184], "ncob": c[5184:5248], "pht": c[5248:5504]}


def debug_fft_schedule(nblocks, workgroups=256, single_ok=True):
    """if_fir_debug_fft_schedule(): the plan of an overlap-save launch (host-only), as the launcher makes it: wgs = workgroups
    launched, nblocks_main = blocks handed out in groups (the rest is the tail phase), single = single-round launch (wave w of
    workgroup b takes block w * wgs + b), tickets = bound of the global counter.  single_ok=False: the single-round form off."""
    out = (ctypes.c_int64 * 4)()
    if not dev_lib().if_fir_debug_fft_schedule(int(nblocks), int(workgroups), 1 if single_ok else 0, out):
        raise IfFirError("if_fir_debug_fft_schedule: bad arguments")
    return dict(zip(("wgs", "nblocks_main", "single", "tickets"), [int(v) for v in out]))


def mc_owner(channel, world):
    """if_fir_mc_owner(): the rank that filters a channel (channel mod world)."""
    return int(lib().if_fir_mc_owner(int(channel), int(world)))


# a chunk request the tests use: 215 040 samples (round 3's global unit); the library rounds any request to the context's own
# unit = lcm(block advance of its filter, 2 D) (IfFirMc.get_chunk_samples)
MC_CHUNK_UNIT = 215040
MC_NEVER_SPLIT = (1 << 64) - 1


def mc_debug_plan(world, channels, rank, samples, in_bytes=8, decimation=1, consumed=0, chunk=0, taps=255):
    """if_fir_mc_debug_plan(): list of dict(kind, phase, group, peer, channel, chunk, offset, bytes) in posting order
    (host-only; chunk=0 means one piece here)."""
    n = dev_lib().if_fir_mc_debug_plan(int(world), int(channels), int(rank), int(samples), int(in_bytes), int(taps),
                                       int(decimation), int(consumed), int(chunk), None, 0)
    buf = np.zeros(8 * max(n, 1), dtype=np.uint64)
    dev_lib().if_fir_mc_debug_plan(int(world), int(channels), int(rank), int(samples), int(in_bytes), int(taps), int(decimation),
                                   int(consumed), int(chunk), buf.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), n)
    keys = ("kind", "phase", "group", "peer", "channel", "chunk", "offset", "bytes")
    return [dict(zip(keys, (int(v) for v in buf[8 * i:8 * i + 8]))) for i in range(n)]


def mc_unique_id():
    """if_fir_mc_unique_id(): rank 0's RCCL bootstrap id (128 bytes) to hand to the other ranks."""
    buf = (ctypes.c_uint8 * MC_ID_BYTES)()
    if not lib().if_fir_mc_unique_id(buf):
        raise IfFirError(lib().if_fir_mc_last_error(None).decode())
    return bytes(buf)


class IfFirMc:
    """One if_fir_mc_ctx_t: channel c -> rank c mod world, inputs/outputs on rank 0's GPU (see include/if_fir.h)."""

    def __init__(self, taps, decimation, max_samples, device=0, rank=0, world=1, unique_id=None, dev=False):
        self._L = dev_lib() if dev else lib()
        taps = np.ascontiguousarray(np.asarray(taps, dtype=np.float32))
        if taps.ndim != 2:
            raise IfFirError("taps must be a (channels, taps) array")
        self.channels, self.rank, self.world = int(taps.shape[0]), int(rank), int(world)
        self._ctx = ctypes.c_void_p(None)
        idbuf = None
        if unique_id is not None:
            idbuf = (ctypes.c_uint8 * MC_ID_BYTES).from_buffer_copy(bytes(unique_id))
        ok = self._L.if_fir_mc_init(ctypes.byref(self._ctx), self.channels, _f32p(taps), int(taps.shape[1]),
                                  int(decimation), int(max_samples), int(device), self.rank, self.world, idbuf)
        if not ok:
            self._ctx = ctypes.c_void_p(None)
            raise IfFirError(self._L.if_fir_mc_last_error(None).decode())

    def _check(self, ok):
        if not ok:
            raise IfFirError(self._L.if_fir_mc_last_error(self._ctx).decode())

    def reset(self):
        self._check(self._L.if_fir_mc_reset(self._ctx))

    def set_input_format(self, fmt):
        self._check(self._L.if_fir_mc_set_input_format(self._ctx, int(fmt)))

    def set_chunk_samples(self, chunk):
        """0 = default chunk, MC_NEVER_SPLIT = whole calls, else a request in samples (rounded to the context's unit)."""
        self._check(self._L.if_fir_mc_set_chunk_samples(self._ctx, int(chunk)))

    def get_chunk_samples(self):
        """(chunk in effect, 0 = calls are not split; the unit it is a multiple of)"""
        c, u = ctypes.c_uint64(0), ctypes.c_uint64(0)
        self._check(self._L.if_fir_mc_get_chunk_samples(self._ctx, ctypes.byref(c), ctypes.byref(u)))
        return int(c.value), int(u.value)

    def channel_ctx(self, channel):
        """Raw if_fir_ctx_t* (int) of a channel this rank owns, else None."""
        return self._L.if_fir_mc_channel_ctx(self._ctx, int(channel))

    def set_backend(self, backend):
        """if_fir_set_backend() on every channel this rank owns."""
        for c in range(self.channels):
            h = self.channel_ctx(c)
            if h and not self._L.if_fir_set_backend(h, int(backend)):
                raise IfFirError(self._L.if_fir_last_error(h).decode())

    def process_device(self, dev_in, dev_out, samples):
        """if_fir_mc_process_device(): lists of device pointers (ints) on rank 0, None elsewhere.  Returns the
        per-channel output sample count."""
        m = ctypes.c_uint64(0)
        pin = pout = None
        if dev_in is not None:
            pin = (ctypes.c_void_p * self.channels)(*[ctypes.c_void_p(int(p)) for p in dev_in])
            pout = (ctypes.c_void_p * self.channels)(*[ctypes.c_void_p(int(p)) for p in dev_out])
        self._check(self._L.if_fir_mc_process_device(self._ctx, pin, pout, int(samples), ctypes.byref(m)))
        return int(m.value)

    def close(self):
        if self._ctx:
            self._L.if_fir_mc_destroy(self._ctx)
            self._ctx = ctypes.c_void_p(None)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
