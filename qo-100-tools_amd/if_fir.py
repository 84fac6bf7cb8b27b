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


# The C ABI, written down once: name -> (restype, [argtypes]) of every symbol include/if_fir.h declares (ABI) and of every symbol
# include/if_fir_debug.h declares (DEV_ABI).  _load() applies them, EXPORTS and DEV_EXPORTS are their keys, and
# tests/test_binding_host.py holds every entry against its prototype in the header.  A new family adds its name to _FAMILIES and
# one _declare() per table below.
_U8, _U32, _U64, _I32, _F64, _VP, _STR = (ctypes.c_uint8, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int32, ctypes.c_double,
                                          ctypes.c_void_p, ctypes.c_char_p)
_U8P, _U16P, _U32P, _U64P, _I32P, _I64P, _F32P, _F64P, _VPP = (ctypes.POINTER(t) for t in (
    ctypes.c_uint8, ctypes.c_uint16, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int32, ctypes.c_int64, ctypes.c_float, ctypes.c_double,
    ctypes.c_void_p))
# the signatures that recur
_DESIGN = (_U8, [_F32P, _U32, _F64, _F64, _U32])
_INIT_TAPS = (_U8, [_VPP, _F32P, _U32, _U32, _U64, _I32])       # (&ctx, taps, tap count, ratio, max_samples, device)
_DESTROY = (None, [_VP])
_STATUS = (_U8, [_VP])
_LAST_ERROR = (_STR, [_VP])
_SET_U32 = (_U8, [_VP, _U32])
_GET_U32 = (_U32, [_VP])
_SET_U64 = (_U8, [_VP, _U64])
_SET_PTR = (_U8, [_VP, _VP])
_SET_F64 = (_U8, [_VP, _F64])
_F64_ARRAY = (_U8, [_VP, _F64P])                                # one double out, or one per channel / bin in or out
_COUNT = (_U64, [_VP, _U64])
_ALLOC = (_U8, [_VP, _VPP, _U64])
_COPY = (_U8, [_VP, _VP, _VP, _U64])
_PROCESS_F32 = (_U8, [_VP, _VP, _F32P, _U64, _U64P])            # host: (ctx, in, float out, count, &emitted)
_PROCESS_ANY = (_U8, [_VP, _VP, _VP, _U64, _U64P])              # (ctx, in, out, count, &emitted): every counted process_device
_PROCESS_CODES = (_U8, [_VP, _VP, _U64, _U16P, _F32P, _U32P])   # host: (ctx, in, count, codes, powers, &frames)
_PROCESS_CODES_DEVICE = (_U8, [_VP, _VP, _U64, _VP, _VP, _U32P])
_TILE_CONFIG = (_U8, [_VP, _U32, _U32P, _U64])                  # (ctx, grid limit, &tile, position)
_POSITION_CONFIG = (_U8, [_VP, _U32, _U64])                     # (ctx, grid limit, position)
_QUERY_U64 = (_U8, [_VP, _U64, _U64P])                          # (ctx, a count or a budget, what it comes to)
_FFT_TABLES = (_U32, [_F32P, _U32, _U32, _U32, _U32, _F32P, _U32])

ABI = {
    "if_bpf_design": _DESIGN, "if_bpf_design_complex": _DESIGN,
    "if_fir_init": _INIT_TAPS, "if_fir_init_complex": _INIT_TAPS, "if_fir_destroy": _DESTROY, "if_fir_reset": _STATUS,
    "if_fir_set_backend": _SET_U32, "if_fir_get_backend": _GET_U32, "if_fir_set_tuning": _SET_U32, "if_fir_set_input_format": _SET_U32,
    "if_fir_set_stream": _SET_PTR, "if_fir_synchronize": _STATUS, "if_fir_last_error": _LAST_ERROR, "if_fir_out_count": _COUNT,
    "if_fir_process": (_U8, [_VP, _F32P, _F32P, _U64, _U64P]), "if_fir_process_device": _PROCESS_ANY,
    "if_fir_synth_device": (_U8, [_VP, _VP, _U64, _U64, _U32]),
    "if_fir_dev_alloc": _ALLOC, "if_fir_dev_free": _SET_PTR, "if_fir_dev_upload": _COPY, "if_fir_dev_download": _COPY,
    "if_fir_device_info": (_U8, [_VP, _STR, _U32]), "if_fir_set_nco": _SET_F64, "if_fir_get_nco": _F64_ARRAY,
    "if_fir_channelizer_process_device": (_U8, [_VP, _U32, _U32P, _VP, _VPP, _U64, _U64P]),
    "if_fir_channelizer_process_device_freq": (_U8, [_VP, _U32, _F64P, _VP, _VPP, _U64, _U64P]),
    "if_fir_host_alloc": _ALLOC, "if_fir_host_free": _SET_PTR, "if_fir_power_device": (_U8, [_VP, _VP, _U64, _F64P]),
    "if_fir_mc_owner": (_U32, [_U32, _U32]), "if_fir_mc_unique_id": (_U8, [_U8P]),
    "if_fir_mc_init": (_U8, [_VPP, _U32, _F32P, _U32, _U32, _U64, _I32, _U32, _U32, _U8P]),
    "if_fir_mc_destroy": _DESTROY, "if_fir_mc_reset": _STATUS, "if_fir_mc_set_input_format": _SET_U32,
    "if_fir_mc_process_device": (_U8, [_VP, _VPP, _VPP, _U64, _U64P]), "if_fir_mc_channel_ctx": (_VP, [_VP, _U32]),
    "if_fir_mc_last_error": _LAST_ERROR, "if_fir_mc_set_chunk_samples": _SET_U64,
    "if_fir_mc_get_chunk_samples": (_U8, [_VP, _U64P, _U64P]),
}
DEV_ABI = {
    "if_fir_time_device": (_U8, [_VP, _VP, _VP, _U64, _U32, _U32, _F32P]), "if_fir_debug_stamps": (_U32, [_VP, _U64P, _U32]),
    "if_fir_debug_fft_tables": _FFT_TABLES, "if_fir_debug_fft_tables_odd": _FFT_TABLES, "if_fir_debug_fft_tables_bank": _FFT_TABLES,
    "if_fir_debug_bank_plan": (_U8, [_U32P, _U32, _U32P]), "if_fir_debug_bank_tail": (_U32, [_U32, _U32]),
    "if_fir_debug_fft_schedule": (_U8, [_U64, _U32, _U32, _I64P]),
    "if_fir_mc_debug_plan": (_U32, [_U32, _U32, _U32, _U64, _U32, _U32, _U32, _U64, _U64, _U64P, _U32]),
    "if_fir_debug_queue_faults": (_U8, [_VP, _U32P]),
}


def _declare(table, stem, **calls):
    """table[stem + call] = (restype, [argtypes]) for every call=(restype, [argtypes]) given"""
    table.update((stem + call, signature) for call, signature in calls.items())


# the streaming families (_StreamCtx): the calls every one declares alike, then, per family, its own product calls
# (if_fir_<family>_<call>) and its development hooks (if_fir_debug_<family>_<call>)
_FAMILIES = ("interp", "resamp", "psd", "combiner", "ddc", "duc", "arb", "pfb", "synth", "sub", "subup", "rpfb", "rsynth", "fpow", "turn")
_STATELESS = ("turn",)   # the corner turn carries no state: it has no reset
for _family in _FAMILIES:
    _declare(ABI, "if_fir_%s_" % _family, destroy=_DESTROY, synchronize=_STATUS, set_input_format=_SET_U32, set_stream=_SET_PTR,
             last_error=_LAST_ERROR)
    if _family not in _STATELESS:
        _declare(ABI, "if_fir_%s_" % _family, reset=_STATUS)
_declare(ABI, "if_fir_interp_", init=_INIT_TAPS, init_complex=_INIT_TAPS, set_backend=_SET_U32, get_backend=_GET_U32, set_nco=_SET_F64,
         get_nco=_F64_ARRAY, out_count=_COUNT, process=_PROCESS_F32, process_device=_PROCESS_ANY)
_declare(DEV_ABI, "if_fir_debug_interp_", config=(_U8, [_VP, _U32, _U32]), seek=_SET_U64, tables=(_U32, [_F32P, _U32, _U32, _F32P, _U32]),
         plan=(_U8, [_U32, _U32, _U32P, _U32P, _U32P]))
_INIT_RESAMP = (_U8, [_VPP, _F32P, _U32, _U32, _U32, _U64, _I32])
_declare(ABI, "if_fir_resamp_", init=_INIT_RESAMP, init_complex=_INIT_RESAMP, out_count=_COUNT, process=_PROCESS_F32,
         process_device=_PROCESS_ANY)
_declare(DEV_ABI, "if_fir_debug_resamp_", config=(_U8, [_VP, _U32, _U32P]))
_declare(ABI, "if_fir_psd_", init=(_U8, [_VPP, ctypes.POINTER(PsdConfig), _F32P, _U64, _I32]), frame_count=_COUNT,
         process=_PROCESS_CODES, process_device=_PROCESS_CODES_DEVICE)
_declare(DEV_ABI, "if_fir_debug_psd_", plan=_QUERY_U64, config=_POSITION_CONFIG)
_INIT_COMBINER = (_U8, [_VPP, _F32P, _U32, _U32, _U32, _F64P, _U64, _I32])
_declare(ABI, "if_fir_combiner_", init=_INIT_COMBINER, init_complex=_INIT_COMBINER, set_backend=_SET_U32, get_backend=_GET_U32,
         set_centres=_F64_ARRAY, get_centres=_F64_ARRAY, out_count=_COUNT, process=(_U8, [_VP, _VPP, _F32P, _U64, _U64P]),
         process_device=(_U8, [_VP, _VPP, _VP, _U64, _U64P]))
_declare(DEV_ABI, "if_fir_debug_combiner_", config=_SET_U32, seek=_SET_U64,
         tables=(_U32, [_F32P, _U32, _U32, _F64, _U32P, _I32P, _F32P, _U32]))
_declare(ABI, "if_fir_ddc_", init=_INIT_TAPS, init_complex=_INIT_TAPS, set_nco=_SET_F64, get_nco=_F64_ARRAY, out_count=_COUNT,
         process=_PROCESS_F32, process_device=_PROCESS_ANY)
_declare(DEV_ABI, "if_fir_debug_ddc_", config=_TILE_CONFIG)
_declare(ABI, "if_fir_duc_", init=_INIT_TAPS, init_complex=_INIT_TAPS, set_output_format=_SET_U32, set_nco=_SET_F64, get_nco=_F64_ARRAY,
         out_count=_COUNT, process=_PROCESS_ANY, process_device=_PROCESS_ANY)
_declare(DEV_ABI, "if_fir_debug_duc_", config=_TILE_CONFIG)
_declare(ABI, "if_fir_arb_", init=(_U8, [_VPP, _F32P, _U32, _U32, _U64, _U64, _I32]), set_step=_SET_U64, out_count=_COUNT,
         process=_PROCESS_F32, process_device=_PROCESS_ANY, step_from_rates=(_U64, [_F64, _F64]))
_declare(DEV_ABI, "if_fir_debug_arb_", config=(_U8, [_VP, _U32, _U32P, _U64, _U64]))
for _family, _config in (("pfb", PfbConfig), ("rpfb", RpfbConfig)):
    _declare(ABI, "if_fir_%s_" % _family, init=(_U8, [_VPP, ctypes.POINTER(_config), _F32P, _U32, _U64, _I32]), frame_count=_COUNT,
             process=_PROCESS_F32, process_device=_PROCESS_ANY)
    _declare(DEV_ABI, "if_fir_debug_%s_" % _family, config=_TILE_CONFIG)
_declare(ABI, "if_fir_synth_", init=(_U8, [_VPP, ctypes.POINTER(SynthConfig), _F32P, _U32, _U64, _I32]), sample_count=_COUNT,
         process=_PROCESS_F32, process_device=_PROCESS_ANY)
_declare(DEV_ABI, "if_fir_debug_synth_", config=(_U8, [_VP, _U32, _U32, _U32P, _U64]), workspace=_QUERY_U64)
_declare(ABI, "if_fir_rsynth_", init=(_U8, [_VPP, ctypes.POINTER(RsynthConfig), _F32P, _U32, _U64, _I32]), set_output_format=_SET_U32,
         sample_count=_COUNT, process=_PROCESS_ANY, process_device=_PROCESS_ANY)
_declare(DEV_ABI, "if_fir_debug_rsynth_", config=_POSITION_CONFIG, workspace=_QUERY_U64)
for _family, _config in (("sub", SubConfig), ("subup", SubUpConfig)):
    _declare(ABI, "if_fir_%s_" % _family, init=(_U8, [_VPP, ctypes.POINTER(_config), _F32P, _U64, _I32]), set_nco=_F64_ARRAY,
             get_nco=_F64_ARRAY, frame_count=_COUNT, process=_PROCESS_F32, process_device=_PROCESS_ANY)
    _declare(DEV_ABI, "if_fir_debug_%s_" % _family, config=_TILE_CONFIG)
del _family, _config
_declare(ABI, "if_fir_fpow_", init=(_U8, [_VPP, ctypes.POINTER(FpowConfig), _U64, _I32]), frame_count=_COUNT, process=_PROCESS_CODES,
         process_device=_PROCESS_CODES_DEVICE)
_declare(DEV_ABI, "if_fir_debug_fpow_", config=_POSITION_CONFIG)
_TURN = (_U8, [_VP, _VP, _VP, _U64, _U64])
_declare(ABI, "if_fir_turn_", init=(_U8, [_VPP, ctypes.POINTER(TurnConfig), _U32P, _U64, _I32]), set_output_format=_SET_U32,
         process=_TURN, process_device=_TURN)
_declare(DEV_ABI, "if_fir_debug_turn_", config=_SET_U32)

EXPORTS = list(ABI)           # every symbol include/if_fir.h declares (tests check the library exports all of them)
DEV_EXPORTS = list(DEV_ABI)   # every symbol include/if_fir_debug.h declares: exported by libif_fir_dev.so only

_libs = {}


def lib():
    """Load libif_fir.so, the product (raises if it has not been built: there is no fallback)."""
    return _load(LIB_PATH, False)


def dev_lib():
    """Load libif_fir_dev.so: the product's code plus the development hooks of include/if_fir_debug.h."""
    return _load(DEV_LIB_PATH, True)


def _load(path, dev):
    """Open a build of the library and give every symbol of ABI (and, for a development build, of DEV_ABI) its signature."""
    if path in _libs:
        return _libs[path]
    if not os.path.exists(path):
        raise IfFirError("%s is not built (%s); run `python -c 'import __graft_entry__ as g; g.build()'`"
                         % (os.path.basename(path), path))
    L = ctypes.CDLL(path)
    for table in (ABI, DEV_ABI) if dev else (ABI,):
        for name, (restype, argtypes) in table.items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = restype, argtypes
    _libs[path] = L
    return L


def _f32p(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


_DUMMY = np.zeros(2, dtype=np.float32)   # where the pointers of an empty call point: the C side refuses NULL even for no data


def _host_ptr(a, as_type=ctypes.c_void_p):
    """pointer (void *, or as_type) to the data of a host array that a streaming process() sends or fills; _DUMMY if it is empty"""
    return (a if a.size else _DUMMY).ctypes.data_as(as_type)


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
    """What the streaming families share (csrc/if_fir_stream_ctx.h is the C side of it), under that header's rule: nothing here
    branches on which family calls it; a difference comes in as an argument or a class attribute.  The base holds the frame of a
    constructor (_open first, _init last), the context's lifetime, the calls every family has under one name, the host arrays a
    process() sends, the counted process() and process_device() calls, the count query, NO_POSITION and the guard of the
    development hooks.  What only some families have is in the mixins below.  A family sets _FAMILY and keeps what is its own:
    its constructor's arguments and refusals, its process() -- what it allocates and returns -- and its debug calls."""
    _FAMILY = None                 # "interp": the C names are if_fir_interp_<call> and if_fir_debug_interp_<call>
    NO_POSITION = (1 << 64) - 1    # the position of a debug_config that leaves the stream where it is

    def _c(self, call):
        return getattr(self._L, "if_fir_%s_%s" % (self._FAMILY, call))

    def _open(self, dev):
        """First in a constructor: the library, no context yet, float32 in and out."""
        self._L = dev_lib() if dev else lib()
        self._ctx = ctypes.c_void_p()
        self._dev, self._grid_limit = bool(dev), 0
        self._i16 = self._o16 = False
        self._process_device_c = self._c("process_device")   # looked up once: process_device is the call made per chunk

    def _init(self, call, *args):
        """Last in a constructor: <prefix><call>(&context, *args); a refusal leaves no context and raises the library's message."""
        if not self._c(call)(ctypes.byref(self._ctx), *args):
            self._ctx = ctypes.c_void_p()
            raise IfFirError(self._c("last_error")(None).decode())

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

    def _count(self, call, n):
        """<prefix>out_count(), frame_count() or sample_count(): what a call with n inputs emits at the current stream position"""
        return int(self._c(call)(self._ctx, int(n)))

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

    def _frames_input(self, frames):
        """(contiguous array, frame count) of a host (frames, bins) array: complex64 / interleaved float32, or int16 pairs after
        set_input_format(INPUT_I16)"""
        x, n = self._host_input(frames)
        if n % self.bins:
            raise IfFirError("if_fir_%s_process: %d elements are not whole frames of %d bins" % (self._FAMILY, n, self.bins))
        return x, n // self.bins

    def _process_host(self, src, out, count, out_type=_F32P):
        """<prefix>process() in its counted form: `count` units of the host array src in, the host array out (passed as out_type,
        the type the family declares) filled; returns the count the call reports"""
        m = ctypes.c_uint64(0)
        self._check(self._c("process")(self._ctx, _host_ptr(src), _host_ptr(out, out_type), count, ctypes.byref(m)))
        return int(m.value)

    def _process(self, iq):
        """<prefix>process() of a family with one input and one output stream: host array in, interleaved float32 out"""
        iq, n = self._host_input(iq)
        out = np.empty(2 * self.out_count(n), dtype=np.float32)
        m = self._process_host(iq, out, n)
        assert m * 2 == out.size
        return out

    def _process_device(self, dev_in, dev_out, count):
        """<prefix>process_device() in its counted form: raw device pointers (ints), asynchronous; the count the call reports"""
        m = ctypes.c_uint64(0)
        if not self._process_device_c(self._ctx, ctypes.c_void_p(dev_in), ctypes.c_void_p(dev_out), int(count), ctypes.byref(m)):
            self._check(False)   # (asked only on failure: the per-chunk call costs a family no more Python than its own copy did)
        return int(m.value)

    def _debug(self, call):
        """The development hook if_fir_debug_<family>_<call>; refused unless the context was made with dev=True."""
        name = "if_fir_debug_%s_%s" % (self._FAMILY, call)
        if not self._dev:
            raise IfFirError("%s is in the development library only: construct with dev=True" % name)
        return getattr(self._L, name)

    def _position(self, position):
        return self.NO_POSITION if position is None else int(position)

    def _debug_config_tile(self, grid_limit, position):
        """if_fir_debug_<family>_config(context, grid limit, &tile, position): returns the tile (what it counts is the family's)"""
        tile = ctypes.c_uint32(0)
        self._check(self._debug("config")(self._ctx, int(grid_limit), ctypes.byref(tile), self._position(position)))
        self._grid_limit = int(grid_limit)
        return int(tile.value)


class _RealInput:
    """Families that take REAL samples (IfFirDdc, IfFirRpfb)."""

    def _host_input(self, r):
        """(contiguous float32 -- or int16 after set_input_format(INPUT_I16) -- array of REAL samples, sample count)"""
        r = np.ascontiguousarray(r, dtype=np.int16 if self._i16 else np.float32).reshape(-1)
        return r, r.size


class _ScalarNco:
    """Families with one NCO (IfFirInterp, IfFirDdc, IfFirDuc); which way it mixes, and by which index, is the family's."""

    def set_nco(self, freq):
        """<prefix>set_nco(): the NCO frequency in cycles per sample; 0 = off."""
        self._check(self._c("set_nco")(self._ctx, float(freq)))

    def get_nco(self):
        f = ctypes.c_double(0.0)
        self._check(self._c("get_nco")(self._ctx, ctypes.byref(f)))
        return float(f.value)


class _BinNco:
    """Families with one NCO per bin of a frame (IfFirSub, IfFirSubUp)."""

    def set_nco(self, freqs):
        """<prefix>set_nco(): `bins` frequencies in cycles per frame of the family's NCO rate, |f| <= 0.5; None sets every word
        to 0."""
        if freqs is None:
            self._check(self._c("set_nco")(self._ctx, None))
            return
        f = np.ascontiguousarray(freqs, dtype=np.float64).reshape(-1)
        if f.size != self.bins:
            raise IfFirError("if_fir_%s_set_nco: %d frequencies for %d bins" % (self._FAMILY, f.size, self.bins))
        self._check(self._c("set_nco")(self._ctx, f.ctypes.data_as(_F64P)))

    def get_nco(self):
        """<prefix>get_nco(): the quantised frequencies in force, one per bin."""
        f = np.zeros(self.bins, dtype=np.float64)
        self._check(self._c("get_nco")(self._ctx, f.ctypes.data_as(_F64P)))
        return f


class _OutputFormat:
    """Families that can emit int16 (IfFirDuc, IfFirRsynth, IfFirTurn)."""

    def set_output_format(self, fmt):
        """<prefix>set_output_format(): OUTPUT_F32 or OUTPUT_I16 (the float32 result times 2^15, to nearest even, saturated)."""
        self._check(self._c("set_output_format")(self._ctx, int(fmt)))
        self._o16 = (int(fmt) == OUTPUT_I16)


class _CodeFrames:
    """Families that emit frames of uint16 spectrum codes and, optionally, float32 powers (IfFirPsd, IfFirFpow)."""

    def _process_codes(self, src, count, frames, width, want_power):
        """<prefix>process(): `count` units of the host array src in; returns ((frames, width) uint16 codes, float32 powers of
        that shape or None)"""
        codes = np.empty((frames, width), dtype=np.uint16)
        power = np.empty((frames, width), dtype=np.float32) if want_power else None
        m = ctypes.c_uint32(0)
        self._check(self._c("process")(self._ctx, _host_ptr(src), count, codes.ctypes.data_as(_U16P) if frames else None,
                                       _f32p(power) if want_power and frames else None, ctypes.byref(m)))
        assert m.value == frames
        return codes, power

    def _process_codes_device(self, dev_in, count, dev_bins, dev_power):
        """<prefix>process_device(): raw device pointers (ints; dev_power may be 0), asynchronous; the frames emitted"""
        m = ctypes.c_uint32(0)
        self._check(self._process_device_c(self._ctx, ctypes.c_void_p(dev_in or None), int(count), ctypes.c_void_p(dev_bins or None),
                                           ctypes.c_void_p(dev_power or None), ctypes.byref(m)))
        return int(m.value)


class IfFirInterp(_ScalarNco, _StreamCtx):
    """One if_fir_interp_t: upsample by `interpolation`, filter, optionally mix up (docs/SPEC.md §6).  Methods mirror the C
    entry points; N input samples give N * interpolation outputs.  set_nco(f) mixes the OUTPUT up by exp(+j 2 pi f n), n =
    absolute output index."""
    _FAMILY = "interp"

    def __init__(self, taps, interpolation, max_samples=1 << 20, device=0, backend=None, complex_taps=False, dev=False):
        self._open(dev)
        taps, count, complex_taps = _taps_arg(taps, complex_taps)
        self.taps = taps
        self.interpolation = int(interpolation)
        self._init("init_complex" if complex_taps else "init", _f32p(taps), count, self.interpolation, int(max_samples), int(device))
        if backend is not None:
            self.set_backend(backend)

    def set_backend(self, backend):
        self._check(self._c("set_backend")(self._ctx, int(backend)))

    def get_backend(self):
        return int(self._c("get_backend")(self._ctx))

    def out_count(self, samples):
        return self._count("out_count", samples)

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
    _FAMILY = "combiner"

    def __init__(self, taps, interpolation, centres, max_samples=1 << 20, device=0, backend=None, complex_taps=False, dev=False):
        self._open(dev)
        taps, count, complex_taps = _taps_arg(taps, complex_taps)
        centres = np.ascontiguousarray(centres, dtype=np.float64).reshape(-1)
        self.taps = taps
        self.interpolation = int(interpolation)
        self.channels = int(centres.size)
        self._init("init_complex" if complex_taps else "init", _f32p(taps), count, self.interpolation, self.channels,
                   centres.ctypes.data_as(_F64P), int(max_samples), int(device))
        if backend is not None:
            self.set_backend(backend)

    def set_backend(self, backend):
        self._check(self._c("set_backend")(self._ctx, int(backend)))

    def get_backend(self):
        return int(self._c("get_backend")(self._ctx))

    def set_centres(self, centres):
        """if_fir_combiner_set_centres(): all centres at once, from the next call, as if set since the last reset."""
        centres = np.ascontiguousarray(centres, dtype=np.float64).reshape(-1)
        if centres.size != self.channels:
            raise IfFirError("if_fir_combiner_set_centres takes %d centres (got %d)" % (self.channels, centres.size))
        self._check(self._c("set_centres")(self._ctx, centres.ctypes.data_as(_F64P)))

    def get_centres(self):
        f = np.zeros(self.channels, dtype=np.float64)
        self._check(self._c("get_centres")(self._ctx, f.ctypes.data_as(_F64P)))
        return f

    def out_count(self, samples):
        return self._count("out_count", samples)

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
        ptrs = (ctypes.c_void_p * self.channels)(*[_host_ptr(a[0]) for a in arrs])
        self._check(self._c("process")(self._ctx, ptrs, _host_ptr(out, _F32P), n, ctypes.byref(m)))
        assert m.value * 2 == out.size
        return out

    def process_device(self, dev_ins, dev_out, samples):
        """if_fir_combiner_process_device(): raw device pointers (ints), one per channel, asynchronous.  Returns the output
        sample count."""
        if len(dev_ins) != self.channels:
            raise IfFirError("if_fir_combiner_process_device takes %d channels (got %d)" % (self.channels, len(dev_ins)))
        m = ctypes.c_uint64(0)
        ptrs = (ctypes.c_void_p * self.channels)(*[int(p) for p in dev_ins])
        self._check(self._process_device_c(self._ctx, ptrs, ctypes.c_void_p(dev_out), int(samples), ctypes.byref(m)))
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
    _FAMILY = "resamp"

    def __init__(self, taps, interpolation, decimation, max_samples=1 << 20, device=0, complex_taps=False, dev=False):
        self._open(dev)
        taps, count, complex_taps = _taps_arg(taps, complex_taps)
        self.taps = taps
        self.interpolation, self.decimation = int(interpolation), int(decimation)
        self._init("init_complex" if complex_taps else "init", _f32p(taps), count, self.interpolation, self.decimation,
                   int(max_samples), int(device))

    def out_count(self, samples):
        """if_fir_resamp_out_count(): outputs of a call with `samples` inputs at the current stream position."""
        return self._count("out_count", samples)

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
        tile = ctypes.c_uint32(0)
        self._check(self._debug("config")(self._ctx, int(grid_limit), ctypes.byref(tile)))
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
    _FAMILY = "arb"

    def __init__(self, taps, phase_bits, step, max_samples=1 << 20, device=0, dev=False):
        self._open(dev)
        taps = np.ascontiguousarray(taps, dtype=np.float32).reshape(-1)
        self.taps = taps
        self.phase_bits, self._step = int(phase_bits), int(step)
        if not (0 <= self.phase_bits < 1 << 32 and 0 <= self._step < 1 << 64):
            raise IfFirError("if_fir_arb_init: phase bits and step must be unsigned (got %d, %d)" % (self.phase_bits, self._step))
        self._init("init", _f32p(taps), taps.size, self.phase_bits, self._step, int(max_samples), int(device))

    @property
    def step(self):
        """the step in force: input samples per output sample times 2^32"""
        return self._step

    def set_step(self, step):
        """if_fir_arb_set_step(): retune between calls; the position, the time of the next output and the history stay."""
        if not 0 <= int(step) < 1 << 64:
            raise IfFirError("if_fir_arb_set_step: step must be 2^26..2^34 (got %d)" % int(step))
        self._check(self._c("set_step")(self._ctx, int(step)))
        self._step = int(step)

    def out_count(self, samples):
        """if_fir_arb_out_count(): outputs of a call with `samples` inputs at the current position and step."""
        return self._count("out_count", samples)

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
        tile = ctypes.c_uint32(0)
        self._check(self._debug("config")(self._ctx, int(grid_limit), ctypes.byref(tile), self._position(position), int(time_offset)))
        self._grid_limit = int(grid_limit)
        return int(tile.value)

    def tile_outputs(self):
        """outputs one workgroup computes per tile (development library); the grid limit and the position stay as they are"""
        return self.debug_config(self._grid_limit)


class IfFirDdc(_RealInput, _ScalarNco, _StreamCtx):
    """One if_fir_ddc_t: REAL IF samples to decimated complex baseband in one pass -- NCO down-mix, filter, keep every
    decimation-th (docs/SPEC.md §10).  Methods mirror the C entry points; how many outputs a call emits depends on the stream
    position (out_count).  set_nco(f) mixes the input down by exp(-j 2 pi f a), a = absolute sample index."""
    _FAMILY = "ddc"

    def __init__(self, taps, decimation, max_samples=1 << 20, device=0, complex_taps=False, dev=False):
        self._open(dev)
        taps, count, complex_taps = _taps_arg(taps, complex_taps)
        self.taps = taps
        self.decimation = int(decimation)
        self._init("init_complex" if complex_taps else "init", _f32p(taps), count, self.decimation, int(max_samples), int(device))

    def out_count(self, samples):
        """if_fir_ddc_out_count(): outputs of a call with `samples` inputs at the current stream position."""
        return self._count("out_count", samples)

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
        return self._debug_config_tile(grid_limit, position)

    def tile_outputs(self):
        """outputs one workgroup computes per tile (development library); the grid limit stays as it is"""
        return self.debug_config(self._grid_limit)


class IfFirDuc(_ScalarNco, _OutputFormat, _StreamCtx):
    """One if_fir_duc_t: complex baseband to a REAL IF stream at `interpolation` times the rate in one pass -- upsample, filter,
    NCO up-mix, real part, optionally int16 (docs/SPEC.md §11).  Methods mirror the C entry points; N input samples give
    N * interpolation real outputs, float32 or (after set_output_format(OUTPUT_I16)) int16.  set_nco(f) mixes the output up by
    exp(+j 2 pi f m), m = absolute output index, before the real part."""
    _FAMILY = "duc"

    def __init__(self, taps, interpolation, max_samples=1 << 20, device=0, complex_taps=False, dev=False):
        self._open(dev)
        taps, count, complex_taps = _taps_arg(taps, complex_taps)
        self.taps = taps
        self.interpolation = int(interpolation)
        self._init("init_complex" if complex_taps else "init", _f32p(taps), count, self.interpolation, int(max_samples), int(device))

    def out_count(self, samples):
        """if_fir_duc_out_count(): samples * interpolation."""
        return self._count("out_count", samples)

    def process(self, iq):
        """if_fir_duc_process(): host interleaved float32 / complex64 (or int16 pairs after set_input_format(INPUT_I16)) in, real
        float32 (or int16 after set_output_format(OUTPUT_I16)) out."""
        iq, n = self._host_input(iq)
        out = np.empty(self.out_count(n), dtype=np.int16 if self._o16 else np.float32)
        m = self._process_host(iq, out, n, ctypes.c_void_p)
        assert m == out.size
        return out

    def process_device(self, dev_in, dev_out, samples):
        """if_fir_duc_process_device(): raw device pointers (ints), asynchronous.  Returns the output sample count."""
        return self._process_device(dev_in, dev_out, samples)

    def debug_config(self, grid_limit=0, position=None):
        """if_fir_debug_duc_config() (development library: construct with dev=True): at most grid_limit workgroups (0 = the
        launcher's choice); position (optional) = the count of input samples before the next call, with the history zeroed.
        Returns the INPUT samples of one tile of this context."""
        return self._debug_config_tile(grid_limit, position)

    def tile_inputs(self):
        """input samples one workgroup takes per tile (development library); the grid limit stays as it is"""
        return self.debug_config(self._grid_limit)


class IfFirPsd(_CodeFrames, _StreamCtx):
    """One if_fir_psd_t: averaged periodogram of an IQ stream as frames of uint16 spectrum codes, the layout wb_detect reads
    (docs/SPEC.md §8).  Methods mirror the C entry points; how many frames a call emits depends on the stream position
    (frame_count)."""
    _FAMILY = "psd"

    def __init__(self, size, hop, segments, first_bin, bins, ref_power=1.0, window=None, input_format=INPUT_F32,
                 max_samples=1 << 20, device=0, dev=False):
        self._open(dev)
        self.size, self.hop, self.segments, self.first_bin, self.bins = int(size), int(hop), int(segments), int(first_bin), int(bins)
        cfg = PsdConfig(self.size, self.hop, self.segments, self.first_bin, self.bins, float(ref_power), int(input_format))
        self._i16 = (int(input_format) == INPUT_I16)
        wp = None
        if window is not None:
            window = np.ascontiguousarray(window, dtype=np.float32)
            if window.size != self.size:
                raise IfFirError("IfFirPsd: the window must have size = %d values (got %d)" % (self.size, window.size))
            wp = _f32p(window)
        self._init("init", ctypes.byref(cfg), wp, int(max_samples), int(device))

    def frame_count(self, samples):
        """if_fir_psd_frame_count(): frames of a call with `samples` samples at the current stream position."""
        return self._count("frame_count", samples)

    def process(self, iq, want_power=True):
        """if_fir_psd_process(): host interleaved float32 / complex64 (or int16 pairs after set_input_format(INPUT_I16)) in;
        returns ((frames, bins) uint16 codes, (frames, bins) float32 power or None)."""
        iq, n = self._host_input(iq)
        return self._process_codes(iq, n, self.frame_count(n), self.bins, want_power)

    def process_device(self, dev_in, samples, dev_bins, dev_power=0):
        """if_fir_psd_process_device(): raw device pointers (ints; dev_power may be 0), asynchronous.  Returns the frames emitted."""
        return self._process_codes_device(dev_in, samples, dev_bins, dev_power)

    def debug_plan(self, samples):
        """if_fir_debug_psd_plan() (development library: construct with dev=True): (segments, chunks, frames, carried samples)
        of the next call of `samples` samples."""
        out = (ctypes.c_uint64 * 4)()
        self._check(self._debug("plan")(self._ctx, int(samples), out))
        return tuple(int(v) for v in out)

    def debug_config(self, grid_limit=0, position=None):
        """if_fir_debug_psd_config() (development library: construct with dev=True): at most grid_limit workgroups of the chunk
        kernel (0 = the launcher's choice); position (optional) = the stream position of the next call's first sample, the first
        sample of a chunk, with nothing carried and the open frame's accumulator at +0."""
        self._check(self._debug("config")(self._ctx, int(grid_limit), self._position(position)))


class IfFirPfb(_StreamCtx):
    """One if_fir_pfb_t: all `channels` channels of a uniform grid out of one IQ stream in one pass, a frame of `bins` complex64
    values every `hop` input samples (docs/SPEC.md §13).  Methods mirror the C entry points; how many frames a call emits
    depends on the stream position (frame_count)."""
    _FAMILY = "pfb"

    def __init__(self, taps, channels, hop=None, first_bin=0, bins=None, max_samples=1 << 20, device=0, dev=False):
        self._open(dev)
        taps = np.ascontiguousarray(taps, dtype=np.float32).reshape(-1)
        self.taps = taps
        self.channels = int(channels)
        self.hop = self.channels if hop is None else int(hop)
        self.first_bin = int(first_bin)
        self.bins = self.channels if bins is None else int(bins)
        if not all(0 <= v < 1 << 32 for v in (self.channels, self.hop, self.bins)) or not -(1 << 31) <= self.first_bin < 1 << 31:
            raise IfFirError("if_fir_pfb_init: channels, hop and bins must be unsigned, first_bin a 32-bit integer")
        cfg = PfbConfig(self.channels, self.hop, self.first_bin, self.bins)
        self._init("init", ctypes.byref(cfg), _f32p(taps) if taps.size else None, taps.size, int(max_samples), int(device))

    def frame_count(self, samples):
        """if_fir_pfb_frame_count(): frames of a call with `samples` samples at the current stream position."""
        return self._count("frame_count", samples)

    def process(self, iq):
        """if_fir_pfb_process(): host interleaved float32 / complex64 (or int16 pairs after set_input_format(INPUT_I16)) in;
        returns the (frames, bins) complex64 array."""
        iq, n = self._host_input(iq)
        out = np.empty((self.frame_count(n), self.bins), dtype=np.complex64)
        m = self._process_host(iq, out, n)
        assert m == out.shape[0]
        return out

    def process_device(self, dev_in, dev_out, samples):
        """if_fir_pfb_process_device(): raw device pointers (ints), asynchronous.  Returns the frames emitted."""
        return self._process_device(dev_in, dev_out, samples)

    def debug_config(self, grid_limit=0, position=None):
        """if_fir_debug_pfb_config() (development library: construct with dev=True): at most grid_limit workgroups (0 = the
        launcher's choice); position (optional) = the absolute index of the next call's first sample, with the history zeroed.
        Returns the consecutive frames one workgroup owns."""
        return self._debug_config_tile(grid_limit, position)


class IfFirRpfb(_RealInput, _StreamCtx):
    """One if_fir_rpfb_t: the `channels` / 2 + 1 distinct channels of a uniform grid out of one REAL sample stream in one pass, a
    frame of `bins` complex64 values every `hop` input samples (docs/SPEC.md §17).  Methods mirror the C entry points; how many
    frames a call emits depends on the stream position (frame_count)."""
    _FAMILY = "rpfb"

    def __init__(self, taps, channels, hop=None, first_bin=0, bins=None, max_samples=1 << 20, device=0, dev=False):
        self._open(dev)
        taps = np.ascontiguousarray(taps, dtype=np.float32).reshape(-1)
        self.taps = taps
        self.channels = int(channels)
        self.hop = self.channels if hop is None else int(hop)
        self.first_bin = int(first_bin)
        self.bins = self.channels // 2 + 1 - self.first_bin if bins is None else int(bins)
        if not all(0 <= v < 1 << 32 for v in (self.channels, self.hop, self.first_bin, self.bins)):
            raise IfFirError("if_fir_rpfb_init: channels, hop, first_bin and bins must be unsigned 32-bit integers")
        cfg = RpfbConfig(self.channels, self.hop, self.first_bin, self.bins)
        self._init("init", ctypes.byref(cfg), _f32p(taps) if taps.size else None, taps.size, int(max_samples), int(device))

    def frame_count(self, samples):
        """if_fir_rpfb_frame_count(): frames of a call with `samples` samples at the current stream position."""
        return self._count("frame_count", samples)

    def process(self, r):
        """if_fir_rpfb_process(): host float32 (or int16 after set_input_format(INPUT_I16)) real samples in; returns the
        (frames, bins) complex64 array."""
        r, n = self._host_input(r)
        out = np.empty((self.frame_count(n), self.bins), dtype=np.complex64)
        m = self._process_host(r, out, n)
        assert m == out.shape[0]
        return out

    def process_device(self, dev_in, dev_out, samples):
        """if_fir_rpfb_process_device(): raw device pointers (ints), asynchronous.  Returns the frames emitted."""
        return self._process_device(dev_in, dev_out, samples)

    def debug_config(self, grid_limit=0, position=None):
        """if_fir_debug_rpfb_config() (development library: construct with dev=True): at most grid_limit workgroups (0 = the
        launcher's choice); position (optional) = the absolute index of the next call's first sample, with the history zeroed.
        Returns the consecutive frames one workgroup owns."""
        return self._debug_config_tile(grid_limit, position)


class IfFirSynth(_StreamCtx):
    """One if_fir_synth_t: `channels` channel streams on a uniform grid to one IQ stream in one pass, `hop` output samples per
    frame of `bins` values (docs/SPEC.md §14).  Methods mirror the C entry points; its input is what IfFirPfb.process returns."""
    _FAMILY = "synth"
    ROUTE_PLAN, ROUTE_WORKSPACE, ROUTE_LDS = 0, 1, 2

    def __init__(self, taps, channels, hop=None, first_bin=0, bins=None, max_frames=1 << 12, device=0, dev=False):
        self._open(dev)
        taps = np.ascontiguousarray(taps, dtype=np.float32).reshape(-1)
        self.taps = taps
        self.channels = int(channels)
        self.hop = self.channels if hop is None else int(hop)
        self.first_bin = int(first_bin)
        self.bins = self.channels if bins is None else int(bins)
        if not all(0 <= v < 1 << 32 for v in (self.channels, self.hop, self.bins)) or not -(1 << 31) <= self.first_bin < 1 << 31:
            raise IfFirError("if_fir_synth_init: channels, hop and bins must be unsigned, first_bin a 32-bit integer")
        cfg = SynthConfig(self.channels, self.hop, self.first_bin, self.bins)
        self._init("init", ctypes.byref(cfg), _f32p(taps) if taps.size else None, taps.size, int(max_frames), int(device))

    def sample_count(self, frames):
        """if_fir_synth_sample_count(): output samples of a call with `frames` frames at the current stream position."""
        return self._count("sample_count", frames)

    def process(self, frames):
        """if_fir_synth_process(): a host (frames, bins) array in (what IfFirPfb.process returns); interleaved float32 out."""
        x, f = self._frames_input(frames)
        out = np.empty(2 * f * self.hop, dtype=np.float32)
        m = self._process_host(x, out, f)
        assert m * 2 == out.size
        return out

    def process_device(self, dev_in, dev_out, frames):
        """if_fir_synth_process_device(): raw device pointers (ints), asynchronous.  Returns the samples emitted."""
        return self._process_device(dev_in, dev_out, frames)

    def debug_config(self, grid_limit=0, route=0, position=None):
        """if_fir_debug_synth_config() (development library: construct with dev=True): at most grid_limit workgroups per kernel
        (0 = the launcher's choice); route 0 = the plan's choice, 1 = workspace, 2 = LDS (refused where it does not fit);
        position (optional) = the absolute index of the next call's first FRAME, with the history zeroed.  Returns the route in
        use."""
        got = ctypes.c_uint32(0)
        self._check(self._debug("config")(self._ctx, int(grid_limit), int(route), ctypes.byref(got), self._position(position)))
        return int(got.value)

    def debug_workspace(self, nbytes=0):
        """if_fir_debug_synth_workspace() (development library): nbytes > 0 replaces the workspace by one of that budget.
        Returns the frames of a call one chunk emits the outputs of."""
        got = ctypes.c_uint64(0)
        self._check(self._debug("workspace")(self._ctx, int(nbytes), ctypes.byref(got)))
        return int(got.value)


class IfFirRsynth(_OutputFormat, _StreamCtx):
    """One if_fir_rsynth_t: the `channels` / 2 + 1 distinct channels of a uniform grid to one REAL stream in one pass, `hop` real
    output samples per frame of `bins` values (docs/SPEC.md §18).  Methods mirror the C entry points; its input is what
    IfFirRpfb.process returns, its output float32 or (after set_output_format(OUTPUT_I16)) int16."""
    _FAMILY = "rsynth"

    def __init__(self, taps, channels, hop=None, first_bin=0, bins=None, max_frames=1 << 12, device=0, dev=False):
        self._open(dev)
        taps = np.ascontiguousarray(taps, dtype=np.float32).reshape(-1)
        self.taps = taps
        self.channels = int(channels)
        self.hop = self.channels if hop is None else int(hop)
        self.first_bin = int(first_bin)
        self.bins = self.channels // 2 + 1 - self.first_bin if bins is None else int(bins)
        if not all(0 <= v < 1 << 32 for v in (self.channels, self.hop, self.first_bin, self.bins)):
            raise IfFirError("if_fir_rsynth_init: channels, hop, first_bin and bins must be unsigned 32-bit integers")
        cfg = RsynthConfig(self.channels, self.hop, self.first_bin, self.bins)
        self._init("init", ctypes.byref(cfg), _f32p(taps) if taps.size else None, taps.size, int(max_frames), int(device))

    def sample_count(self, frames):
        """if_fir_rsynth_sample_count(): output samples of a call with `frames` frames at the current stream position."""
        return self._count("sample_count", frames)

    def process(self, frames):
        """if_fir_rsynth_process(): a host (frames, bins) array in (what IfFirRpfb.process returns); real float32 (or int16 after
        set_output_format(OUTPUT_I16)) out."""
        x, f = self._frames_input(frames)
        out = np.empty(f * self.hop, dtype=np.int16 if self._o16 else np.float32)
        m = self._process_host(x, out, f, ctypes.c_void_p)
        assert m == out.size
        return out

    def process_device(self, dev_in, dev_out, frames):
        """if_fir_rsynth_process_device(): raw device pointers (ints), asynchronous.  Returns the samples emitted."""
        return self._process_device(dev_in, dev_out, frames)

    def debug_config(self, grid_limit=0, position=None):
        """if_fir_debug_rsynth_config() (development library: construct with dev=True): at most grid_limit workgroups per kernel
        (0 = the launcher's choice); position (optional) = the absolute index of the next call's first FRAME, with the history
        zeroed."""
        self._check(self._debug("config")(self._ctx, int(grid_limit), self._position(position)))

    def debug_workspace(self, nbytes=0):
        """if_fir_debug_rsynth_workspace() (development library): nbytes > 0 replaces the workspace by one of that budget.
        Returns the frames of a call one chunk emits the outputs of."""
        got = ctypes.c_uint64(0)
        self._check(self._debug("workspace")(self._ctx, int(nbytes), ctypes.byref(got)))
        return int(got.value)


class IfFirSub(_BinNco, _StreamCtx):
    """One if_fir_sub_t: the second stage of a two-stage channelizer over frames of `bins` elements (what IfFirPfb.process
    returns and IfFirSynth.process takes): every bin filtered by its own row of `taps` (one row for all bins, or a (bins, T)
    array), decimated by `decimation` and mixed by its own NCO in one pass (docs/SPEC.md §15).  Methods mirror the C entry
    points; how many frames a call emits depends on the stream position (frame_count).  The NCO frequencies (set_nco) are in
    cycles per input frame."""
    _FAMILY = "sub"

    def __init__(self, taps, bins, decimation=1, max_frames=1 << 12, device=0, dev=False, tap_rows=None):
        self._open(dev)
        taps = np.ascontiguousarray(taps, dtype=np.float32)
        self.bins = int(bins)
        self.decimation = int(decimation)
        self.tap_rows = int(tap_rows) if tap_rows is not None else (taps.shape[0] if taps.ndim == 2 else 1)
        self.taps = taps.reshape(-1)
        self.ntaps = self.taps.size // self.tap_rows if self.tap_rows > 0 else 0
        if not all(0 <= v < 1 << 32 for v in (self.bins, self.ntaps, self.tap_rows, self.decimation)):
            raise IfFirError("if_fir_sub_init: bins, taps, tap rows and decimation must be unsigned 32-bit integers")
        cfg = SubConfig(self.bins, self.ntaps, self.tap_rows, self.decimation)
        self._init("init", ctypes.byref(cfg), _f32p(self.taps) if self.taps.size else None, int(max_frames), int(device))

    def frame_count(self, frames):
        """if_fir_sub_frame_count(): output frames of a call with `frames` frames at the current stream position."""
        return self._count("frame_count", frames)

    def process(self, frames):
        """if_fir_sub_process(): a host (frames, bins) array in (complex64 / interleaved float32, or int16 pairs after
        set_input_format(INPUT_I16)); returns the (output frames, bins) complex64 array."""
        x, f = self._frames_input(frames)
        out = np.empty((self.frame_count(f), self.bins), dtype=np.complex64)
        m = self._process_host(x, out, f)
        assert m == out.shape[0]
        return out

    def process_device(self, dev_in, dev_out, frames):
        """if_fir_sub_process_device(): raw device pointers (ints), asynchronous.  Returns the frames emitted."""
        return self._process_device(dev_in, dev_out, frames)

    def debug_config(self, grid_limit=0, position=None):
        """if_fir_debug_sub_config() (development library: construct with dev=True): at most grid_limit workgroups per kernel
        (0 = the launcher's choice); position (optional) = the absolute index of the next call's first FRAME, with the history
        zeroed.  Returns the (output, bin) values one tile holds."""
        return self._debug_config_tile(grid_limit, position)


class IfFirSubUp(_BinNco, _StreamCtx):
    """One if_fir_subup_t: the transmit mirror of IfFirSub over frames of `bins` elements (what IfFirSynth.process takes): every
    bin interpolated by `interpolation` through its own row of `taps` (one row for all bins, or a (bins, T) array) and mixed up
    by its own NCO in one pass (docs/SPEC.md §16).  Methods mirror the C entry points; F frames in give F * interpolation out.
    The NCO frequencies (set_nco) are in cycles per OUTPUT frame."""
    _FAMILY = "subup"

    def __init__(self, taps, bins, interpolation=1, max_frames=1 << 12, device=0, dev=False, tap_rows=None):
        self._open(dev)
        taps = np.ascontiguousarray(taps, dtype=np.float32)
        self.bins = int(bins)
        self.interpolation = int(interpolation)
        self.tap_rows = int(tap_rows) if tap_rows is not None else (taps.shape[0] if taps.ndim == 2 else 1)
        self.taps = taps.reshape(-1)
        self.ntaps = self.taps.size // self.tap_rows if self.tap_rows > 0 else 0
        if not all(0 <= v < 1 << 32 for v in (self.bins, self.ntaps, self.tap_rows, self.interpolation)):
            raise IfFirError("if_fir_subup_init: bins, taps, tap rows and interpolation must be unsigned 32-bit integers")
        cfg = SubUpConfig(self.bins, self.ntaps, self.tap_rows, self.interpolation)
        self._init("init", ctypes.byref(cfg), _f32p(self.taps) if self.taps.size else None, int(max_frames), int(device))

    def frame_count(self, frames):
        """if_fir_subup_frame_count(): output frames of a call with `frames` frames (0 where the call would be refused)."""
        return self._count("frame_count", frames)

    def process(self, frames):
        """if_fir_subup_process(): a host (frames, bins) array in (complex64 / interleaved float32, or int16 pairs after
        set_input_format(INPUT_I16)); returns the (frames * interpolation, bins) complex64 array."""
        x, f = self._frames_input(frames)
        out = np.empty((self.frame_count(f), self.bins), dtype=np.complex64)
        m = self._process_host(x, out, f)
        assert m == out.shape[0]
        return out

    def process_device(self, dev_in, dev_out, frames):
        """if_fir_subup_process_device(): raw device pointers (ints), asynchronous.  Returns the frames emitted."""
        return self._process_device(dev_in, dev_out, frames)

    def debug_config(self, grid_limit=0, position=None):
        """if_fir_debug_subup_config() (development library: construct with dev=True): at most grid_limit workgroups per
        kernel (0 = the launcher's choice); position (optional) = the absolute index of the next call's first INPUT frame, with
        the history zeroed.  Returns the (output, bin) values one tile holds."""
        return self._debug_config_tile(grid_limit, position)


FFT_TABLE_FLOATS = 2 * (4096 + 4096 + 256 + 1024 + 1024 + 64 + 256)


class IfFirFpow(_CodeFrames, _StreamCtx):
    """One if_fir_fpow_t: the power stage over frames of `bins` elements (what IfFirPfb, IfFirRpfb and IfFirSub emit): every
    output bin sums `group` adjacent elements from `first` on, every output frame averages `frames` input frames, and the result
    comes as the uint16 spectrum codes wb_detect reads and, optionally, as float32 powers (docs/SPEC.md §19).  Methods mirror
    the C entry points; how many frames a call emits depends on the stream position (frame_count)."""
    _FAMILY = "fpow"

    def __init__(self, bins, frames, norm=1.0, first=0, group=1, out_bins=None, ref_power=1.0, input_format=INPUT_F32,
                 max_frames=1 << 12, device=0, dev=False):
        self._open(dev)
        self.bins, self.first, self.group, self.frames = int(bins), int(first), int(group), int(frames)
        self.out_bins = int(out_bins) if out_bins is not None else (max(self.bins - self.first, 0) // self.group if self.group > 0 else 0)
        self._i16 = (int(input_format) == INPUT_I16)
        if not all(0 <= v < 1 << 32 for v in (self.bins, self.first, self.group, self.out_bins, self.frames, int(input_format))):
            raise IfFirError("if_fir_fpow_init: bins, first, group, output bins, frames and format must be unsigned 32-bit integers")
        cfg = FpowConfig(self.bins, self.first, self.group, self.out_bins, self.frames, float(norm), float(ref_power), int(input_format))
        self._init("init", ctypes.byref(cfg), int(max_frames), int(device))

    def frame_count(self, frames):
        """if_fir_fpow_frame_count(): output frames of a call with `frames` input frames at the current stream position."""
        return self._count("frame_count", frames)

    def process(self, frames, want_power=True):
        """if_fir_fpow_process(): a host (frames, bins) array in (complex64 / interleaved float32, or int16 pairs after
        set_input_format(INPUT_I16)); returns ((output frames, out_bins) uint16 codes, float32 powers of that shape or None)."""
        x, f = self._frames_input(frames)
        return self._process_codes(x, f, self.frame_count(f), self.out_bins, want_power)

    def process_device(self, dev_in, frames, dev_bins, dev_power=0):
        """if_fir_fpow_process_device(): raw device pointers (ints; dev_power may be 0), asynchronous.  Returns the frames emitted."""
        return self._process_codes_device(dev_in, frames, dev_bins, dev_power)

    def debug_config(self, grid_limit=0, position=None):
        """if_fir_debug_fpow_config() (development library: construct with dev=True): at most grid_limit workgroups per kernel
        (0 = the launcher's choice); position (optional) = the absolute index of the next call's first input FRAME, with the
        carried sums cleared."""
        self._check(self._debug("config")(self._ctx, int(grid_limit), self._position(position)))


TURN_TO_STREAMS, TURN_TO_FRAMES = 0, 1


class IfFirTurn(_OutputFormat, _StreamCtx):
    """One if_fir_turn_t: the corner turn between frames of `bins` elements (the layout of IfFirPfb, IfFirRpfb, IfFirSub, IfFirSubUp,
    IfFirSynth, IfFirRsynth and IfFirFpow) and one contiguous row per listed bin (what the stream families read and write), with
    the format conversion fused (docs/SPEC.md §20; for OUTPUT_I16 a NaN gives 0).  `sel` is a list of distinct bins in any order,
    or None for the span first .. first + channels - 1.  The stage carries no state: there is no reset.  Methods mirror the C
    entry points."""
    _FAMILY = "turn"

    def __init__(self, direction, bins, sel=None, channels=None, first=0, input_format=INPUT_F32, output_format=OUTPUT_F32,
                 max_frames=1 << 12, device=0, dev=False):
        self._open(dev)
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
        self._init("init", ctypes.byref(cfg), arr, int(max_frames), int(device))
        self.sel = list(sel) if sel is not None else list(range(self.first, self.first + self.channels))

    def reset(self):
        raise IfFirError("if_fir_turn_t carries no state: there is no reset")

    def process(self, data, pitch=None, frames=None):
        """if_fir_turn_process(): host arrays.  TO_STREAMS: a (frames, bins) array in (complex64 / interleaved float32, or int16
        pairs after set_input_format(INPUT_I16)), a (channels, pitch, 2) float32 or int16 array out (pitch: default frames), of
        which [:, :frames] is written and the rest is zero.  TO_FRAMES: a (channels, pitch) array of elements in, of which the
        first `frames` (default: pitch) of every row are used, a (frames, bins, 2) array out."""
        odt = np.int16 if self._o16 else np.float32
        if self.direction == TURN_TO_FRAMES:
            x, n = self._host_input(data)
            if n % self.channels:
                raise IfFirError("if_fir_turn_process: %d elements are not %d rows" % (n, self.channels))
            p = n // self.channels
            f = p if frames is None else int(frames)
            out = np.zeros((max(f, 0), self.bins, 2), dtype=odt)
        else:
            x, f = self._frames_input(data)
            p = f if pitch is None else int(pitch)
            out = np.zeros((self.channels, p, 2), dtype=odt)
        self._check(self._c("process")(self._ctx, _host_ptr(x), _host_ptr(out), f, p))
        return out

    def process_device(self, dev_in, dev_out, frames, pitch=None):
        """if_fir_turn_process_device(): raw device pointers (ints), asynchronous; pitch in elements (default: frames)."""
        self._check(self._process_device_c(self._ctx, ctypes.c_void_p(dev_in or None), ctypes.c_void_p(dev_out or None),
                                           int(frames), int(frames if pitch is None else pitch)))

    def debug_config(self, grid_limit=0):
        """if_fir_debug_turn_config() (development library: construct with dev=True): at most grid_limit workgroups (0 = the
        launcher's choice)."""
        self._check(self._debug("config")(self._ctx, int(grid_limit)))


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
    n = dev_lib().if_fir_debug_fft_tables_bank(_f32p(taps), t, 1 if complex_taps else 0, int(bank), int(parity), _f32p(out), out.size)
    if n != FFT_TABLE_FLOATS:
        raise IfFirError("if_fir_debug_fft_tables_bank: (taps=%d, bank=%d) is not served" % (t, bank))
    c = out.view(np.complex64)
    return {"tw1": c[0:4096], "hp": c[4096:8192], "tw2": c[8192:8448], "twd": c[8448:9472], "twe": c[9472:10496], "ncob": c[10496:10560]}


def debug_bank_tail(decimation, own_centres=False):
    """if_fir_debug_bank_tail(): the bank's tail (4, 8, 16) for a decimation, 0 if the bank does not serve it."""
    return int(dev_lib().if_fir_debug_bank_tail(int(decimation), 1 if own_centres else 0))


def debug_bank8_plan(slots):
    """if_fir_debug_bank_plan(): (mask of the even slots' all-slots launch, mask of the odd slots', channels left per channel)."""
    k = len(slots)
    arr = (ctypes.c_uint32 * k)(*[int(v) for v in slots])
    out = (ctypes.c_uint32 * 3)()
    if not dev_lib().if_fir_debug_bank_plan(arr, k, out):
        raise IfFirError("if_fir_debug_bank_plan: 1..16 channels")
    return int(out[0]), int(out[1]), [c for c in range(k) if (out[2] >> c) & 1]


def debug_fft_tables_odd(taps, decimation, complex_taps=False, nco_delta=0):
    """if_fir_debug_fft_tables_odd(): the odd-decimation kernel's table image (decimation 3, 9, 15, ...) as complex64 sections."""
    taps = np.ascontiguousarray(taps, dtype=np.float32)
    t = taps.size // 2 if complex_taps else taps.size
    nfl = 10496 + 512
    out = np.zeros(nfl, dtype=np.float32)
    n = dev_lib().if_fir_debug_fft_tables_odd(_f32p(taps), t, 1 if complex_taps else 0, int(decimation), int(nco_delta) & 0xFFFFFFFF,
                                              _f32p(out), out.size)
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
