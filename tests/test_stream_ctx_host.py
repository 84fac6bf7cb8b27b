"""The C ABI the three streaming contexts share (if_fir_interp_t, if_fir_resamp_t, if_fir_psd_t; csrc/if_fir_stream_ctx.h), as far as
it answers without a device: every refusal of the three inits word for word, in the product and in the development library; the
calls that return 0 for a NULL context; one init message per family.  All of it returns before the device is asked for."""
import ctypes

import numpy as np
import pytest

DEVS = [False, True]
TAPS = np.linspace(-1.0, 1.0, 4097, dtype=np.float32)   # room for the one tap too many
PSD_OK = dict(size=1024, hop=512, segments=4, first_bin=-100, bins=200, ref_power=1.0, input_format=0, max_samples=4096)


def load(fir, dev):
    return fir.dev_lib() if dev else fir.lib()


def f32p(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def interp_init(L, T=15, interpolation=4, max_samples=1024):
    ctx = ctypes.c_void_p()
    return L.if_fir_interp_init(ctypes.byref(ctx), f32p(TAPS), T, interpolation, max_samples, 0), ctx


def resamp_init(L, T=15, interpolation=3, decimation=2, max_samples=1024):
    ctx = ctypes.c_void_p()
    return L.if_fir_resamp_init(ctypes.byref(ctx), f32p(TAPS), T, interpolation, decimation, max_samples, 0), ctx


def psd_init(fir, L, window=None, **changes):
    a = dict(PSD_OK, **changes)
    cfg = fir.PsdConfig(a["size"], a["hop"], a["segments"], a["first_bin"], a["bins"], a["ref_power"], a["input_format"])
    ctx = ctypes.c_void_p()
    return L.if_fir_psd_init(ctypes.byref(ctx), ctypes.byref(cfg), None if window is None else f32p(window), a["max_samples"], 0), ctx


def refused(L, family, ok, ctx):
    """the message of a refused init, without its "if_fir_<family>_init: "; no context is handed out"""
    assert ok == 0 and not ctx.value
    msg = getattr(L, "if_fir_%s_last_error" % family)(None).decode()
    head = "if_fir_%s_init: " % family
    assert msg.startswith(head), msg
    return msg[len(head):]


@pytest.mark.parametrize("dev", DEVS)
@pytest.mark.parametrize("args,message", [
    (dict(T=0), "taps must be 1..4096 (got 0)"),
    (dict(T=4097), "taps must be 1..4096 (got 4097)"),
    (dict(interpolation=0), "interpolation must be 1..64 (got 0)"),
    (dict(interpolation=65), "interpolation must be 1..64 (got 65)"),
    (dict(max_samples=0), "ullMaxSamples must be 1..2^40/L (got 0)"),
    (dict(interpolation=2, max_samples=(1 << 39) + 1), "ullMaxSamples must be 1..2^40/L (got 549755813889)"),
])
def test_interp_init_refusals(fir, dev, args, message):
    L = load(fir, dev)
    assert refused(L, "interp", *interp_init(L, **args)) == message


@pytest.mark.parametrize("dev", DEVS)
@pytest.mark.parametrize("args,message", [
    (dict(T=0), "taps must be 1..4096 (got 0)"),
    (dict(interpolation=0), "interpolation must be 1..64 (got 0)"),
    (dict(interpolation=65), "interpolation must be 1..64 (got 65)"),
    (dict(max_samples=0), "ullMaxSamples must be 1..2^40/L (got 0)"),
    (dict(decimation=0), "decimation must be 1..64 (got 0)"),
    (dict(decimation=65), "decimation must be 1..64 (got 65)"),
])
def test_resamp_init_refusals(fir, dev, args, message):
    L = load(fir, dev)
    assert refused(L, "resamp", *resamp_init(L, **args)) == message


NAN_WINDOW = np.ones(1024, dtype=np.float32)
NAN_WINDOW[0] = np.nan


@pytest.mark.parametrize("dev", DEVS)
@pytest.mark.parametrize("window,args,message", [
    (None, dict(size=1000), "transform size must be 256, 512, 1024, 2048 or 4096 (got 1000)"),
    (None, dict(hop=0), "hop must be 1..1024 (got 0)"),
    (None, dict(hop=1025), "hop must be 1..1024 (got 1025)"),
    (None, dict(segments=0), "segments per frame must be 1..65535 (got 0)"),
    (None, dict(first_bin=-513, bins=200), "bins [-513, -313) are outside [-512, 512) (ulBins 1..1024)"),
    (None, dict(ref_power=0.0), "fRefPower must be a finite value > 0"),
    (None, dict(input_format=2), "unknown input format 2"),
    (None, dict(max_samples=0), "ullMaxSamples must be 1..2^40 (got 0)"),
    (NAN_WINDOW, dict(), "window value 0 is not finite"),
    (np.zeros(1024, dtype=np.float32), dict(), "the window is all zero"),
])
def test_psd_init_refusals(fir, dev, window, args, message):
    L = load(fir, dev)
    assert refused(L, "psd", *psd_init(fir, L, window, **args)) == message


@pytest.mark.parametrize("dev", DEVS)
def test_valid_arguments_without_a_device(fir, dev):
    """with nothing to refuse, an init fails only where there is no device, and then says so (where there is one, it succeeds)"""
    L = load(fir, dev)
    for family, (ok, ctx) in (("interp", interp_init(L)), ("resamp", resamp_init(L)), ("psd", psd_init(fir, L))):
        if ok:
            getattr(L, "if_fir_%s_destroy" % family)(ctx)
        else:
            assert refused(L, family, ok, ctx) == "no HIP device"


@pytest.mark.parametrize("dev", DEVS)
def test_null_context_returns_zero(fir, dev):
    L = load(fir, dev)
    for family in ("interp", "resamp", "psd"):
        call = lambda name: getattr(L, "if_fir_%s_%s" % (family, name))
        assert call("reset")(None) == 0
        assert call("synchronize")(None) == 0
        assert call("set_stream")(None, None) == 0
        assert call("set_input_format")(None, 0) == 0
    assert L.if_fir_interp_out_count(None, 1000) == 0
    assert L.if_fir_resamp_out_count(None, 1000) == 0
    assert L.if_fir_psd_frame_count(None, 1 << 20) == 0


@pytest.mark.parametrize("dev", DEVS)
def test_each_family_keeps_its_own_init_message(fir, dev):
    L = load(fir, dev)
    assert refused(L, "psd", *psd_init(fir, L, hop=0)) == "hop must be 1..1024 (got 0)"
    assert refused(L, "resamp", *resamp_init(L, decimation=0)) == "decimation must be 1..64 (got 0)"
    assert refused(L, "interp", *interp_init(L, interpolation=0)) == "interpolation must be 1..64 (got 0)"
    assert L.if_fir_resamp_last_error(None).decode() == "if_fir_resamp_init: decimation must be 1..64 (got 0)"
    assert L.if_fir_interp_last_error(None).decode() == "if_fir_interp_init: interpolation must be 1..64 (got 0)"
    assert L.if_fir_psd_last_error(None).decode() == "if_fir_psd_init: hop must be 1..1024 (got 0)"
