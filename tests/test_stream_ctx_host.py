"""The C ABI the nine streaming contexts share (FAMILIES below; csrc/if_fir_stream_ctx.h), as far as it answers without a
device: every refusal of the nine inits word for word, in the product and in the development library; the calls that return 0
for a NULL context; one init message per family.  All of it returns before the device is asked for."""
import ctypes

import numpy as np
import pytest

DEVS = [False, True]
TAPS = np.linspace(-1.0, 1.0, 4097, dtype=np.float32)   # room for the one tap too many
FAMILIES = ("interp", "combiner", "resamp", "psd", "ddc", "duc", "arb", "pfb", "synth")
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


def combiner_init(L, T=15, interpolation=4, channels=2, centres=(0.1, -0.2), max_samples=1024):
    ctx = ctypes.c_void_p()
    c = None if centres is None else (ctypes.c_double * len(centres))(*centres)
    return L.if_fir_combiner_init(ctypes.byref(ctx), f32p(TAPS), T, interpolation, channels, c, max_samples, 0), ctx


def ddc_init(L, T=15, decimation=4, max_samples=1024):
    ctx = ctypes.c_void_p()
    return L.if_fir_ddc_init(ctypes.byref(ctx), f32p(TAPS), T, decimation, max_samples, 0), ctx


def duc_init(L, taps=TAPS, T=15, interpolation=4, max_samples=1024):
    ctx = ctypes.c_void_p()
    return L.if_fir_duc_init(ctypes.byref(ctx), f32p(taps), T, interpolation, max_samples, 0), ctx


def arb_init(L, T=31, phase_bits=4, step=3 << 31, max_samples=1024):
    ctx = ctypes.c_void_p()
    return L.if_fir_arb_init(ctypes.byref(ctx), f32p(np.ones(8193, dtype=np.float32)), T, phase_bits, step, max_samples, 0), ctx


def bank_init(fir, L, family, cfg=True, T=131, channels=64, hop=32, first_bin=-16, bins=32, max_samples=256):
    """pfb or synth: the two banks take the same arguments"""
    ctx = ctypes.c_void_p()
    c = (fir.PfbConfig if family == "pfb" else fir.SynthConfig)(channels, hop, first_bin, bins)
    init = getattr(L, "if_fir_%s_init" % family)
    return init(ctypes.byref(ctx), ctypes.byref(c) if cfg else None, f32p(TAPS), T, max_samples, 0), ctx


def any_init(fir, L, family, **args):
    """the family's init with valid arguments but for **args"""
    if family in ("pfb", "synth"):
        return bank_init(fir, L, family, **args)
    if family == "psd":
        return psd_init(fir, L, **args)
    return globals()[family + "_init"](L, **args)


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


NAN_TAPS = np.ones(15, dtype=np.float32)
NAN_TAPS[7] = np.inf
# what the other six inits refuse before they ask for the device, in the order of their checks
REFUSALS = [
    ("combiner", dict(T=0), "taps must be 1..4096 (got 0)"),
    ("combiner", dict(T=4097), "taps must be 1..4096 (got 4097)"),
    ("combiner", dict(interpolation=0), "interpolation must be 1..64 (got 0)"),
    ("combiner", dict(interpolation=65), "interpolation must be 1..64 (got 65)"),
    ("combiner", dict(channels=0), "channels must be 1..64 (got 0)"),
    ("combiner", dict(channels=65), "channels must be 1..64 (got 65)"),
    ("combiner", dict(max_samples=0), "ullMaxSamples must be 1..2^40/L (got 0)"),
    ("combiner", dict(interpolation=2, max_samples=(1 << 39) + 1), "ullMaxSamples must be 1..2^40/L (got 549755813889)"),
    ("combiner", dict(centres=None), "pdCentre is NULL"),
    ("combiner", dict(centres=(0.1, 0.75)), "centre 1 must be within +-0.5 cycles/sample (got 0.75)"),
    ("combiner", dict(centres=(float("nan"), 0.1)), "centre 0 must be within +-0.5 cycles/sample (got nan)"),
    ("ddc", dict(T=0), "taps must be 1..4096 (got 0)"),
    ("ddc", dict(T=4097), "taps must be 1..4096 (got 4097)"),
    ("ddc", dict(decimation=0), "decimation must be 1..64 (got 0)"),
    ("ddc", dict(decimation=65), "decimation must be 1..64 (got 65)"),
    ("ddc", dict(max_samples=0), "ullMaxSamples must be 1..2^40 (got 0)"),
    ("ddc", dict(max_samples=(1 << 40) + 1), "ullMaxSamples must be 1..2^40 (got 1099511627777)"),
    ("duc", dict(T=0), "taps must be 1..4096 (got 0)"),
    ("duc", dict(T=4097), "taps must be 1..4096 (got 4097)"),
    ("duc", dict(interpolation=0), "interpolation must be 1..64 (got 0)"),
    ("duc", dict(interpolation=65), "interpolation must be 1..64 (got 65)"),
    ("duc", dict(taps=NAN_TAPS), "tap 7 is not finite"),
    ("duc", dict(max_samples=0), "ullMaxSamples must be 1..2^40 (got 0)"),
    ("arb", dict(T=0), "taps must be 1..8192 (got 0)"),
    ("arb", dict(T=8193), "taps must be 1..8192 (got 8193)"),
    ("arb", dict(phase_bits=3), "phase bits must be 4..10 (got 3)"),
    ("arb", dict(phase_bits=11), "phase bits must be 4..10 (got 11)"),
    ("arb", dict(step=(1 << 26) - 1), "step must be 2^26..2^34 (got 67108863)"),
    ("arb", dict(step=(1 << 34) + 1), "step must be 2^26..2^34 (got 17179869185)"),
    ("arb", dict(max_samples=0), "ullMaxSamples must be 1..2^30 (got 0)"),
    ("arb", dict(max_samples=(1 << 30) + 1), "ullMaxSamples must be 1..2^30 (got 1073741825)"),
    ("pfb", dict(cfg=False), "pCfg is NULL"),
    ("pfb", dict(channels=100), "channels must be 64, 128, 256, 512, 1024, 2048 or 4096 (got 100)"),
    ("pfb", dict(T=0), "taps must be 1..1024 = 16 x channels (got 0)"),
    ("pfb", dict(T=1025), "taps must be 1..1024 = 16 x channels (got 1025)"),
    ("pfb", dict(hop=0), "hop must be 1..64 (got 0)"),
    ("pfb", dict(hop=65), "hop must be 1..64 (got 65)"),
    ("pfb", dict(first_bin=-33, bins=64), "the span needs -32 <= lFirstBin < 64 and 1 <= ulBins <= 64 (got -33, 64)"),
    ("pfb", dict(first_bin=0, bins=65), "the span needs -32 <= lFirstBin < 64 and 1 <= ulBins <= 64 (got 0, 65)"),
    ("pfb", dict(max_samples=0), "ullMaxSamples must be 1..2^40 (got 0)"),
    ("synth", dict(cfg=False), "pCfg is NULL"),
    ("synth", dict(channels=100), "channels must be 64, 128, 256, 512, 1024, 2048 or 4096 (got 100)"),
    ("synth", dict(T=0), "taps must be 1..1024 = 16 x channels (got 0)"),
    ("synth", dict(T=1025), "taps must be 1..1024 = 16 x channels (got 1025)"),
    ("synth", dict(hop=0), "hop must be 1..64 (got 0)"),
    ("synth", dict(hop=65), "hop must be 1..64 (got 65)"),
    ("synth", dict(T=100, hop=1), "ceil(taps / hop) must be at most 32 (got 100 taps at hop 1: 100)"),
    ("synth", dict(first_bin=64, bins=1), "the span needs -32 <= lFirstBin < 64 and 1 <= ulBins <= 64 (got 64, 1)"),
    ("synth", dict(bins=0), "the span needs -32 <= lFirstBin < 64 and 1 <= ulBins <= 64 (got -16, 0)"),
    ("synth", dict(max_samples=0), "ullMaxFrames must be 1..2^32 (got 0)"),
    ("synth", dict(max_samples=(1 << 32) + 1), "ullMaxFrames must be 1..2^32 (got 4294967297)"),
]


@pytest.mark.parametrize("dev", DEVS)
@pytest.mark.parametrize("family,args,message", REFUSALS)
def test_init_refusals_of_the_later_families(fir, dev, family, args, message):
    L = load(fir, dev)
    assert refused(L, family, *any_init(fir, L, family, **args)) == message


@pytest.mark.parametrize("dev", DEVS)
def test_missing_pointers_of_every_init(fir, dev):
    """no ppCtx: said first, whatever else is wrong; no taps: said with the count; no configuration"""
    L = load(fir, dev)
    cfg, scfg = fir.PfbConfig(64, 32, -16, 32), fir.SynthConfig(64, 32, -16, 32)
    no_ctx = dict(interp=(None, f32p(TAPS), 0, 4, 1024, 0), combiner=(None, f32p(TAPS), 0, 4, 2, None, 1024, 0),
                  resamp=(None, f32p(TAPS), 0, 3, 2, 1024, 0), psd=(None, None, None, 1024, 0), ddc=(None, f32p(TAPS), 0, 4, 1024, 0),
                  duc=(None, f32p(TAPS), 0, 4, 1024, 0), arb=(None, f32p(TAPS), 0, 4, 3 << 31, 1024, 0),
                  pfb=(None, None, f32p(TAPS), 131, 256, 0), synth=(None, None, f32p(TAPS), 131, 256, 0))
    no_taps = dict(interp=(None, 15, 4, 1024, 0), combiner=(None, 15, 4, 2, None, 1024, 0), resamp=(None, 15, 3, 2, 1024, 0),
                   ddc=(None, 15, 4, 1024, 0), duc=(None, 15, 4, 1024, 0), arb=(None, 31, 4, 3 << 31, 1024, 0),
                   pfb=(ctypes.byref(cfg), None, 131, 256, 0), synth=(ctypes.byref(scfg), None, 131, 256, 0))
    limit = dict(arb="8192", pfb="1024 = 16 x channels", synth="1024 = 16 x channels")
    assert set(no_ctx) == set(FAMILIES)
    for family in FAMILIES:
        init, last = getattr(L, "if_fir_%s_init" % family), getattr(L, "if_fir_%s_last_error" % family)
        assert init(*no_ctx[family]) == 0
        assert last(None).decode() == "if_fir_%s_init: ppCtx is NULL" % family
        ctx = ctypes.c_void_p(1)
        if family == "psd":
            assert init(ctypes.byref(ctx), None, None, 1024, 0) == 0
            assert refused(L, family, 0, ctx) == "pCfg is NULL"
            continue
        assert init(ctypes.byref(ctx), *no_taps[family]) == 0
        count = no_taps[family][1 if family not in ("pfb", "synth") else 2]
        assert refused(L, family, 0, ctx) == "taps must be 1..%s (got %d), pfTaps is NULL" % (limit.get(family, "4096"), count)
    for family in ("interp", "combiner", "resamp", "ddc", "duc"):
        init = getattr(L, "if_fir_%s_init_complex" % family)
        assert init(*no_ctx[family]) == 0
        assert getattr(L, "if_fir_%s_last_error" % family)(None).decode() == "if_fir_%s_init: ppCtx is NULL" % family


@pytest.mark.parametrize("dev", DEVS)
def test_valid_arguments_without_a_device(fir, dev):
    """with nothing to refuse, an init fails only where there is no device, and then says so (where there is one, it succeeds)"""
    L = load(fir, dev)
    for family in FAMILIES:
        ok, ctx = any_init(fir, L, family)
        if ok:
            getattr(L, "if_fir_%s_destroy" % family)(ctx)
        else:
            assert refused(L, family, ok, ctx) == "no HIP device"


@pytest.mark.parametrize("dev", DEVS)
def test_null_context_returns_zero(fir, dev):
    """every entry point that takes a context, of all nine families and of their development hooks"""
    L = load(fir, dev)
    f64, words = ctypes.c_double(0.0), (ctypes.c_uint64 * 4)()
    two = (ctypes.c_double * 2)(0.1, -0.2)
    for family in FAMILIES:
        call = lambda name: getattr(L, "if_fir_%s_%s" % (family, name))
        assert call("reset")(None) == 0
        assert call("synchronize")(None) == 0
        assert call("set_stream")(None, None) == 0
        assert call("set_input_format")(None, 0) == 0
        call("destroy")(None)
        if family == "psd":
            assert call("process")(None, None, 0, None, None, None) == 0
            assert call("process_device")(None, None, 0, None, None, None) == 0
        else:
            assert call("process")(None, None, None, 0, None) == 0
            assert call("process_device")(None, None, None, 0, None) == 0
    for family in ("interp", "combiner", "resamp", "ddc", "duc", "arb"):
        assert getattr(L, "if_fir_%s_out_count" % family)(None, 1000) == 0
    assert L.if_fir_psd_frame_count(None, 1 << 20) == 0
    assert L.if_fir_pfb_frame_count(None, 1 << 20) == 0
    assert L.if_fir_synth_sample_count(None, 1000) == 0
    for family in ("interp", "ddc", "duc"):
        assert getattr(L, "if_fir_%s_set_nco" % family)(None, 0.1) == 0
        assert getattr(L, "if_fir_%s_get_nco" % family)(None, ctypes.byref(f64)) == 0
    for family in ("interp", "combiner"):
        assert getattr(L, "if_fir_%s_set_backend" % family)(None, 0) == 0
        assert getattr(L, "if_fir_%s_get_backend" % family)(None) == 0
    assert L.if_fir_combiner_set_centres(None, two) == 0 and L.if_fir_combiner_get_centres(None, two) == 0
    assert L.if_fir_duc_set_output_format(None, 0) == 0
    assert L.if_fir_arb_set_step(None, 1 << 32) == 0
    if dev:
        assert L.if_fir_debug_interp_config(None, 0, 0) == 0 and L.if_fir_debug_interp_seek(None, 0) == 0
        assert L.if_fir_debug_combiner_config(None, 0) == 0 and L.if_fir_debug_combiner_seek(None, 0) == 0
        assert L.if_fir_debug_resamp_config(None, 0, None) == 0
        assert L.if_fir_debug_psd_plan(None, 1000, words) == 0
        assert L.if_fir_debug_ddc_config(None, 0, None, 0) == 0 and L.if_fir_debug_duc_config(None, 0, None, 0) == 0
        assert L.if_fir_debug_arb_config(None, 0, None, 0, 0) == 0
        assert L.if_fir_debug_pfb_config(None, 0, None, 0) == 0
        assert L.if_fir_debug_synth_config(None, 0, 0, None, 0) == 0 and L.if_fir_debug_synth_workspace(None, 0, None) == 0


@pytest.mark.parametrize("dev", DEVS)
def test_each_family_keeps_its_own_init_message(fir, dev):
    L = load(fir, dev)
    said = dict(psd=(dict(hop=0), "hop must be 1..1024 (got 0)"), resamp=(dict(decimation=0), "decimation must be 1..64 (got 0)"),
                interp=(dict(interpolation=0), "interpolation must be 1..64 (got 0)"), combiner=(dict(channels=0), "channels must be 1..64 (got 0)"),
                ddc=(dict(decimation=65), "decimation must be 1..64 (got 65)"), duc=(dict(interpolation=65), "interpolation must be 1..64 (got 65)"),
                arb=(dict(phase_bits=3), "phase bits must be 4..10 (got 3)"), pfb=(dict(hop=0), "hop must be 1..64 (got 0)"),
                synth=(dict(hop=65), "hop must be 1..64 (got 65)"))
    assert set(said) == set(FAMILIES)
    for family, (args, message) in said.items():
        assert refused(L, family, *any_init(fir, L, family, **args)) == message
    for family, (args, message) in said.items():
        assert getattr(L, "if_fir_%s_last_error" % family)(None).decode() == "if_fir_%s_init: %s" % (family, message)


