"""What the nine streaming contexts' C-ABI shims (csrc/if_fir_*_shim.cpp over csrc/if_fir_stream_ctx.h) do alike on a call, on the
GPU, through the raw C ABI: every per-call refusal word for word (a device pointer off by one byte, a NULL pointer, a host call
above init's maximum, a NULL host buffer), that a refused call leaves the stream where it was (the next calls' counts and
outputs are bit-equal to those of a context that was never refused), the empty call, and reset (the history-zeroing path).
One context of the smallest legal shape per family; every refused call returns before a launch."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
FAMILIES = ("interp", "combiner", "resamp", "psd", "ddc", "duc", "arb", "pfb", "synth")
N1, N2, N3 = 301, 211, 97     # units (samples; frames for synth) of the three calls: odd, no multiple of a tile
MAX = 512                     # init's ullMaxSamples / ullMaxFrames
vp = ctypes.c_void_p


def f32p(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


class Family:
    """One family's calls under common names.  A unit is an input sample (a frame of `bins` values for synth); in_bytes is
    its size, out_bytes that of one counted output (sample or frame)."""

    def __init__(self, fir, name):
        self.fir, self.name = fir, name
        self.L = fir.lib() if name == "psd" else fir.dev_lib()    # psd has no grid-limit hook
        self.taps = np.linspace(-1.0, 1.0, 131, dtype=np.float32)
        self.channels = 2 if name == "combiner" else 1
        self.in_bytes = dict(ddc=4, synth=32 * 8).get(name, 8)
        self.out_bytes = dict(duc=4, pfb=32 * 8, psd=128 * 2).get(name, 8)
        self.counter = dict(psd="frame_count", pfb="frame_count", synth="sample_count").get(name, "out_count")
        self.noun = "frames" if name == "synth" else "samples"

    def c(self, call):
        return getattr(self.L, "if_fir_%s_%s" % (self.name, call))

    def open(self):
        L, ctx, t = self.L, vp(), f32p(self.taps)
        ok = dict(
            interp=lambda: L.if_fir_interp_init(ctypes.byref(ctx), t, 15, 4, MAX, 0),
            combiner=lambda: L.if_fir_combiner_init(ctypes.byref(ctx), t, 15, 4, 2, (ctypes.c_double * 2)(0.1, -0.2), MAX, 0),
            resamp=lambda: L.if_fir_resamp_init(ctypes.byref(ctx), t, 15, 3, 2, MAX, 0),
            psd=lambda: L.if_fir_psd_init(ctypes.byref(ctx), ctypes.byref(self.fir.PsdConfig(256, 32, 2, -64, 128, 1.0, 0)), None, MAX, 0),
            ddc=lambda: L.if_fir_ddc_init(ctypes.byref(ctx), t, 15, 4, MAX, 0),
            duc=lambda: L.if_fir_duc_init(ctypes.byref(ctx), t, 15, 4, MAX, 0),
            arb=lambda: L.if_fir_arb_init(ctypes.byref(ctx), t, 31, 4, 3 << 31, MAX, 0),
            pfb=lambda: L.if_fir_pfb_init(ctypes.byref(ctx), ctypes.byref(self.fir.PfbConfig(64, 32, -16, 32)), t, 131, MAX, 0),
            synth=lambda: L.if_fir_synth_init(ctypes.byref(ctx), ctypes.byref(self.fir.SynthConfig(64, 32, -16, 32)), t, 131, MAX, 0),
        )[self.name]()
        assert ok and ctx.value, self.c("last_error")(None).decode()
        # more than one block per launch where the family has the hook: a grid of 3
        hook = dict(
            interp=lambda: L.if_fir_debug_interp_config(ctx, 0, 3), combiner=lambda: L.if_fir_debug_combiner_config(ctx, 3),
            resamp=lambda: L.if_fir_debug_resamp_config(ctx, 3, None), ddc=lambda: L.if_fir_debug_ddc_config(ctx, 3, None, 2 ** 64 - 1),
            duc=lambda: L.if_fir_debug_duc_config(ctx, 3, None, 2 ** 64 - 1), arb=lambda: L.if_fir_debug_arb_config(ctx, 3, None, 2 ** 64 - 1, 0),
            pfb=lambda: L.if_fir_debug_pfb_config(ctx, 3, None, 2 ** 64 - 1), synth=lambda: L.if_fir_debug_synth_config(ctx, 3, 0, None, 2 ** 64 - 1),
        ).get(self.name)
        assert hook is None or hook() == 1, self.error(ctx)
        return ctx

    def error(self, ctx):
        return self.c("last_error")(ctx).decode()

    def count(self, ctx, n):
        return int(self.c(self.counter)(ctx, n))

    def device(self, ctx, ins, out, n, power=None):
        """process_device: ins = one device address per channel, out = the output's (psd: the codes'); (status, count)"""
        m = ctypes.c_uint32(77) if self.name == "psd" else ctypes.c_uint64(77)
        if self.name == "psd":
            ok = self.c("process_device")(ctx, vp(ins[0]), n, vp(out), vp(power), ctypes.byref(m))
        elif self.name == "combiner":
            ok = self.c("process_device")(ctx, (vp * 2)(*ins), vp(out), n, ctypes.byref(m))
        else:
            ok = self.c("process_device")(ctx, vp(ins[0]), vp(out), n, ctypes.byref(m))
        return ok, int(m.value)

    def host(self, ctx, ins, out, n):
        """process: ins = one host array (or None) per channel, out = a host array (or None); (status, count)"""
        m = ctypes.c_uint32(77) if self.name == "psd" else ctypes.c_uint64(77)
        ptr = [vp(a.ctypes.data) if a is not None else None for a in ins]
        if self.name == "psd":
            ok = self.c("process")(ctx, ptr[0], n, None if out is None else out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint16)), None,
                                   ctypes.byref(m))
        elif self.name == "combiner":
            ok = self.c("process")(ctx, (vp * 2)(*ptr), None if out is None else f32p(out), n, ctypes.byref(m))
        elif self.name == "duc":
            ok = self.c("process")(ctx, ptr[0], None if out is None else vp(out.ctypes.data), n, ctypes.byref(m))
        else:
            ok = self.c("process")(ctx, ptr[0], None if out is None else f32p(out), n, ctypes.byref(m))
        return ok, int(m.value)

    def alignment_message(self, ctx):
        who = "if_fir_%s_process_device: " % self.name
        if self.name in ("interp", "combiner"):
            fft = self.c("get_backend")(ctx) == self.fir.BACKEND_HIP_FFT
            return who + "device pointers must be %d-byte (input) and %d-byte (output) aligned for this backend" % ((8, 8) if fft else (16, 16))
        if self.name == "psd":
            return who + "device pointers must be aligned to one element: 8-byte (input), 2-byte (codes), 4-byte (power)"
        noun = "element" if self.name in ("duc", "synth") else "sample"
        return who + "device pointers must be aligned to one %s: %d-byte (input) and %d-byte (output)" % (
            noun, 4 if self.name == "ddc" else 8, 4 if self.name == "duc" else 8)


class Stream:
    """a context with its device buffers; run() makes one device call of input units [first, first + n) and returns
    (count, the output's bytes)"""

    def __init__(self, fam, x):
        self.fam, self.ctx = fam, fam.open()
        self.x = [torch.from_numpy(ch).cuda() for ch in x]
        self.out = torch.zeros(MAX * 64 * 8, dtype=torch.uint8, device="cuda")
        self.power = torch.zeros(MAX * 64 * 8, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()

    def close(self):
        self.fam.c("destroy")(self.ctx)

    def ins(self, first):
        return [ch.data_ptr() + first * self.fam.in_bytes for ch in self.x]

    def run(self, first, n):
        fam = self.fam
        want = fam.count(self.ctx, n)
        self.out.zero_()
        torch.cuda.synchronize()
        ok, m = fam.device(self.ctx, self.ins(first), self.out.data_ptr(), n, self.power.data_ptr())
        assert ok == 1 and m == want, fam.error(self.ctx)
        assert fam.c("synchronize")(self.ctx) == 1
        return m, self.out[:m * fam.out_bytes].cpu().numpy().tobytes()

    def run_host(self, x, first, n):
        fam = self.fam
        want = fam.count(self.ctx, n)
        out = np.zeros(MAX * 64 * 2, dtype=np.float32)
        ok, m = fam.host(self.ctx, [np.ascontiguousarray(ch[first * fam.in_bytes:(first + n) * fam.in_bytes]) for ch in x], out, n)
        assert ok == 1 and m == want, fam.error(self.ctx)
        return m, out.tobytes()[:m * fam.out_bytes]


def refuse(fam, ctx, result, message):
    ok, m = result
    assert ok == 0 and fam.error(ctx) == message, (ok, fam.error(ctx))


@pytest.mark.parametrize("name", FAMILIES)
def test_refused_calls_leave_the_stream_where_it_was(fir, gpu_ok, name):
    fam = Family(fir, name)
    rng = np.random.default_rng(20)
    units = N1 + N2 + N3
    # float32 inputs as bytes, one array per channel (the combiner has two)
    x = [rng.standard_normal(units * fam.in_bytes // 4).astype(np.float32).view(np.uint8) for _ in range(fam.channels)]
    a, b = Stream(fam, x), Stream(fam, x)
    try:
        first = a.run(0, N1)
        assert first == b.run(0, N1) and any(first[1])
        ctx, ins, out, power = a.ctx, a.ins(N1), a.out.data_ptr(), a.power.data_ptr()
        assert fam.count(ctx, N2) > 0    # outputs are due, so a missing output pointer is refused
        dev, hst = "if_fir_%s_process_device: " % name, "if_fir_%s_process: " % name
        refuse(fam, ctx, fam.device(ctx, [ins[0] + 1] + ins[1:], out, N2, power), fam.alignment_message(ctx))
        refuse(fam, ctx, fam.device(ctx, ins[:-1] + [ins[-1] + 1], out, N2, power), fam.alignment_message(ctx))
        refuse(fam, ctx, fam.device(ctx, ins, out + 1, N2, power), fam.alignment_message(ctx))
        refuse(fam, ctx, fam.device(ctx, [None] + ins[1:], out, N2, power), dev + "NULL device pointer")
        refuse(fam, ctx, fam.device(ctx, ins[:-1] + [None], out, N2, power), dev + "NULL device pointer")
        refuse(fam, ctx, fam.device(ctx, ins, None, N2, power), dev + "NULL device pointer")
        if name == "psd":
            refuse(fam, ctx, fam.device(ctx, ins, out, N2, power + 2), fam.alignment_message(ctx))
        hx = [np.zeros(16, dtype=np.uint8) for _ in x]     # never read: the count is refused first
        hout = np.zeros(16, dtype=np.float32)
        refuse(fam, ctx, fam.host(ctx, hx, hout, MAX + 1),
               hst + "%d %s exceed %s %d of init" % (MAX + 1, fam.noun, "ullMaxFrames" if name == "synth" else "ullMaxSamples", MAX))
        refuse(fam, ctx, fam.host(ctx, [None] + hx[1:], hout, N2), hst + "NULL buffer")
        refuse(fam, ctx, fam.host(ctx, hx[:-1] + [None], hout, N2), hst + "NULL buffer")
        refuse(fam, ctx, fam.host(ctx, hx, None, N2), hst + "NULL buffer")
        # the empty call: 1, a count of 0, and nothing moves
        assert fam.device(ctx, ins, out, 0, power) == (1, 0), fam.error(ctx)
        assert fam.host(ctx, hx, hout, 0) == (1, 0), fam.error(ctx)
        # the stream is where it was: a device call, then a host call, against the context that was never refused
        second = a.run(N1, N2)
        assert second == b.run(N1, N2) and second[0] > 0 and any(second[1])
        third = a.run_host(x, N1 + N2, N3)
        assert third == b.run_host(x, N1 + N2, N3) and any(third[1])
        # reset zeroes the history: the same input gives a fresh context's bits
        assert fam.c("reset")(ctx) == 1, fam.error(ctx)
        assert a.run(0, N1) == first
    finally:
        a.close()
        b.close()
