"""Full-size (BASELINE.json configs[1], configs[2]) property tests on the GPU: the oracle cannot run 2^28 samples in
seconds, so parity is checked (a) exactly on windows of the stream against the oracle, (b) through size-independent
properties: one call ≡ two calls at an odd split (tile placement independence, history/phase carry), and a checksum
of the whole output that must not depend on the split."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
SEG = dict(seg_mode=1, seg_len=32)


@pytest.mark.parametrize("t,d,log2n", [(127, 1, 26), (255, 4, 28), (255, 1, 26)])
def test_full_size_windows_and_split_invariance(fir, oracle, gpu_ok, t, d, log2n):
    import torch
    torch.cuda.set_device(0)
    n = 1 << log2n
    taps = fir.bpf_design(t)
    with fir.IfFir(taps, d, 0, backend=fir.BACKEND_HIP_DIRECT) as f:
        x = torch.empty(2 * n, dtype=torch.float32, device="cuda")
        m = f.out_count(n)
        y = torch.empty(2 * m, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        f.synth_device(x.data_ptr(), 0, n, 0)
        assert f.process_device(x.data_ptr(), y.data_ptr(), n) == m
        f.synchronize()
        # (a) windows: start, tile seams, an arbitrary interior place, the very end
        w = 4096
        for start in [0, 8192 - 100, (n // 3) & ~3, n - w]:
            lo = max(0, start - (t - 1))
            xs = x[2 * lo:2 * (start + w)].cpu().numpy()
            assert np.array_equal(xs, oracle.synth_iq(start + w - lo, 0, lo))
            hist = np.zeros(2 * (t - 1), dtype=np.float32)
            hist[2 * (t - 1 - (start - lo)):] = xs[:2 * (start - lo)]
            model = oracle.fir_f32fma(taps, xs[2 * (start - lo):], d, hist, start, **SEG)
            first_out = (start + d - 1) // d
            got = y[2 * first_out:2 * first_out + model.size].cpu().numpy()
            assert np.array_equal(got, model), (start, np.max(np.abs(got - model)))
            ref = oracle.fir_f64(taps, xs[2 * (start - lo):], d, hist, start)
            l2, mx = oracle.err_metrics(got, ref)
            assert l2 <= 1e-6 and mx <= 1e-6
        # (b) split invariance + checksum
        ck1 = y.double().sum().item()
        ab1 = y.double().abs().sum().item()
        y2 = torch.empty_like(y)
        f.reset()
        cut = (n // 2) + 12345   # odd: second call starts off-phase and misaligned
        m1 = f.process_device(x.data_ptr(), y2.data_ptr(), cut)
        m2 = f.process_device(x.data_ptr() + 8 * cut, y2.data_ptr() + 8 * m1, n - cut) if cut % 2 == 0 else None
        if m2 is None:
            # device pointers must stay 16-byte aligned: move the tail to an aligned buffer
            tail = x[2 * cut:].clone()
            torch.cuda.synchronize()
            ytail = torch.empty(2 * (m - m1), dtype=torch.float32, device="cuda")
            m2 = f.process_device(tail.data_ptr(), ytail.data_ptr(), n - cut)
            f.synchronize()
            y2[2 * m1:] = ytail
        f.synchronize()
        assert m1 + m2 == m
        assert torch.equal(y, y2)
        assert y2.double().sum().item() == ck1 and y2.double().abs().sum().item() == ab1 and ab1 > 0


@pytest.mark.parametrize("t,d,log2n", [(255, 4, 28), (1023, 1, 28), (127, 1, 26),
                                       (255, 2, 28), (255, 8, 28), (511, 16, 28), (1023, 32, 28), (255, 64, 28),
                                       (255, 12, 28), (255, 24, 28)])
def test_full_size_fft_backend(fir, oracle, gpu_ok, t, d, log2n):
    """Overlap-save backend (AUTO) at BASELINE sizes: windows of the stream within SPEC tolerance of the float64 oracle,
    and split invariance (one call vs two calls at an odd cut) within tolerance of each other.  Decimations 2, 8, 16, 32
    and 64 are the decimating tails of round 3 (frequency-domain alias fold + small inverse) at the same size."""
    import torch
    torch.cuda.set_device(0)
    n = 1 << log2n
    taps = fir.bpf_design(t)
    with fir.IfFir(taps, d, 0) as f:
        assert f.get_backend() == fir.BACKEND_HIP_FFT
        x = torch.empty(2 * n, dtype=torch.float32, device="cuda")
        m = f.out_count(n)
        y = torch.empty(2 * m, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        f.synth_device(x.data_ptr(), 0, n, 0)
        assert f.process_device(x.data_ptr(), y.data_ptr(), n) == m
        f.synchronize()
        w = 8192
        for start in [0, 3840 * 7 - 100, (n // 3) & ~3, n - w]:
            lo = max(0, start - (t - 1))
            xs = x[2 * lo:2 * (start + w)].cpu().numpy()
            hist = np.zeros(2 * (t - 1), dtype=np.float32)
            hist[2 * (t - 1 - (start - lo)):] = xs[:2 * (start - lo)]
            ref = oracle.fir_f64(taps, xs[2 * (start - lo):], d, hist, start)
            first_out = (start + d - 1) // d
            got = y[2 * first_out:2 * first_out + ref.size].cpu().numpy()
            l2, mx = oracle.err_metrics(got, ref)
            assert l2 <= 1e-6 and mx <= 1e-6, (start, l2, mx)
        # completeness: EVERY output of the launch against the direct form (or the one-output-per-thread kernel) on the
        # same input -- windows alone can miss blocks a work-queue bug leaves unwritten
        f.reset()
        f.set_backend(fir.BACKEND_HIP_DIRECT if (t, d) in ((255, 4), (127, 1)) else fir.BACKEND_HIP_GENERIC)
        yd = torch.empty_like(y)
        assert f.process_device(x.data_ptr(), yd.data_ptr(), n) == m
        f.synchronize()
        scale = yd.abs().max().item()
        assert scale > 0.1
        assert (y - yd).abs().max().item() <= 2e-6 * scale   # each side is within 1e-6 of the float64 result
        del yd
        f.set_backend(fir.BACKEND_HIP_FFT)
        f.reset()
        cut = (n // 2) + 12345
        y2 = torch.empty_like(y)
        m1 = f.process_device(x.data_ptr(), y2.data_ptr(), cut)
        tail = x[2 * cut:].clone()
        ytail = torch.empty(2 * (m - m1), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        m2 = f.process_device(tail.data_ptr(), ytail.data_ptr(), n - cut)
        f.synchronize()
        assert m1 + m2 == m
        y2[2 * m1:] = ytail
        scale = y.abs().max().item()
        assert (y - y2).abs().max().item() <= 1e-6 * scale   # block placement differs, values agree to tolerance


def test_full_size_nco_and_index_wrap(fir, oracle, gpu_ok):
    """NCO at BASELINE size (SPEC §3.2): every output against the generic kernel, windows against the float64 oracle;
    then the stream is continued past 2^32 samples (17 calls of 2^28) so that the 32-bit phase arithmetic of the
    kernels wraps: a window of the last call against the oracle at consumed = 16 * 2^28."""
    import torch
    torch.cuda.set_device(0)
    t, d, n = 255, 4, 1 << 28
    taps = fir.bpf_design(t, 0.0, 0.06)
    f_nco = 0.1871
    pw = oracle.nco_phase_word(f_nco)
    with fir.IfFir(taps, d, 0) as f:
        f.set_nco(f_nco)
        assert f.get_backend() == fir.BACKEND_HIP_FFT
        x = torch.empty(2 * n, dtype=torch.float32, device="cuda")
        m = f.out_count(n)
        y = torch.empty(2 * m, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        f.synth_device(x.data_ptr(), 0, n, 3)

        def window_check(start, consumed, w=8192):
            lo = max(0, start - (t - 1))
            xs = x[2 * lo:2 * (start + w)].cpu().numpy()
            if consumed == 0:
                hist = np.zeros(2 * (t - 1), dtype=np.float32)
                hist[2 * (t - 1 - (start - lo)):] = xs[:2 * (start - lo)]
            else:   # the call continues a stream of identical buffers: the history is the tail of x
                assert start == 0
                hist = x[2 * (n - (t - 1)):].cpu().numpy()
            ref = oracle.fir_nco_f64(taps, xs[2 * (start - lo):], d, pw, hist=hist, consumed=consumed + start)
            first_out = (start + d - 1) // d
            got = y[2 * first_out:2 * first_out + ref.size].cpu().numpy()
            l2, mx = oracle.err_metrics(got, ref)
            assert l2 <= 1e-6 and mx <= 1e-6, (start, consumed, l2, mx)

        assert f.process_device(x.data_ptr(), y.data_ptr(), n) == m
        f.synchronize()
        for start in (0, 3840 * 5 - 64, (n // 3) & ~3, n - 8192):
            window_check(start, 0)
        f.reset()
        f.set_backend(fir.BACKEND_HIP_GENERIC)
        yg = torch.empty_like(y)
        f.process_device(x.data_ptr(), yg.data_ptr(), n)
        f.synchronize()
        scale = yg.abs().max().item()
        assert scale > 0.05 and (y - yg).abs().max().item() <= 2e-6 * scale
        del yg
        f.set_backend(fir.BACKEND_HIP_FFT)
        f.reset()
        for _ in range(17):
            f.process_device(x.data_ptr(), y.data_ptr(), n)
        f.synchronize()
        window_check(0, 16 * n)          # absolute indices 2^32 .. 2^32 + 8191


def test_beyond_32_bit_offsets(fir, oracle, gpu_ok):
    """One call of 2^31 + 12 293 samples (17 GB in, 4.3 GB out): sample indices above 2^31 and byte offsets above 2^32
    in every backend's address arithmetic.  Overlap-save against the direct form on every output, windows against the
    float64 oracle at the start, around the 2^32-byte line of the input and of the output, and at the very end."""
    import torch
    torch.cuda.set_device(0)
    t, d = 255, 4
    n = (1 << 31) + 12_293
    taps = fir.bpf_design(t)
    with fir.IfFir(taps, d, 0) as f:
        x = torch.empty(2 * n, dtype=torch.float32, device="cuda")
        m = f.out_count(n)
        y = torch.empty(2 * m, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        f.synth_device(x.data_ptr(), 0, n, 5)
        assert f.get_backend() == fir.BACKEND_HIP_FFT
        assert f.process_device(x.data_ptr(), y.data_ptr(), n) == m
        f.synchronize()
        w = 4096
        for start in (0, (1 << 29) - 2048, (1 << 31) - 2048, n - w):      # 2^29 samples = 2^32 input bytes; 2^31 samples = 2^32 output bytes
            start -= start % d
            lo = start - (t - 1) if start else 0
            xs = x[2 * lo:2 * (start + w)].cpu().numpy()
            assert np.array_equal(xs, oracle.synth_iq(start + w - lo, 5, lo))
            hist = np.zeros(2 * (t - 1), dtype=np.float32)
            hist[2 * (t - 1 - (start - lo)):] = xs[:2 * (start - lo)]
            ref = oracle.fir_f64(taps, xs[2 * (start - lo):], d, hist, start)
            got = y[2 * (start // d):2 * (start // d) + ref.size].cpu().numpy()
            l2, mx = oracle.err_metrics(got, ref)
            assert l2 <= 1e-6 and mx <= 1e-6, (start, l2, mx)
        # decimation 12 = the same tail keeping every 3rd output (round 3): the very bits of every 3rd decimate-by-4 output, with
        # block indices up to 2^31 / 3840 in its index arithmetic
        with fir.IfFir(taps, 12, 0) as f12:
            m12 = f12.out_count(n)
            y12 = torch.empty(2 * m12, dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            assert f12.process_device(x.data_ptr(), y12.data_ptr(), n) == m12
            f12.synchronize()
            yv, y12v = y.view(-1, 2), y12.view(-1, 2)
            step12 = 1 << 26
            for a in range(0, m12, step12):
                b = min(m12, a + step12)
                assert torch.equal(y12v[a:b], yv[3 * a:3 * b:3]), a
            del y12, y12v
        f.reset()
        f.set_backend(fir.BACKEND_HIP_DIRECT)
        yd = torch.empty_like(y)
        assert f.process_device(x.data_ptr(), yd.data_ptr(), n) == m
        f.synchronize()
        scale = yd.abs().max().item()
        step = 1 << 28
        worst = max((y[a:a + step] - yd[a:a + step]).abs().max().item() for a in range(0, y.numel(), step))
        assert worst <= 2e-6 * scale, worst / scale


@pytest.mark.parametrize("t,d", [(4095, 1), (4095, 4)])
def test_full_size_two_partition_filter(fir, oracle, gpu_ok, t, d):
    """3074..4096 taps (two partitions, accumulating second launch) on 2^25 samples: every output against the tap-split
    kernel (another algorithm: time-domain MACs), windows against the float64 oracle, the unit impulse returns the taps,
    and a split at a multiple of the block advance is bit-identical to the unsplit call (history = 4096 samples)."""
    import torch
    torch.cuda.set_device(0)
    n = 1 << 25
    taps = fir.bpf_design(t)
    with fir.IfFir(taps, d, 0) as f:
        assert f.get_backend() == fir.BACKEND_HIP_FFT
        x = torch.empty(2 * n, dtype=torch.float32, device="cuda")
        m = f.out_count(n)
        y = torch.empty(2 * m, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        f.synth_device(x.data_ptr(), 0, n, 3)
        assert f.process_device(x.data_ptr(), y.data_ptr(), n) == m
        f.synchronize()
        scale = float(y.abs().max().item())
        for start in [0, 2048 - 16, 4096, (n // 3) & ~3, n - 8192]:
            w = 8192
            lo = max(0, start - (t - 1))
            xs = x[2 * lo:2 * (start + w)].cpu().numpy()
            hist = np.zeros(2 * (t - 1), dtype=np.float32)
            hist[2 * (t - 1 - (start - lo)):] = xs[:2 * (start - lo)]
            ref = oracle.fir_f64(taps, xs[2 * (start - lo):], d, hist, start)
            first_out = (start + d - 1) // d
            got = y[2 * first_out:2 * first_out + ref.size].cpu().numpy()
            l2, mx = oracle.err_metrics(got, ref)
            assert l2 <= 1e-6 and mx <= 1e-6, (start, l2, mx)
        # split at 300 block advances of the 32-row kernel (2048 samples each): same blocks, same bits
        cut = 300 * 2048 * 8
        y2 = torch.empty_like(y)
        f.reset()
        m1 = f.process_device(x.data_ptr(), y2.data_ptr(), cut)
        m2 = f.process_device(x.data_ptr() + 8 * cut, y2.data_ptr() + 8 * m1, n - cut)
        f.synchronize()
        assert m1 + m2 == m and torch.equal(y, y2)
        # another algorithm on the whole array
        yt = torch.empty_like(y)
        f.set_backend(fir.BACKEND_HIP_TAPSPLIT)
        f.reset()
        assert f.process_device(x.data_ptr(), yt.data_ptr(), n) == m
        f.synchronize()
        assert float((y - yt).abs().max().item()) <= 2e-6 * scale
        # impulse response
        f.set_backend(fir.BACKEND_HIP_FFT)
        f.reset()
        x[:2 * 16384].zero_()
        x[2 * 5] = 1.0
        f.process_device(x.data_ptr(), y.data_ptr(), 16384)
        f.synchronize()
        got = y[:2 * (16384 // d)].cpu().numpy()
        full = np.zeros(16384, dtype=np.float64)
        full[5:5 + t] = taps
        want = full[::d][:got.size // 2]
        assert np.max(np.abs(got[0::2] - want)) <= 1e-6 * np.max(np.abs(taps)) and np.max(np.abs(got[1::2])) <= 1e-6 * np.max(np.abs(taps))


@pytest.mark.parametrize("n", [(1 << 23) + 777, (1 << 24) + 12_345, (1 << 25) + 1, 16_773_120])
def test_mid_size_launches_with_the_tail_phase(fir, oracle, gpu_ok, n):
    """Launches of 1 to 6 two-wave rounds hand the remainder out one block per SIMD (the block queue's tail phase, round 3;
    16 773 120 samples = the multi-channel front's chunk): EVERY output against the direct-form kernel on the same input,
    a window at the very end (the tail blocks) against the float64 oracle, and the launch without the tail phase
    (development variant) bit for bit."""
    import torch
    torch.cuda.set_device(0)
    t, d = 255, 4
    taps = fir.bpf_design(t)
    old = os.environ.get("IF_FIR_DEBUG")
    os.environ["IF_FIR_DEBUG"] = "1"
    try:
        with fir.IfFir(taps, d, 0, dev=True) as f:
            x = torch.empty(2 * n, dtype=torch.float32, device="cuda")
            m = f.out_count(n)
            y = torch.empty(2 * m, dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            f.synth_device(x.data_ptr(), 0, n, 3)
            assert f.get_backend() == fir.BACKEND_HIP_FFT
            assert f.process_device(x.data_ptr(), y.data_ptr(), n) == m
            f.synchronize()
            assert f.debug_queue_faults() == 0
            w = 8192
            start = (n - w) & ~3
            xs = x[2 * (start - (t - 1)):].cpu().numpy()
            hist = xs[:2 * (t - 1)].copy()
            ref = oracle.fir_f64(taps, xs[2 * (t - 1):], d, hist, start)
            got = y[2 * (start // d):].cpu().numpy()
            l2, mx = oracle.err_metrics(got, ref)
            assert l2 <= 1e-6 and mx <= 1e-6, (l2, mx)
            f.reset()
            f.set_tuning(1000000 + 256)          # the same launch without the tail phase: the same bits
            y2 = torch.empty_like(y)
            assert f.process_device(x.data_ptr(), y2.data_ptr(), n) == m
            f.synchronize()
            assert torch.equal(y, y2)
            f.set_tuning(0)
            f.reset()
            f.set_backend(fir.BACKEND_HIP_DIRECT)
            assert f.process_device(x.data_ptr(), y2.data_ptr(), n) == m
            f.synchronize()
            scale = y2.abs().max().item()
            assert scale > 0.1 and (y - y2).abs().max().item() <= 2e-6 * scale
    finally:
        if old is None:
            os.environ.pop("IF_FIR_DEBUG", None)
        else:
            os.environ["IF_FIR_DEBUG"] = old


@pytest.mark.parametrize("d,nch", [(8, 16), (8, 6), (16, 16)])
def test_full_size_filter_bank(fir, oracle, gpu_ok, monkeypatch, d, nch):
    """The filter bank at the headline size (2^28 samples of one wideband stream): EVERY output of every channel against (a) the
    other form of the same bank -- decimation 8: the all-slots launches (round 4) against the per-channel form (development launch
    4096) -- and (b), for two channels, a context that mixes, filters and decimates that one channel (if_fir_set_nco); windows of one
    channel against the float64 NCO oracle; one call = two calls at an odd cut."""
    import torch
    torch.cuda.set_device(0)
    monkeypatch.setenv("IF_FIR_DEBUG", "1")
    n, t = 1 << 28, 255
    taps = fir.bpf_design(t, 0.0, 0.02)
    slots = list(range(16)) if nch == 16 else [1, 3, 5, 7, 9, 2]   # (6: five odd slots through the all-slots launch + an even one per channel)
    with fir.IfFir(taps, d, 0, dev=True) as f:
        x = torch.empty(2 * n, dtype=torch.float32, device="cuda")
        m = f.out_count(n)
        outs = [torch.empty(2 * m, dtype=torch.float32, device="cuda") for _ in slots]
        torch.cuda.synchronize()
        f.synth_device(x.data_ptr(), 0, n, 5)
        assert f.get_backend() == fir.BACKEND_HIP_FFT
        assert f.channelizer_process_device(slots, x.data_ptr(), [o.data_ptr() for o in outs], n) == m
        f.synchronize()
        assert f.debug_queue_faults() == 0
        scale = max(o.abs().max().item() for o in outs)
        assert scale > 0.05
        if d == 8:
            # (a) the per-channel form, every output of every channel
            f.set_tuning(1000000 + 4096)
            f.reset()
            other = torch.empty(2 * m, dtype=torch.float32, device="cuda")
            for c, s in enumerate(slots):
                assert f.channelizer_process_device([s], x.data_ptr(), [other.data_ptr()], n) == m
                f.synchronize()
                f.reset()
                assert (outs[c] - other).abs().max().item() <= 2e-6 * scale, (d, s)
            del other
            f.set_tuning(0)
        # split invariance: two calls at an odd cut (the all-slots launches carry the history and the mix-down phase like any call)
        f.reset()
        cut = (n // 2) + 12345
        part = [torch.empty(2 * m, dtype=torch.float32, device="cuda") for _ in slots]
        m1 = f.channelizer_process_device(slots, x.data_ptr(), [p.data_ptr() for p in part], cut)
        tail = x[2 * cut:].clone()
        torch.cuda.synchronize()
        m2 = f.channelizer_process_device(slots, tail.data_ptr(), [p.data_ptr() + 8 * m1 for p in part], n - cut)
        f.synchronize()
        assert m1 + m2 == m
        for c in range(len(slots)):
            assert (outs[c] - part[c]).abs().max().item() <= 1e-6 * scale, (d, slots[c])
        del part, tail
    # (b) one context per channel, every output
    ref = torch.empty(2 * m, dtype=torch.float32, device="cuda")
    for c in (1, len(slots) - 1):
        s = slots[c]
        with fir.IfFir(taps, d, 0) as f1:
            f1.set_nco(s / 16.0 if s <= 8 else s / 16.0 - 1.0)
            assert f1.process_device(x.data_ptr(), ref.data_ptr(), n) == m
            f1.synchronize()
        assert (outs[c] - ref).abs().max().item() <= 2e-6 * scale, (d, s)
    # windows of one channel against the float64 NCO oracle
    c = 2
    s = slots[c]
    w = 8192
    for start in [0, (n // 3) & ~15, n - w]:
        lo = max(0, start - (t - 1))
        xs = x[2 * lo:2 * (start + w)].cpu().numpy()
        hist = np.zeros(2 * (t - 1), dtype=np.float32)
        hist[2 * (t - 1 - (start - lo)):] = xs[:2 * (start - lo)]
        refw = oracle.fir_nco_f64(taps, xs[2 * (start - lo):], d, (s << 28) & 0xFFFFFFFF, hist, start)
        first_out = (start + d - 1) // d
        got = outs[c][2 * first_out:2 * first_out + refw.size].cpu().numpy()
        l2, mx = oracle.err_metrics(got, refw)
        assert l2 <= 1e-6 and mx <= 1e-6, (d, s, start, l2, mx)


# ---- the filter bank with every channel at its own centre (if_fir_channelizer_process_device_freq, SPEC §3.3) at size --------------
TOL = 1e-6           # SPEC §3
MARGIN = 4096        # canary floats on either side of a channel's outputs
# six centres on the 1/4096 grid, two off it (819/4096 and 0.2 sit on the generator's 0.2 tone, the others see its noise floor)
BANK_CENTRES = [300 / 4096.0, 819 / 4096.0, -333 / 4096.0, 2047 / 4096.0, -2048 / 4096.0, 1 / 4096.0, 0.2, -0.123456789]
BANK_MORE = [0.0, 255 / 4096.0, 256 / 4096.0, 257 / 4096.0, 1638 / 4096.0]     # (13 channels: the partial group of four of tail 17)


def _on_grid(fc):
    return fc * 4096.0 == np.round(fc * 4096.0)


def _bank_input(torch, f, n, i16):
    """2^28-class input on the device: the synthetic stream (channel 5); int16: scaled by 12000, rounded and clipped in chunks."""
    x = torch.empty(2 * n, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    f.synth_device(x.data_ptr(), 0, n, 5)
    f.synchronize()
    if not i16:
        return x
    xi = torch.empty(2 * n, dtype=torch.int16, device="cuda")
    step = 1 << 26
    for a in range(0, 2 * n, step):
        xi[a:a + step] = torch.clamp(torch.round(x[a:a + step] * 12000.0), -32768, 32767).to(torch.int16)
    torch.cuda.synchronize()
    return xi


def _samples(xd, i16, lo, hi):
    """Samples [lo, hi) of the device buffer as the interleaved float32 values the filter sees."""
    xs = xd[2 * lo:2 * hi].cpu().numpy()
    return xs.astype(np.float32) * np.float32(2.0 ** -15) if i16 else xs


def _window_input(xd, i16, n, t, start, w, continued):
    """The t - 1 samples before sample `start` of this call and the window's w samples; in front of the call's first sample: zeros, or
    the end of the same buffer when the call continues a stream of identical buffers."""
    lo = max(0, start - (t - 1))
    xs = _samples(xd, i16, lo, start + w)
    missing = t - 1 - (start - lo)
    if missing:
        head = _samples(xd, i16, n - missing, n) if continued else np.zeros(2 * missing, dtype=np.float32)
        xs = np.concatenate([head, xs])
    return xs


def _bank_outputs(torch, nch, m):
    """One buffer per channel, MARGIN canary floats on either side of its m outputs."""
    bufs = [torch.full((2 * m + 2 * MARGIN,), 3.0, dtype=torch.float32, device="cuda") for _ in range(nch)]
    return bufs, [b[MARGIN:MARGIN + 2 * m] for b in bufs]


def _canaries_intact(torch, bufs, m):
    return all(bool(torch.all(b[:MARGIN] == 3.0)) and bool(torch.all(b[MARGIN + 2 * m:] == 3.0)) for b in bufs)


def _max_abs_diff(a, b, step=1 << 27):
    """(max |a - b|, max |b|) over two device arrays, in slices (no full-size temporaries)."""
    worst = scale = 0.0
    for i in range(0, a.numel(), step):
        worst = max(worst, (a[i:i + step] - b[i:i + step]).abs().max().item())
        scale = max(scale, b[i:i + step].abs().max().item())
    return worst, scale


def _check_bank_windows(oracle, taps, d, centres, outs, xd, i16, n, consumed, starts, what):
    """Windows of every channel against tests/bank_ref.py.  starts: (first sample of the window within this call, samples)."""
    import bank_ref
    t = len(taps)
    for start, w in starts:
        xs = _window_input(xd, i16, n, t, start, w, consumed > 0)
        first_out = oracle.out_count(consumed, start, d)
        for c, fc in enumerate(centres):
            ref = bank_ref.bank_window_ref(oracle, taps, xs, t, d, fc, consumed + start)
            assert ref.size == 2 * 2048 and np.max(np.abs(ref)) > 0.01
            got = outs[c][2 * first_out:2 * first_out + ref.size].cpu().numpy()
            l2, mx = oracle.err_metrics(got, ref)
            print("%s window d=%d start=%d centre=%.9f: l2=%.3g max=%.3g (largest output %.3g)"
                  % (what, d, consumed + start, fc, l2, mx, np.max(np.abs(ref))))
            assert l2 <= TOL and mx <= TOL, (what, d, fc, consumed + start, l2, mx)


@pytest.mark.parametrize("d,i16,nch", [(4, False, 8), (4, True, 8), (8, False, 8), (16, False, 8), (16, True, 8), (64, False, 8),
                                       (12, False, 8), (24, True, 8), (48, False, 8), (16, False, 13), (8, False, 5)])
def test_full_size_filter_bank_own_centres(fir, oracle, gpu_ok, monkeypatch, d, i16, nch):
    """The filter bank with every channel at its own centre (if_fir_channelizer_process_device_freq) at the headline size, 2^28 samples
    = 70 000 blocks through the two-level block queue: each per-channel tail once plain (decimation 4, 8, 16) and once keeping every
    sub-th output (12; 24; 64 = power of two and 48 = general divisor inside the four-channels-per-inverse tail), float32 and int16,
    and channel counts that leave a partial group (13 of four, 5 of two).  Per case: the return value, no expired queue wait, canaries on both
    sides of every channel's buffer; EVERY output of every channel on the 1/4096 grid against a one-channel context with
    if_fir_set_nco(centre) (both within TOL of the float64 result: 2 TOL of that channel's largest output); windows of 2048 outputs
    of EVERY channel (first block, first block seam, interior, the last outputs) against the float64 definition (tests/bank_ref.py); one
    call = two calls at an odd cut, to TOL of the channel's largest output (measured on the MI355X: not bit-identical -- the second call's
    block grid starts at the cut -- so no equality is asserted).  Measured there over these tests' 448 windows: l2 <= 5.6e-7, max <= 7.0e-7;
    every output against the one-channel context <= 5.7e-7 of the channel's largest output."""
    import torch
    torch.cuda.set_device(0)
    monkeypatch.setenv("IF_FIR_DEBUG", "1")
    n, t = 1 << 28, 255
    taps = fir.bpf_design(t, 0.0, 0.02)
    centres = {8: BANK_CENTRES, 13: BANK_CENTRES + BANK_MORE, 5: [BANK_CENTRES[i] for i in (0, 1, 4, 6, 7)]}[nch]
    what = "own_centres[%d-%s-%d]" % (d, "i16" if i16 else "f32", nch)
    with fir.IfFir(taps, d, 0, dev=True) as f:
        if i16:
            f.set_input_format(fir.INPUT_I16)
        xd = _bank_input(torch, f, n, i16)
        m = f.out_count(n)
        assert m == oracle.out_count(0, n, d)
        bufs, outs = _bank_outputs(torch, nch, m)
        torch.cuda.synchronize()
        assert f.get_backend() == fir.BACKEND_HIP_FFT
        assert f.channelizer_process_device_freq(centres, xd.data_ptr(), [o.data_ptr() for o in outs], n) == m
        f.synchronize()
        assert f.debug_queue_faults() == 0
        assert _canaries_intact(torch, bufs, m)
        # every output of the channels on the grid: one context that mixes, filters and decimates that channel alone
        ref = torch.empty(2 * m, dtype=torch.float32, device="cuda")
        with fir.IfFir(taps, d, 0) as f1:
            if i16:
                f1.set_input_format(fir.INPUT_I16)
            for c, fc in enumerate(centres):
                if not _on_grid(fc):
                    continue
                f1.reset()
                f1.set_nco(fc)
                assert f1.process_device(xd.data_ptr(), ref.data_ptr(), n) == m
                f1.synchronize()
                worst, scale = _max_abs_diff(outs[c], ref)
                print("%s every output, centre %.9f: max diff %.3g of largest output %.3g" % (what, fc, worst / scale, scale))
                assert scale > 0.01 and worst <= 2 * TOL * scale, (what, fc, worst / scale)
        del ref
        # windows of every channel against the float64 definition
        w = 2048 * d
        seam = 3840 * 5 - 64
        _check_bank_windows(oracle, taps, d, centres, outs, xd, i16, n, 0,
                            [(0, w), (seam - seam % d, w), ((n // 3) - (n // 3) % (4 * d), w), ((m - 2048) * d, n - (m - 2048) * d)], what)
        # one call = two calls at an odd cut (the second call's input in a buffer of its own: aligned, and the cut stays odd for int16)
        f.reset()
        cut = (n // 2) + 12345
        bufs2, part = _bank_outputs(torch, nch, m)
        torch.cuda.synchronize()
        m1 = f.channelizer_process_device_freq(centres, xd.data_ptr(), [p.data_ptr() for p in part], cut)
        tail = xd[2 * cut:].clone()
        ptail = [torch.empty(2 * (m - m1), dtype=torch.float32, device="cuda") for _ in range(nch)]
        torch.cuda.synchronize()
        m2 = f.channelizer_process_device_freq(centres, tail.data_ptr(), [p.data_ptr() for p in ptail], n - cut)
        f.synchronize()
        assert m1 == oracle.out_count(0, cut, d) and m1 + m2 == m
        assert f.debug_queue_faults() == 0
        same = True
        for c in range(nch):
            part[c][2 * m1:] = ptail[c]
            worst, scale = _max_abs_diff(part[c], outs[c])
            same = same and torch.equal(part[c], outs[c])
            assert worst <= TOL * scale, (what, centres[c], worst / scale)
        print("%s one call vs two calls: bit-identical = %s" % (what, same))
        assert _canaries_intact(torch, bufs2, m)


@pytest.mark.parametrize("d", [4, 8, 16, 48])
def test_filter_bank_own_centres_past_2_32_samples(fir, oracle, gpu_ok, monkeypatch, d):
    """A stream continued past 2^32 samples (17 calls of 2^28 samples of one buffer on one context): the only place where the absolute
    sample index of a bank call no longer fits 32 bits.  The mix-down phase is P a mod 2^32; the centres off the grid have odd P, for
    which every bit of a below 2^32 counts and a truncated or sign-extended index shows.  (Decimation 48: 2^28 is no multiple of it, so
    every call also starts at another decimation phase.)  The 17th call's first 2048 outputs of every channel (history = the end of the
    buffer) and 2048 in its middle against the float64 definition."""
    import torch
    torch.cuda.set_device(0)
    monkeypatch.setenv("IF_FIR_DEBUG", "1")
    n, t = 1 << 28, 255
    taps = fir.bpf_design(t, 0.0, 0.02)
    centres = BANK_CENTRES
    with fir.IfFir(taps, d, 0, dev=True) as f:
        xd = _bank_input(torch, f, n, False)
        mmax = n // d + 1
        bufs, outs = _bank_outputs(torch, len(centres), mmax)
        torch.cuda.synchronize()
        for call in range(17):
            m = f.channelizer_process_device_freq(centres, xd.data_ptr(), [o.data_ptr() for o in outs], n)
            assert m == oracle.out_count(call * n, n, d)
        f.synchronize()
        assert f.debug_queue_faults() == 0
        assert _canaries_intact(torch, bufs, mmax)
        w = 2048 * d
        _check_bank_windows(oracle, taps, d, centres, outs, xd, False, n, 16 * n, [(0, w), ((n // 2) - (n // 2) % (4 * d) + 4 * d, w)],
                            "past_2_32[%d]" % d)


def test_filter_bank_own_centres_beyond_32_bit_offsets(fir, oracle, gpu_ok, monkeypatch):
    """One call of 2^31 + 12 293 samples (17 GB of float32 in), three channels at their own centres.  Decimation 4: 4.3 GB per channel,
    so the per-lane 32-bit store offsets sit on a 64-bit base that passes 2^32 bytes -- windows against the float64 definition at the
    start, around the 2^32-byte line of the input (sample 2^29) and of the OUTPUT (sample 2^31) and the last 2048 outputs; the channels
    on the grid whole against a context with if_fir_set_nco; canaries.  Decimation 12 (every 3rd output of the same tail, block indices up to
    2^31 / 3840 through KeepEvery): the same windows, and every output against every third output of the decimate-by-4 run: the same bits
    (measured on the MI355X before it was asserted; the single-channel tail has the same property in test_beyond_32_bit_offsets).
    Peak device memory about 39 GB: 17 in, 3 x 4.3 out, 4.3 for the one-channel reference or 3 x 1.4 for decimation 12."""
    import torch
    torch.cuda.set_device(0)
    monkeypatch.setenv("IF_FIR_DEBUG", "1")
    t = 255
    n = (1 << 31) + 12_293
    taps = fir.bpf_design(t, 0.0, 0.02)
    centres = [300 / 4096.0, 0.2, -2048 / 4096.0]

    def windows(d, m):
        w = 2048 * d
        mids = [(1 << 29) - w // 2, (1 << 31) - w // 2]
        return [(0, w)] + [(s - s % d, w) for s in mids] + [((m - 2048) * d, n - (m - 2048) * d)]

    with fir.IfFir(taps, 4, 0, dev=True) as f:
        xd = _bank_input(torch, f, n, False)
        m = f.out_count(n)
        assert m == oracle.out_count(0, n, 4) and 8 * m > 1 << 32
        bufs, outs = _bank_outputs(torch, 3, m)
        torch.cuda.synchronize()
        assert f.channelizer_process_device_freq(centres, xd.data_ptr(), [o.data_ptr() for o in outs], n) == m
        f.synchronize()
        assert f.debug_queue_faults() == 0
        assert _canaries_intact(torch, bufs, m)
        _check_bank_windows(oracle, taps, 4, centres, outs, xd, False, n, 0, windows(4, m), "beyond_32_bit[4]")
        ref = torch.empty(2 * m, dtype=torch.float32, device="cuda")
        with fir.IfFir(taps, 4, 0) as f1:
            for c in (0, 2):
                f1.reset()
                f1.set_nco(centres[c])
                assert f1.process_device(xd.data_ptr(), ref.data_ptr(), n) == m
                f1.synchronize()
                worst, scale = _max_abs_diff(outs[c], ref)       # (slices of 2^26 outputs)
                print("beyond_32_bit[4] every output, centre %.9f: max diff %.3g of largest output %.3g" % (centres[c], worst / scale, scale))
                assert scale > 0.01 and worst <= 2 * TOL * scale, (centres[c], worst / scale)
        del ref
        with fir.IfFir(taps, 12, 0, dev=True) as f12:
            m12 = f12.out_count(n)
            assert m12 == oracle.out_count(0, n, 12)
            bufs12, outs12 = _bank_outputs(torch, 3, m12)
            torch.cuda.synchronize()
            assert f12.channelizer_process_device_freq(centres, xd.data_ptr(), [o.data_ptr() for o in outs12], n) == m12
            f12.synchronize()
            assert f12.debug_queue_faults() == 0
            assert _canaries_intact(torch, bufs12, m12)
            _check_bank_windows(oracle, taps, 12, centres, outs12, xd, False, n, 0, windows(12, m12), "beyond_32_bit[12]")
            same = True
            step = 1 << 26
            for c in range(3):
                y4, y12 = outs[c].view(-1, 2), outs12[c].view(-1, 2)
                worst = scale = 0.0
                for a in range(0, m12, step):
                    b = min(m12, a + step)
                    third = y4[3 * a:3 * b:3]
                    worst = max(worst, (y12[a:b] - third).abs().max().item())
                    scale = max(scale, third.abs().max().item())
                    same = same and torch.equal(y12[a:b], third)
                assert scale > 0.01 and worst <= 2 * TOL * scale, (centres[c], worst / scale)
            print("beyond_32_bit[12] vs every third decimate-by-4 output: bit-identical = %s" % same)
            assert same     # (measured on the MI355X: the same tail with two of three stores left out, the same bits)
