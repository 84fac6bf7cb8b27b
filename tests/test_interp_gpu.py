"""The interpolator (if_fir_interp_t, docs/SPEC.md §6) on the GPU against a float64 reference: oracle.fir_f64 of the
zero-stuffed input (numpy for the complex-tap and NCO parts), SPEC §3 tolerance."""
import functools
import os
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-6
TAPS = (31, 255, 1023, 3073)


@pytest.fixture(scope="module")
def torch_cuda(gpu_ok):
    import torch
    torch.cuda.set_device(0)
    return torch


def zero_stuffed(x, L):
    """interleaved float32 x (n samples) -> interleaved float32 u (n L samples), u[n L] = x[n]"""
    x = np.asarray(x, dtype=np.float32).reshape(-1, 2)
    u = np.zeros((x.shape[0] * L, 2), dtype=np.float32)
    u[::L] = x
    return u.reshape(-1)


def as_c(y):
    y = np.asarray(y, dtype=np.float64).reshape(-1, 2)
    return y[:, 0] + 1j * y[:, 1]


def as_iq(c):
    return np.stack([c.real, c.imag], axis=1).reshape(-1)


def reference(oracle, taps, x, L, complex_taps=False, word=0, first_out=0):
    """float64: y'[n] = exp(+j 2 pi P n / 2^32) sum_k h[k] u[n-k], n = first_out + output index"""
    u = zero_stuffed(x, L)
    if complex_taps:
        t = np.asarray(taps, dtype=np.float32).reshape(-1, 2)
        y = as_c(oracle.fir_f64(np.ascontiguousarray(t[:, 0]), u, 1)) + 1j * as_c(oracle.fir_f64(np.ascontiguousarray(t[:, 1]), u, 1))
    else:
        y = as_c(oracle.fir_f64(taps, u, 1))
    if word:
        n = (np.arange(y.size, dtype=np.uint64) + np.uint64(first_out)) % np.uint64(1 << 32)
        ph = (n * np.uint64(word)) % np.uint64(1 << 32)
        y = y * np.exp(2j * np.pi * ph.astype(np.float64) / 4294967296.0)
    return as_iq(y)


def taps_for(fir, T, L, complex_taps):
    """image-rejection low-pass of gain L (complex: shifted off centre)"""
    if complex_taps:
        return (fir.bpf_design_complex(T, 0.1 / L, 0.8 / L) * np.float32(L)).astype(np.float32)
    return (fir.bpf_design(T, 0.0, 0.45 / L) * np.float32(L)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def signal(n, i16):
    import __graft_entry__ as g
    x = g.load_oracle().synth_iq(n, channel=3)
    if i16:
        xi = np.clip(np.round(x * 14000.0), -32768, 32767).astype(np.int16)
        return xi, xi.astype(np.float32) * np.float32(2.0 ** -15)
    return x, x


FORMS = ("small", "full", "generic")


def cases():
    out = []
    for L in (1, 2, 3, 4, 5, 8, 16, 64):
        for form in FORMS:
            if form == "small" and (L < 4 or 64 % L):
                continue
            if form == "full" and 64 % L:
                continue
            for ct in (False, True):
                for i16 in (False, True):
                    T = TAPS[(L + 2 * ct + i16 + FORMS.index(form)) % 4]
                    out.append((L, form, ct, i16, T))
    return out


def make(fir, taps, L, form, ct, n, dev=True):
    f = fir.IfFirInterp(taps, L, max_samples=n, complex_taps=ct, dev=dev)
    if form == "generic":
        f.set_backend(fir.BACKEND_HIP_GENERIC)
    else:
        assert f.get_backend() == fir.BACKEND_HIP_FFT
        f.debug_config(force_full=(form == "full"))
    return f


@pytest.mark.gpu
@pytest.mark.parametrize("L,form,ct,i16,T", cases())
def test_interp_matches_float64_reference(gpu_ok, fir, oracle, L, form, ct, i16, T):
    n = max(4000, 400_000 // L)
    raw, x = signal(n, i16)
    taps = taps_for(fir, T, L, ct)
    with make(fir, taps, L, form, ct, n) as f:
        if i16:
            f.set_input_format(fir.INPUT_I16)
        cut = n // 3
        y = np.concatenate([f.process(raw[:2 * cut]), f.process(raw[2 * cut:])])
    ref = reference(oracle, taps, x, L, ct)
    assert y.size == 2 * n * L
    l2, mx = oracle.err_metrics(y, ref)
    assert l2 <= TOL and mx <= TOL, (l2, mx)


@pytest.mark.gpu
def test_auto_backend_choice(gpu_ok, fir):
    h = fir.bpf_design(255)
    for L, T, want in ((4, 255, fir.BACKEND_HIP_FFT), (64, 3073, fir.BACKEND_HIP_FFT), (3, 255, fir.BACKEND_HIP_GENERIC),
                       (4, 3075, fir.BACKEND_HIP_GENERIC), (1, 31, fir.BACKEND_HIP_FFT)):
        with fir.IfFirInterp(fir.bpf_design(T) if T != 255 else h, L, max_samples=1000) as f:
            assert f.get_backend() == want, (L, T)
            assert f.out_count(1000) == 1000 * L


@pytest.mark.gpu
@pytest.mark.parametrize("L,form", [(4, "small"), (16, "small"), (2, "full"), (8, "full"), (3, "generic"), (8, "generic")])
def test_pieces(gpu_ok, fir, oracle, L, form):
    """ragged pieces match one call within tolerance; pieces cut at multiples of A/L inputs match it bit for bit (overlap-save);
    the generic kernel is bit-exact for any cut"""
    T = 255
    n = 60_000
    x, _ = signal(n, False)
    taps = taps_for(fir, T, L, False)
    with make(fir, taps, L, form, False, n) as f:
        one = f.process(x)
        a_in = (4096 - 256) // L if 64 % L == 0 else 1000
        for sizes, exact in (([1, 7, a_in - 1, a_in + 1, 2, 3 * a_in + 5, 1000], form == "generic"),
                             ([a_in, 3 * a_in, 2 * a_in, a_in], True)):
            f.reset()
            parts, pos = [], 0
            for s in sizes:
                parts.append(f.process(x[2 * pos:2 * (pos + s)]))
                pos += s
            parts.append(f.process(x[2 * pos:]))
            y = np.concatenate(parts)
            assert y.size == one.size
            if exact:
                assert np.array_equal(y, one), np.max(np.abs(y - one))
            else:
                l2, mx = oracle.err_metrics(y, one.astype(np.float64))
                assert l2 <= TOL and mx <= TOL, (sizes, l2, mx)


@pytest.mark.gpu
def test_reset_and_bad_arguments(gpu_ok, fir, oracle, torch_cuda):
    torch = torch_cuda
    n = 20_000
    x, _ = signal(n, False)
    taps = taps_for(fir, 255, 4, False)
    with fir.IfFirInterp(taps, 4, max_samples=n) as f:
        y0 = f.process(x)
        f.process(x[:2000])
        f.reset()
        assert np.array_equal(f.process(x), y0)
        for bad in (lambda: f.set_backend(fir.BACKEND_HIP_DIRECT), lambda: f.set_backend(fir.BACKEND_HIP_TAPSPLIT),
                    lambda: f.set_backend(9), lambda: f.set_nco(0.7), lambda: f.set_input_format(5),
                    lambda: f.process(np.zeros(2 * (n + 1), dtype=np.float32))):
            with pytest.raises(fir.IfFirError) as e:
                bad()
            assert str(e.value)
        buf = torch.zeros(2 * 1000 * 4 + 8, dtype=torch.float32, device="cuda")
        with pytest.raises(fir.IfFirError, match="aligned"):
            f.process_device(buf.data_ptr() + 4, buf.data_ptr(), 100)      # input off by half a sample
        with pytest.raises(fir.IfFirError, match="aligned"):
            f.process_device(buf.data_ptr(), buf.data_ptr() + 4, 100)
        f.set_backend(fir.BACKEND_HIP_GENERIC)
        with pytest.raises(fir.IfFirError, match="16-byte"):
            f.process_device(buf.data_ptr() + 8, buf.data_ptr(), 100)       # the generic kernel: 16-byte rule
        f.set_backend(fir.BACKEND_AUTO)
        f.reset()
        assert np.array_equal(f.process(x), y0)  # still usable
    with fir.IfFirInterp(fir.bpf_design(31), 3, max_samples=10) as f:
        with pytest.raises(fir.IfFirError, match="overlap-save"):
            f.set_backend(fir.BACKEND_HIP_FFT)
        assert f.get_backend() == fir.BACKEND_HIP_GENERIC
    for T, L in ((0, 4), (4097, 4), (31, 0), (31, 65)):
        with pytest.raises(fir.IfFirError):
            fir.IfFirInterp(np.ones(max(T, 1), dtype=np.float32)[:T] if T else np.zeros(0, dtype=np.float32), L)


@pytest.mark.gpu
@pytest.mark.parametrize("freq,form", [(0.37, "small"), (-0.37, "full"), (1 / 4096, "small"), (0.37, "generic"), (-0.21, "small")])
def test_nco_up_mix(gpu_ok, fir, oracle, freq, form):
    L, T, n = 8, 255, 30_000
    x, _ = signal(n, False)
    ct = freq == -0.21
    taps = taps_for(fir, T, L, ct)
    with make(fir, taps, L, form, ct, n) as f:
        f.set_nco(freq)
        word = oracle.nco_phase_word(freq)
        assert f.get_nco() == pytest.approx(((word + (1 << 31)) % (1 << 32) - (1 << 31)) / 2.0 ** 32, abs=0)
        y = np.concatenate([f.process(x[:2 * 777]), f.process(x[2 * 777:])])
    l2, mx = oracle.err_metrics(y, reference(oracle, taps, x, L, ct, word))
    assert l2 <= TOL and mx <= TOL, (l2, mx)


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["small", "generic"])
def test_nco_past_output_index_2_32(gpu_ok, fir, oracle, form):
    """the up-mix is indexed by the absolute output index mod 2^32: a window just across 2^32 (development seek hook)"""
    L, T, n = 16, 255, 20_000
    x, _ = signal(n, False)
    taps = taps_for(fir, T, L, False)
    first_in = (1 << 32) // L - 5000
    with make(fir, taps, L, form, False, n) as f:
        f.set_nco(0.37)
        f.debug_seek(first_in)
        y = f.process(x)
    ref = reference(oracle, taps, x, L, False, oracle.nco_phase_word(0.37), first_out=first_in * L)
    l2, mx = oracle.err_metrics(y, ref)
    assert l2 <= TOL and mx <= TOL, (l2, mx)


@pytest.mark.gpu
def test_small_grid_multi_round(gpu_ok, fir):
    """a few persistent workgroups take many blocks each: same results bit for bit"""
    n = 50_000
    x, _ = signal(n, False)
    for L, form in ((4, "small"), (2, "full"), (5, "generic")):
        taps = taps_for(fir, 255, L, False)
        with make(fir, taps, L, form, False, n) as f:
            y = f.process(x)
            for k in (1, 3, 7):
                f.reset()
                f.debug_config(force_full=(form == "full"), grid_limit=k)
                assert np.array_equal(f.process(x), y), (L, form, k)


@pytest.mark.gpu
def test_canaries_and_device_path(gpu_ok, fir, torch_cuda):
    torch = torch_cuda
    n, L, pad = 9_999, 8, 4096
    x, _ = signal(n, False)
    taps = taps_for(fir, 1023, L, False)
    with fir.IfFirInterp(taps, L, max_samples=n, dev=True) as f:
        y = f.process(x)
        for form in ("small", "full", "generic"):
            f.reset()
            if form == "generic":
                f.set_backend(fir.BACKEND_HIP_GENERIC)
            else:
                f.debug_config(force_full=(form == "full"))
            din = torch.from_numpy(x).cuda()
            buf = torch.full((2 * (n * L + 2 * pad),), 12345.0, dtype=torch.float32, device="cuda")
            m = f.process_device(din.data_ptr(), buf.data_ptr() + 8 * pad, n)
            f.synchronize()
            assert m == n * L
            h = buf.cpu().numpy()
            assert np.all(h[:2 * pad] == 12345.0) and np.all(h[-2 * pad:] == 12345.0), form
            got = h[2 * pad:-2 * pad]
            if form == "small":
                assert np.array_equal(got, y)
            else:
                assert np.max(np.abs(got - y)) <= 1e-5 * np.max(np.abs(y)), form


@pytest.mark.gpu
@pytest.mark.parametrize("L", [4, 16])
def test_full_size_small_against_full(gpu_ok, fir, oracle, torch_cuda, L):
    """2^28 outputs: the whole output of the small form against the full form, and windows against float64"""
    torch = torch_cuda
    T = 255
    M = 1 << 28
    n = M // L
    x = oracle.synth_iq(n, channel=5)
    taps = taps_for(fir, T, L, False)
    din = torch.from_numpy(x).cuda()
    with fir.IfFirInterp(taps, L, max_samples=1 << 10, dev=True) as f:
        ys = torch.empty(2 * M, dtype=torch.float32, device="cuda")
        assert f.process_device(din.data_ptr(), ys.data_ptr(), n) == M
        f.synchronize()
        f.reset()
        f.debug_config(force_full=True)
        yf = torch.empty(2 * M, dtype=torch.float32, device="cuda")
        f.process_device(din.data_ptr(), yf.data_ptr(), n)
        f.synchronize()
    diff = (ys.double() - yf.double()).norm().item() / yf.double().norm().item()
    mxd = (ys - yf).abs().max().item() / yf.abs().max().item()
    assert diff <= TOL and mxd <= TOL, (diff, mxd)
    del yf
    for o in (0, (M // 3) // L * L, M - 8192):
        j_lo = max(0, (o - (T - 1)) // L)
        j_hi = min(n, (o + 8192) // L + 1)
        ref = reference(oracle, taps, x[2 * j_lo:2 * j_hi], L)
        ref = ref[2 * (o - j_lo * L):2 * (o - j_lo * L + 8192)]
        got = ys[2 * o:2 * (o + 8192)].cpu().numpy()
        l2, mx = oracle.err_metrics(got, ref)
        assert l2 <= TOL and mx <= TOL, (o, l2, mx)


@pytest.mark.gpu
def test_c_program_on_the_interp_abi(gpu_ok):
    libdir = os.path.join(ROOT, "qo-100-tools_amd")
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "if_fir_interp_selftest")
        subprocess.check_call(["gcc", "-std=c99", "-O1", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"),
                               os.path.join(ROOT, "tests", "c", "if_fir_interp_selftest.c"), "-L" + libdir, "-lif_fir", "-lm",
                               "-Wl,-rpath," + libdir, "-o", exe])
        run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
        assert run.returncode == 0, run.stdout + run.stderr
        assert "all checks passed" in run.stdout
