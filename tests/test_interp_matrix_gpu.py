"""The interpolator (if_fir_interp_t, docs/SPEC.md §6) unit by unit: every compiled instantiation of the overlap-save and the
generic kernel, every tap count either side of an overlap class, every L | 64, call sizes round a block, pieces shorter than
the history, outputs beyond 2^32 bytes.  Reference as in tests/test_interp_gpu.py: oracle.fir_f64 of the zero-stuffed input
(complex taps as two real passes), the up-mix in float64 with the integer phase (P n) mod 2^32; SPEC §3 tolerance.

The taps here (tests/matrix_util.py) are not a windowed design (whose end taps are zero, and the next ones 1e-6 of the peak): the
first and the last tap are the largest of the set, so one tap wrapped into the kept region or one sample missing from the
history costs about 1/sqrt(T) of the output norm."""
import numpy as np
import pytest

from matrix_util import TOL, as_c, as_iq, check, edge_taps, signal

OVERLAPS = (256, 512, 1024, 2048, 3072)  # SPEC §6: overlap = the smallest of these that is >= T - 1 (overlap-save: T <= 3073)
BLOCK = 4096
BOUNDARY_TAPS = (1, 2, 3, 256, 257, 258, 512, 513, 514, 1024, 1025, 1026, 2048, 2049, 2050, 3072, 3073)
GENERIC_TAPS = BOUNDARY_TAPS + (3074, 4095, 4096)
GENERIC_L = (3, 7, 33, 63, 64)
NCO_FREQS = (0.37, -0.21, 1 / 4096, -0.4999, 0.123456)


@pytest.fixture(scope="module")
def torch_cuda(gpu_ok):
    import torch
    torch.cuda.set_device(0)
    return torch


def overlap_of(T):
    return min(o for o in OVERLAPS if o >= T - 1)


def rows_of(T):
    return overlap_of(T) // 64


def zero_stuffed(x, L):
    x = np.asarray(x, dtype=np.float32).reshape(-1, 2)
    u = np.zeros((x.shape[0] * L, 2), dtype=np.float32)
    u[::L] = x
    return u.reshape(-1)


def reference(oracle, taps, x, L, complex_taps=False, word=0, first_out=0):
    """float64: y'[n] = exp(+j 2 pi P n / 2^32) sum_k h[k] u[n-k], n = first_out + output index; x = float32 samples"""
    u = zero_stuffed(x, L)
    if complex_taps:
        t = np.asarray(taps, dtype=np.float32).reshape(-1, 2)
        y = as_c(oracle.fir_f64(np.ascontiguousarray(t[:, 0]), u, 1)) + 1j * as_c(oracle.fir_f64(np.ascontiguousarray(t[:, 1]), u, 1))
    else:
        y = as_c(oracle.fir_f64(taps, u, 1))
    if word:
        n = (np.arange(y.size, dtype=np.uint64) + np.uint64(first_out % (1 << 32))) % np.uint64(1 << 32)
        ph = (n * np.uint64(word)) % np.uint64(1 << 32)
        y = y * np.exp(2j * np.pi * ph.astype(np.float64) / 4294967296.0)
    return as_iq(y)


def make(fir, taps, L, form, ct, n, i16=False, freq=0.0):
    """a development-library context on the form asked for; asserts the backend AUTO chose first"""
    T = taps.size // (2 if ct else 1)
    f = fir.IfFirInterp(taps, L, max_samples=n, complex_taps=ct, dev=True)
    try:
        auto = fir.BACKEND_HIP_FFT if (T <= 3073 and 64 % L == 0) else fir.BACKEND_HIP_GENERIC
        assert f.get_backend() == auto, (T, L, f.get_backend())
        if form == "generic":
            f.set_backend(fir.BACKEND_HIP_GENERIC)
            assert f.get_backend() == fir.BACKEND_HIP_GENERIC
        else:
            assert auto == fir.BACKEND_HIP_FFT
            f.debug_config(force_full=(form == "full"))
        if i16:
            f.set_input_format(fir.INPUT_I16)
        if freq:
            f.set_nco(freq)
    except Exception:
        f.close()
        raise
    return f


def run_pieces(f, raw, sizes):
    """process raw (interleaved) in pieces of the given sample counts, then the rest"""
    parts, pos = [], 0
    for s in sizes:
        parts.append(f.process(raw[2 * pos:2 * (pos + s)]))
        pos += s
    if 2 * pos < raw.size:
        parts.append(f.process(raw[2 * pos:]))
    return np.concatenate(parts)


# ---------------------------------------------------------------- B: every instantiation, every boundary

def cases():
    """(T, L, form, complex taps, int16, NCO).  Overlap-save: every boundary tap count x every L | 64 in the full form, every
    L >= 4 in the small form; generic: those tap counts and 3074, 4095, 4096 x L in 3, 7, 33, 63, 64.  The flags cycle so
    that every (rows, int16, NCO, form) and every generic (int16, complex taps, NCO) comes up (asserted below)."""
    out = []
    for ti, T in enumerate(BOUNDARY_TAPS):
        for form in ("small", "full"):
            for li, L in enumerate((4, 8, 16, 32, 64) if form == "small" else (1, 2, 4, 8, 16, 32, 64)):
                c = li + 3 * (ti % 3) + (form == "full")
                out.append((T, L, form, bool((c >> 2) & 1) ^ bool(ti % 2), bool(c & 1), bool((c >> 1) & 1)))
    for ti, T in enumerate(GENERIC_TAPS):
        for li, L in enumerate(GENERIC_L):
            c = li + 5 * ti
            out.append((T, L, "generic", bool((c >> 2) & 1), bool(c & 1), bool((c >> 1) & 1)))
    return out


def _coverage():
    os_units = {(rows_of(T), i16, nco, form == "small") for T, L, form, ct, i16, nco in cases() if form != "generic"}
    generic_units = {(i16, ct, nco) for T, L, form, ct, i16, nco in cases() if form == "generic"}
    ct_by_rows = {(rows_of(T), nco) for T, L, form, ct, i16, nco in cases() if form != "generic" and ct}
    return os_units, generic_units, ct_by_rows


# every fir_interp_kernel<ROWS, I16, NCO, SMALL> and every fir_interp_generic_kernel<I16, CT, NCO> the library compiles
_B = (False, True)
assert _coverage()[0] == {(r, a, b, c) for r in (4, 8, 16, 32, 48) for a in _B for b in _B for c in _B}
assert _coverage()[1] == {(a, b, c) for a in _B for b in _B for c in _B}
assert _coverage()[2] == {(r, b) for r in (4, 8, 16, 32, 48) for b in _B}              # complex taps: each rows class, NCO on and off
assert {L for T, L, form, *_ in cases() if form == "small"} == {4, 8, 16, 32, 64}
assert {L for T, L, form, *_ in cases() if form == "full"} == {1, 2, 4, 8, 16, 32, 64}
assert {T for T, L, form, *_ in cases() if form == "small"} == set(BOUNDARY_TAPS) == {T for T, L, form, *_ in cases() if form == "full"}
assert {(1, 64), (3, 16)} <= {(T, L) for T, L, form, *_ in cases() if form != "generic"}  # T < L: most phases have no tap


def test_the_case_list_reaches_every_instantiation():
    os_units, generic_units, ct_by_rows = _coverage()
    assert len(os_units) == 40 and len(generic_units) == 8 and len(ct_by_rows) == 10
    assert all(overlap_of(T) == o for T, o in ((1, 256), (257, 256), (258, 512), (513, 512), (514, 1024), (1025, 1024), (1026, 2048),
                                                 (2049, 2048), (2050, 3072), (3073, 3072)))


def case_samples(T, L, form):
    """about ten blocks of the overlap-save kernel and a ragged rest: 10^4 to 4 10^4 outputs"""
    if form == "generic":
        return 20_000 // L + 37
    return 10 * (BLOCK - overlap_of(T)) // L + 37


@pytest.mark.gpu
@pytest.mark.parametrize("T,L,form,ct,i16,nco", cases())
def test_matrix_against_float64(gpu_ok, fir, oracle, T, L, form, ct, i16, nco):
    n = case_samples(T, L, form)
    raw, x = signal(oracle, n, i16)
    taps = edge_taps(T, L, ct)
    freq = NCO_FREQS[(T + L) % len(NCO_FREQS)] if nco else 0.0
    cut = n // 3
    if form != "generic" and cut % ((BLOCK - overlap_of(T)) // L) == 0:
        cut += 1
    with make(fir, taps, L, form, ct, n, i16, freq) as f:
        y = run_pieces(f, raw, [cut])
    assert y.size == 2 * n * L
    ref = reference(oracle, taps, x, L, ct, oracle.nco_phase_word(freq) if nco else 0)
    check(oracle, y, ref, ("rows", rows_of(T) if T <= 3073 else 0, form, T, L, ct, i16, nco))


# ---------------------------------------------------------------- C: call sizes and streaming state

ROWS_TAPS = {4: 257, 8: 513, 16: 1025, 32: 2049, 48: 3073}  # T - 1 = overlap: the longest filter of each rows class


@pytest.mark.gpu
@pytest.mark.parametrize("rows,form,L", [(4, "small", 4), (8, "small", 8), (16, "small", 64), (32, "small", 32), (48, "small", 16),
                                         (4, "full", 1), (8, "full", 2), (16, "full", 4), (32, "full", 64), (48, "full", 1)])
def test_single_calls_round_a_block(gpu_ok, fir, oracle, rows, form, L):
    """one call of n samples after a reset, n round the samples a block advances by (a_in = (4096 - overlap) / L)"""
    T = ROWS_TAPS[rows]
    a_in = (BLOCK - 64 * rows) // L
    i16 = form == "full"
    raw, x = signal(oracle, 3 * a_in, i16)
    taps = edge_taps(T, L, rows in (8, 32))
    with make(fir, taps, L, form, rows in (8, 32), 3 * a_in, i16, 0.37 if rows >= 16 else 0.0) as f:
        for n in (1, 2, a_in - 1, a_in, a_in + 1, 2 * a_in, 2 * a_in + 1, 3 * a_in - 1):
            f.reset()
            y = f.process(raw[:2 * n])
            assert y.size == 2 * n * L
            ref = reference(oracle, taps, x[:2 * n], L, rows in (8, 32), oracle.nco_phase_word(0.37) if rows >= 16 else 0)
            check(oracle, y, ref, ("single", rows, form, L, n))


SHORT_PIECES = [(T, L, i16, backend) for T, L in ((3073, 1), (3073, 4), (2049, 2)) for i16 in (False, True)
                for backend in ("overlap-save", "generic")]
# one tap at an L that does not divide 64: the generic kernel reads ceil((T - 1) / L) = 0 samples of the history
SHORT_PIECES.append((1, 3, False, "generic"))


@pytest.mark.gpu
@pytest.mark.parametrize("T,L,i16,backend", SHORT_PIECES)
def test_pieces_shorter_than_the_history(gpu_ok, fir, oracle, T, L, i16, backend):
    """hist_len = ceil(overlap / L) input samples (3072, 768, 1024): a piece shorter than that shifts the old history instead of
    replacing it.  Overlap-save in its production form (small for L = 4, full for L = 1, 2).  T = 1 is the filter with no
    history: 1000 samples in one call, and as 1 + 999, are taps[0] times the zero-stuffed input, exactly."""
    hist = -(-overlap_of(T) // L)
    assert fir.debug_interp_plan(T, L)[1] == hist
    sizes = [1, 1, 5, 100, hist - 1, 1, hist + 1, 2, hist // 2, 3, 2 * hist + 7, hist - 100, hist]
    n = sum(sizes) + 1501
    if T == 1:
        sizes, n = [1], 1000
    raw, x = signal(oracle, n, i16)
    taps = edge_taps(T, L, False)
    form = "generic" if backend == "generic" else ("small" if L >= 4 else "full")
    with make(fir, taps, L, form, False, n, i16) as f:
        y = run_pieces(f, raw, sizes)
        if backend == "generic":
            f.reset()
            one = f.process(raw)
            assert np.array_equal(y, one), np.max(np.abs(y - one))
    if T == 1:
        assert np.array_equal(y, taps[0] * zero_stuffed(x, L))
    check(oracle, y, reference(oracle, taps, x, L), ("short pieces", T, L, i16, backend))


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["small", "full", "generic"])
def test_zero_sample_calls(gpu_ok, fir, oracle, torch_cuda, form):
    """a call with 0 samples succeeds, returns 0 outputs and leaves the stream as it was: if_fir_interp_process and
    if_fir_interp_process_device"""
    torch = torch_cuda
    T, L, n, cut = 513, 8, 5001, 1778   # (cut even: the generic kernel wants 16-byte pointers)
    raw, x = signal(oracle, n, False)
    taps = edge_taps(T, L, True)
    with make(fir, taps, L, form, True, n, False, 0.37) as f:
        plain = run_pieces(f, raw, [cut])
        f.reset()
        parts = [f.process(raw[:0]), f.process(raw[:2 * cut]), f.process(raw[:0]), f.process(raw[:0]), f.process(raw[2 * cut:]),
                 f.process(raw[:0])]
        assert [p.size for p in parts] == [0, 2 * cut * L, 0, 0, 2 * (n - cut) * L, 0]
        assert np.array_equal(np.concatenate(parts), plain)
        f.reset()
        din = torch.from_numpy(raw).cuda()
        out = torch.full((2 * n * L + 16,), 777.0, dtype=torch.float32, device="cuda")
        assert f.process_device(din.data_ptr(), out.data_ptr(), 0) == 0
        assert f.process_device(din.data_ptr(), out.data_ptr(), cut) == cut * L
        assert f.process_device(din.data_ptr() + 8 * cut, out.data_ptr() + 8 * cut * L, 0) == 0
        assert f.process_device(0, 0, 0) == 0
        assert f.process_device(din.data_ptr() + 8 * cut, out.data_ptr() + 8 * cut * L, n - cut) == (n - cut) * L
        f.synchronize()
        h = out.cpu().numpy()
        assert np.all(h[2 * n * L:] == 777.0)
        assert np.array_equal(h[:2 * n * L], plain)
    check(oracle, plain, reference(oracle, taps, x, L, True, oracle.nco_phase_word(0.37)), ("zero-sample", form))


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["small", "full", "generic"])
@pytest.mark.parametrize("T", [513, 2049])
@pytest.mark.parametrize("between", [False, True])
def test_nco_across_pieces(gpu_ok, fir, oracle, T, form, between):
    """int16 input, complex taps, rows 8 and 32: the up-mix phase continues over ragged pieces; set between two pieces it
    "takes effect from the next call, as if set since the last reset" (include/if_fir.h): phase P n, n the absolute output index"""
    L, freq = 8, -0.21
    a_in = (BLOCK - overlap_of(T)) // L
    sizes = [a_in + 3, 1, 2 * a_in - 1, 37]
    n = sum(sizes) + 3 * a_in + 11
    raw, x = signal(oracle, n, True)
    taps = edge_taps(T, L, True)
    word = oracle.nco_phase_word(freq)
    with make(fir, taps, L, form, True, n, True, 0.0 if between else freq) as f:
        if between:
            first = f.process(raw[:2 * sizes[0]])
            f.set_nco(freq)
            y = np.concatenate([first, run_pieces(f, raw[2 * sizes[0]:], sizes[1:])])
        else:
            y = run_pieces(f, raw, sizes)
    ref = reference(oracle, taps, x, L, True, word)
    if between:
        ref[:2 * sizes[0] * L] = reference(oracle, taps, x, L, True)[:2 * sizes[0] * L]
    check(oracle, y, ref, ("nco pieces", T, form, between))


@pytest.mark.gpu
@pytest.mark.parametrize("form,i16", [("full", False), ("full", True), ("small", True), ("generic", True)])
def test_nco_past_output_index_2_32_full_form_and_int16(gpu_ok, fir, oracle, form, i16):
    """the absolute output index mod 2^32 through the development seek hook: a window across 2^32"""
    L, T, n = 16, 513, 20_000
    raw, x = signal(oracle, n, i16)
    taps = edge_taps(T, L, True)
    first_in = (1 << 32) // L - 5000
    with make(fir, taps, L, form, True, n, i16, 0.37) as f:
        f.debug_seek(first_in)
        y = run_pieces(f, raw, [4999, 1, 1])            # (the third piece starts on output index 2^32)
    ref = reference(oracle, taps, x, L, True, oracle.nco_phase_word(0.37), first_out=first_in * L)
    check(oracle, y, ref, ("nco 2^32", form, i16))


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["small", "full"])
@pytest.mark.parametrize("i16", [False, True])
def test_sample_aligned_device_pointers(gpu_ok, fir, oracle, torch_cuda, form, i16):
    """include/if_fir.h: the overlap-save backend takes pointers aligned to one sample: input + 8 bytes (int16: + 4), output + 8"""
    torch = torch_cuda
    T, L, n, pad = 1025, 4, 5001, 4096
    raw, x = signal(oracle, n, i16)
    taps = edge_taps(T, L, False)
    din = torch.zeros(raw.size + 2, dtype=torch.int16 if i16 else torch.float32, device="cuda")
    din[2:] = torch.from_numpy(raw).cuda()
    off_in = 4 if i16 else 8
    with make(fir, taps, L, form, False, n, i16, 0.123456) as f:
        m = n * L
        a = torch.full((2 * (m + 2 * pad),), 12345.0, dtype=torch.float32, device="cuda")
        assert f.process_device(din.data_ptr() + off_in, a.data_ptr() + 8 * pad, n) == m      # output on 16 bytes
        f.synchronize()
        f.reset()
        b = torch.full((2 * (m + 2 * pad) + 2,), 12345.0, dtype=torch.float32, device="cuda")
        assert (b.data_ptr() + 8 * pad + 8) % 16 == 8
        assert f.process_device(din.data_ptr() + off_in, b.data_ptr() + 8 * pad + 8, n) == m
        f.synchronize()
        aligned = torch.from_numpy(raw).cuda()
        f.reset()
        c = torch.empty(2 * m, dtype=torch.float32, device="cuda")
        f.process_device(aligned.data_ptr(), c.data_ptr(), n)
        f.synchronize()
    ha, hb, hc = a.cpu().numpy(), b.cpu().numpy(), c.cpu().numpy()
    assert np.all(ha[:2 * pad] == 12345.0) and np.all(ha[2 * pad + 2 * m:] == 12345.0)
    assert np.all(hb[:2 * pad + 2] == 12345.0) and np.all(hb[2 * pad + 2 + 2 * m:] == 12345.0)
    assert np.array_equal(ha[2 * pad:2 * pad + 2 * m], hc)
    assert np.array_equal(hb[2 * pad + 2:2 * pad + 2 + 2 * m], hc)
    check(oracle, hc, reference(oracle, taps, x, L, False, oracle.nco_phase_word(0.123456)), ("sample-aligned", form, i16))


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["small", "generic"])
def test_caller_stream(gpu_ok, fir, oracle, torch_cuda, form):
    """if_fir_interp_set_stream: the launches go to a caller-owned stream, ordered after the caller's own work on it"""
    torch = torch_cuda
    T, L, n = 257, 4, 20_000
    raw, x = signal(oracle, n, False)
    taps = edge_taps(T, L, False)
    s = torch.cuda.Stream()
    with make(fir, taps, L, form, False, n) as f, torch.cuda.stream(s):
        f.set_stream(s.cuda_stream)
        host = torch.from_numpy(raw).pin_memory()
        din = torch.empty(raw.size, dtype=torch.float32, device="cuda")
        out = torch.empty(2 * n * L, dtype=torch.float32, device="cuda")
        din.copy_(host, non_blocking=True)                 # on s: the kernel must wait for it
        assert f.process_device(din.data_ptr(), out.data_ptr(), n // 2) == (n // 2) * L
        assert f.process_device(din.data_ptr() + 8 * (n // 2), out.data_ptr() + 8 * (n // 2) * L, n - n // 2) == (n - n // 2) * L
        s.synchronize()
        y = out.cpu().numpy()
        f.set_stream(0)                                    # back to the context's own stream
        f.reset()
        assert np.array_equal(run_pieces(f, raw, [n // 2]), y)
    check(oracle, y, reference(oracle, taps, x, L), ("caller stream", form))


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["small", "generic"])
def test_stream_capture_is_refused(gpu_ok, fir, oracle, torch_cuda, form):
    """a call carries host-side streaming state (sample index, phase, history ping-pong): a capturing stream is refused with
    a message, nothing is launched, and the context goes on afterwards"""
    torch = torch_cuda
    T, L, n = 257, 4, 8192
    raw, x = signal(oracle, n, False)
    taps = edge_taps(T, L, False)
    din = torch.from_numpy(raw).cuda()
    with make(fir, taps, L, form, False, n) as f:
        out = torch.empty(2 * n * L, dtype=torch.float32, device="cuda")
        s = torch.cuda.Stream()
        f.set_stream(s.cuda_stream)
        f.process_device(din.data_ptr(), out.data_ptr(), n // 2)
        f.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(s):
            g.capture_begin()
            try:
                with pytest.raises(fir.IfFirError, match="captured"):
                    f.process_device(din.data_ptr() + 8 * (n // 2), out.data_ptr() + 8 * (n // 2) * L, n - n // 2)
            finally:
                g.capture_end()
        # the refused call consumed nothing: the stream goes on where it was
        f.process_device(din.data_ptr() + 8 * (n // 2), out.data_ptr() + 8 * (n // 2) * L, n - n // 2)
        f.synchronize()
        y = out.cpu().numpy()
    check(oracle, y, reference(oracle, taps, x, L), ("capture refused", form))


# ---------------------------------------------------------------- D: large runs

def device_input(torch, oracle, n, i16):
    """n input samples on the device: 2^22 oracle samples (int16: with full-scale ones) repeated"""
    base = 1 << 22
    raw, _ = signal(oracle, min(n, base), i16)
    t = torch.from_numpy(raw).cuda()
    if n > base:
        t = t.repeat((n + base - 1) // base)[:2 * n].contiguous()
    return t


def window_check(oracle, torch, ys, din, i16, taps, T, L, ct, word, o, what, count=8192):
    """outputs o .. o + count of a one-call run against float64 (input read back from the device)"""
    n = din.numel() // 2
    j_lo = max(0, (o - (T - 1)) // L)
    j_hi = min(n, (o + count) // L + 1)
    xin = din[2 * j_lo:2 * j_hi].cpu().numpy()
    if i16:
        xin = xin.astype(np.float32) * np.float32(2.0 ** -15)
    ref = reference(oracle, taps, xin, L, ct, word, first_out=j_lo * L)
    ref = ref[2 * (o - j_lo * L):2 * (o - j_lo * L + count)]
    got = ys[2 * o:2 * (o + count)].cpu().numpy()
    check(oracle, got, ref, what + (o,))


def device_compare(torch, ya, yb):
    """(relative L2, relative max) of two device buffers, in slices of 2^25 floats"""
    num = den = 0.0
    mxd = mxr = 0.0
    for lo in range(0, ya.numel(), 1 << 25):
        a, b = ya[lo:lo + (1 << 25)].double(), yb[lo:lo + (1 << 25)].double()
        num += ((a - b) ** 2).sum().item()
        den += (b ** 2).sum().item()
        mxd = max(mxd, (a - b).abs().max().item())
        mxr = max(mxr, b.abs().max().item())
    return (num / den) ** 0.5, mxd / mxr


@pytest.mark.gpu
def test_one_call_beyond_2_32_output_bytes_small_form(gpu_ok, fir, oracle, torch_cuda):
    """2^29 + A + 5 outputs (rounded up to a multiple of L) at L = 16 in one call, 4.3 GB: windows against float64 at the
    start, across output index 2^29 (byte offset 2^32) and at the tail; a canary after the last output; the whole buffer
    against the full form, run in slices cut at multiples of A / L inputs"""
    torch = torch_cuda
    T, L, pad = 257, 16, 1 << 16
    A = BLOCK - overlap_of(T)
    n = ((1 << 29) + A + 5 + L - 1) // L
    M = n * L
    assert 8 * M > 1 << 32
    taps = edge_taps(T, L, False)
    din = device_input(torch, oracle, n, False)
    ys = torch.empty(2 * (M + pad), dtype=torch.float32, device="cuda")
    ys[2 * M:] = 12345.0
    with make(fir, taps, L, "small", False, 1 << 10) as f:
        assert f.process_device(din.data_ptr(), ys.data_ptr(), n) == M
        f.synchronize()
        assert bool((ys[2 * M:] == 12345.0).all())
        for o in (0, (1 << 29) - 3 * 8192, M - 8192):          # (the tail window lies across output index 2^29)
            assert o + 8192 <= M and (o == 0 or M - 8192 < 1 << 29 < M)
            window_check(oracle, torch, ys, din, False, taps, T, L, False, 0, o, ("beyond 2^32 bytes", "small"))
        f.reset()
        f.debug_config(force_full=True)
        a_in = A // L
        step = a_in * ((1 << 26) // A)
        tmp = torch.empty(2 * step * L, dtype=torch.float32, device="cuda")
        num = den = mxd = mxr = 0.0
        for j in range(0, n, step):
            k = min(step, n - j)
            assert f.process_device(din.data_ptr() + 8 * j, tmp.data_ptr(), k) == k * L
            f.synchronize()
            a, b = ys[2 * j * L:2 * (j + k) * L], tmp[:2 * k * L]
            for lo in range(0, a.numel(), 1 << 25):
                da, db = a[lo:lo + (1 << 25)].double(), b[lo:lo + (1 << 25)].double()
                num += ((da - db) ** 2).sum().item()
                den += (db ** 2).sum().item()
                mxd = max(mxd, (da - db).abs().max().item())
                mxr = max(mxr, db.abs().max().item())
    l2, mx = (num / den) ** 0.5, mxd / mxr
    print("interp-matrix", ("beyond 2^32 bytes", "small against full"), "l2=%.3g max=%.3g" % (l2, mx))
    assert l2 <= TOL and mx <= TOL, (l2, mx)


@pytest.mark.gpu
def test_one_call_beyond_2_32_output_bytes_generic(gpu_ok, fir, oracle, torch_cuda):
    """the generic kernel at L = 5, just above 2^29 outputs in one call"""
    torch = torch_cuda
    T, L, pad = 33, 5, 1 << 16
    n = (1 << 29) // L + 2001
    M = n * L
    assert 8 * M > 1 << 32
    taps = edge_taps(T, L, False)
    din = device_input(torch, oracle, n, False)
    ys = torch.empty(2 * (M + pad), dtype=torch.float32, device="cuda")
    ys[2 * M:] = 12345.0
    with make(fir, taps, L, "generic", False, 1 << 10) as f:
        assert f.process_device(din.data_ptr(), ys.data_ptr(), n) == M
        f.synchronize()
    assert bool((ys[2 * M:] == 12345.0).all())
    for o in (0, (1 << 29) - 4096, (1 << 29), M - 8192):
        window_check(oracle, torch, ys, din, False, taps, T, L, False, 0, o, ("beyond 2^32 bytes", "generic"))


@pytest.mark.gpu
@pytest.mark.parametrize("L,T,form,other,ct,i16,freq", [(1, 257, "full", "generic", False, False, 0.0),
                                                        (2, 513, "full", "generic", False, False, 0.0),
                                                        (64, 257, "small", "full", False, False, 0.0),
                                                        (8, 257, "small", "full", True, True, 0.37)])
def test_full_size_on_the_other_paths(gpu_ok, fir, oracle, torch_cuda, L, T, form, other, ct, i16, freq):
    """2^28 outputs in one call: L = 1 and L = 2 (the full form is their production path), L = 64 small, int16 with complex
    taps and the NCO at L = 8: windows against float64, the whole buffer against the other form / the generic kernel"""
    torch = torch_cuda
    M = 1 << 28
    n = M // L
    taps = edge_taps(T, L, ct)
    word = oracle.nco_phase_word(freq) if freq else 0
    din = device_input(torch, oracle, n, i16)
    ys = torch.empty(2 * M, dtype=torch.float32, device="cuda")
    with make(fir, taps, L, form, ct, 1 << 10, i16, freq) as f:
        assert f.process_device(din.data_ptr(), ys.data_ptr(), n) == M
        f.synchronize()
    for o in (0, (M // 3) // L * L + 1, M - 8192):
        window_check(oracle, torch, ys, din, i16, taps, T, L, ct, word, o, ("full size", L, form))
    yo = torch.empty(2 * M, dtype=torch.float32, device="cuda")
    with make(fir, taps, L, other, ct, 1 << 10, i16, freq) as f:
        assert f.process_device(din.data_ptr(), yo.data_ptr(), n) == M
        f.synchronize()
    l2, mx = device_compare(torch, ys, yo)
    print("interp-matrix", ("full size", L, form, "against", other), "l2=%.3g max=%.3g" % (l2, mx))
    assert l2 <= TOL and mx <= TOL, (L, form, other, l2, mx)


# ---------------------------------------------------------------- E: random configurations

def random_draws(count=40, seed=20260):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        L = int(rng.integers(1, 65)) if rng.integers(2) else 1 << int(rng.integers(0, 7))  # (half of the draws on an L | 64)
        T = int(min(4096, max(1, round(float(np.exp(rng.uniform(0.0, np.log(4096.0))))))))
        ct, i16 = bool(rng.integers(2)), bool(rng.integers(2))
        freq = float(rng.uniform(-0.5, 0.5)) if rng.integers(2) else 0.0
        forms = ["generic"]
        if T <= 3073 and 64 % L == 0:
            forms += ["full"] + (["small"] if L >= 4 else [])
        form = forms[int(rng.integers(len(forms)))]
        n = 30_000 // L + 50
        cuts = sorted(int(c) for c in rng.integers(0, n + 1, size=int(rng.integers(0, 5))))
        sizes = [b - a for a, b in zip([0] + cuts, cuts)]
        out.append((L, T, ct, i16, freq, form, n, tuple(sizes)))
    return out


@pytest.mark.gpu
def test_random_configurations_against_float64(gpu_ok, fir, oracle):
    """40 seeded draws: L in 1..64, T log-uniform in 1..4096, real or complex taps, float32 or int16 input, NCO off or anywhere
    in +-0.5, the form where there is a choice, 1 to 5 ragged pieces (a piece may be empty)"""
    for draw in random_draws():
        L, T, ct, i16, freq, form, n, sizes = draw
        raw, x = signal(oracle, n, i16)
        taps = edge_taps(T, L, ct, seed=1)
        with make(fir, taps, L, form, ct, n, i16, freq) as f:
            y = run_pieces(f, raw, sizes)
        assert y.size == 2 * n * L, draw
        ref = reference(oracle, taps, x, L, ct, oracle.nco_phase_word(freq) if freq else 0)
        l2, mx = oracle.err_metrics(y, ref)
        print("interp-matrix", ("random",) + draw[:6], "l2=%.3g max=%.3g" % (l2, mx))
        assert l2 <= TOL and mx <= TOL, (draw, l2, mx)
