"""The real-input polyphase filter bank (if_fir_rpfb_t, docs/SPEC.md §17) on the GPU against the float64 fold form of
tests/rpfb_ref.py (which tests/test_rpfb_host.py holds to the definition and to oracle.fir_nco_f64 at 1e-12), SPEC §3 tolerance
over the whole output; the real bins, bin spans, the routes it replaces, stream cuts, grid limits and stream positions past 2^32
bit for bit.  Device output buffers carry a sentinel guard behind their last value, and the guard is checked."""
import functools

import numpy as np
import pytest

import ddc_ref
import rpfb_ref
from matrix_util import row_edge_taps
from test_pfb_gpu import ragged_pieces

TOL = 1e-6          # SPEC §17: §3's bound over all channels of all frames together (the float32 model stays below 5e-7)
GUARD = 64          # float32 words behind the last output
SENTINEL = 12345.0
# (M, T, D): every M with K = 16 rows at D = M (the longest prototype) and K = 3 rows, T off the multiple of M, at D = M/2; then
# an odd hop that divides nothing, an odd hop one short of M, D = 1, a non-divisor hop with T one short of 4 M, a single tap, and
# T off the multiple at M = 8192
MATRIX = tuple((M, 16 * M, M) for M in rpfb_ref.SIZES) + tuple((M, 3 * M - 5, M // 2) for M in rpfb_ref.SIZES) + (
    (128, 187, 17), (256, 2047, 255), (512, 1017, 1), (1024, 4095, 768), (2048, 1, 2048), (8192, 65340, 4096))


def frames_of(M, D):
    return 24 if M < 4096 else 12


def stream_len(M, T, D):
    """24 frames at D > 1 (12 from M = 4096 up; the last one's hop cut short); at D = 1 a lead-in of T - 1 samples and then 200
    frames, so that those 200 weigh the whole prototype"""
    return (frames_of(M, D) - 1) * D + 1 + (D - 1) // 2 if D > 1 else T - 1 + 200


@pytest.fixture(scope="module")
def torch_cuda(gpu_ok):
    import torch
    torch.cuda.set_device(0)
    return torch


def oracle_mod():
    import __graft_entry__ as g
    return g.load_oracle()


def signal(n, i16):
    """(what the context is fed, the same samples as float32): REAL samples; int16 with full-scale samples"""
    return ddc_ref.real_signal(oracle_mod(), n, i16)


@functools.lru_cache(maxsize=None)
def reference(M, T, D, i16, n, first=0):
    ref = rpfb_ref.fold_f64(row_edge_taps(T, M, False), signal(n, i16)[1], M, D, first=first)
    ref.setflags(write=False)
    return ref


def run_device(torch, f, raw, pieces, first=0, formats=None):
    """feed `raw` from ONE device buffer in consecutive pieces (sample-aligned offsets) to a context at absolute index `first`;
    returns ((frames, bins) complex64, frames per piece).  With `formats` (one input format per piece, set before that piece)
    `raw` maps each format to the stream in that format: the same values in every one, one device buffer each.  frame_count is
    checked at every step, and the guard behind the last output after the last."""
    both = {None: raw} if formats is None else raw
    n = next(iter(both.values())).size
    assert all(v.size == n for v in both.values()) and sum(pieces) == n
    din = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in both.items()}
    D, bins = f.hop, f.bins
    total = rpfb_ref.frame_count(first, n, D)
    buf = torch.full((2 * total * bins + GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
    pos = done = 0
    counts = []
    for k, s in enumerate(pieces):
        if formats is not None:
            f.set_input_format(formats[k])
        src = din[None if formats is None else formats[k]]
        want = f.frame_count(s)
        got = f.process_device(src.data_ptr() + src.element_size() * pos, buf.data_ptr() + 8 * done * bins, s)
        assert got == want == rpfb_ref.frame_count(first + pos, s, D), (pos, s, got, want)
        counts.append(got)
        pos += s
        done += got
    f.synchronize()
    assert pos == n and done == total
    h = buf.cpu().numpy()
    assert np.all(h[2 * total * bins:] == SENTINEL), "the guard behind the last output was written"
    return h[:2 * total * bins].view(np.complex64).reshape(total, bins).copy(), counts


def check(oracle, y, ref, what, tol=TOL):
    l2, mx = oracle.err_metrics(rpfb_ref.iq(y), rpfb_ref.iq(ref))
    print("rpfb %s: l2=%.3g max=%.3g" % (what, l2, mx))
    assert l2 <= tol and mx <= tol, (what, l2, mx)
    return l2, mx


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


@pytest.mark.gpu
@pytest.mark.parametrize("i16", [False, True])
@pytest.mark.parametrize("M,T,D", MATRIX)
def test_matrix_against_float64(gpu_ok, fir, oracle, torch_cuda, M, T, D, i16):
    """taps loud at both ends of every row; the host path in two calls within tolerance of float64 over the whole output, the
    device path the same bits"""
    n = stream_len(M, T, D)
    raw, _ = signal(n, i16)
    taps = row_edge_taps(T, M, False)
    cut = n // 3 + 1
    with fir.IfFirRpfb(taps, M, D, max_samples=n) as f:
        if i16:
            f.set_input_format(fir.INPUT_I16)
        y = np.concatenate([f.process(raw[:cut]), f.process(raw[cut:])])
        f.reset()
        yd, _ = run_device(torch_cuda, f, raw, [cut, n - cut])
    ref = reference(M, T, D, i16, n)
    assert y.shape == ref.shape == (frames_of(M, D) if D > 1 else n, M // 2 + 1)
    check(oracle, y, ref, "matrix M=%d T=%d D=%d i16=%d" % (M, T, D, i16))
    assert same_bits(yd, y)


@pytest.mark.gpu
@pytest.mark.parametrize("M", [128, 2048])
def test_real_bins_and_spans(gpu_ok, fir, oracle, torch_cuda, M):
    """bins 0 and M/2 are real: their imaginary part is exactly zero (of either sign); bin M/4, its own partner, is within
    tolerance; every span -- all bins, bin 0 alone, bin M/2 alone, three bins around M/4, a few from 5 -- equals the same
    columns of the full result bit for bit"""
    T, D = 3 * M - 5, M // 2
    n = stream_len(M, T, D)
    raw, _ = signal(n, False)
    taps = row_edge_taps(T, M, False)
    with fir.IfFirRpfb(taps, M, D, max_samples=n) as f:
        assert (f.first_bin, f.bins) == (0, M // 2 + 1)
        full, _ = run_device(torch_cuda, f, raw, [n])
    ref = reference(M, T, D, False, n)
    check(oracle, full, ref, "spans M=%d" % M)
    assert np.all(full[:, 0].imag == 0.0) and np.all(full[:, M // 2].imag == 0.0)
    assert np.max(np.abs(full[:, 0].real)) > 0 and np.max(np.abs(full[:, M // 2].real)) > 0
    peak = np.max(np.abs(ref))
    assert np.max(np.abs(full[:, M // 4] - ref[:, M // 4])) <= TOL * peak
    for first_bin, bins in ((0, M // 2 + 1), (0, 1), (M // 2, 1), (M // 4 - 1, 3), (5, 7)):
        with fir.IfFirRpfb(taps, M, D, first_bin=first_bin, bins=bins, max_samples=n) as f:
            y, _ = run_device(torch_cuda, f, raw, [n // 2, n - n // 2])
        assert y.shape == (frames_of(M, D), bins)
        assert same_bits(y, full[:, first_bin:first_bin + bins]), (first_bin, bins)


@pytest.mark.gpu
@pytest.mark.parametrize("M,T,D", [(1024, 3067, 512), (128, 379, 64)])
def test_against_the_complex_bank_fed_zeros(gpu_ok, fir, oracle, torch_cuda, M, T, D):
    """the route it replaces: IfFirPfb fed (r, 0), channels 0 .. M/2.  Both are within TOL of float64, so they are within
    2 TOL of the overall peak of each other"""
    n = stream_len(M, T, D)
    raw, x = signal(n, False)
    taps = row_edge_taps(T, M, False)
    with fir.IfFirRpfb(taps, M, D, max_samples=n) as f:
        y = f.process(raw)
    with fir.IfFirPfb(taps, M, D, first_bin=0, bins=M // 2 + 1, max_samples=n) as p:
        want = p.process(rpfb_ref.widen(x))
    assert y.shape == want.shape
    check(oracle, y, reference(M, T, D, False, n), "vs pfb M=%d (float64)" % M)
    check(oracle, y, want, "vs pfb M=%d" % M, tol=2 * TOL)


@pytest.mark.gpu
def test_against_the_down_converter_per_channel(gpu_ok, fir, oracle, torch_cuda):
    """SPEC §17's definition: channel k is IfFirDdc with its NCO at k / M, for k = 0, 5 and M/2; each within 2 TOL of the bank's
    overall peak"""
    M, T, D = 128, 1000, 48
    n = stream_len(M, T, D)
    raw, _ = signal(n, False)
    taps = row_edge_taps(T, M, False)
    with fir.IfFirRpfb(taps, M, D, max_samples=n) as f:
        y = f.process(raw)
    ref = reference(M, T, D, False, n)
    check(oracle, y, ref, "vs ddc M=%d (float64)" % M)
    peak = np.max(np.abs(ref))
    for k in (0, 5, M // 2):
        with fir.IfFirDdc(taps, D, max_samples=n) as d:
            d.set_nco(k / M)
            out = d.process(raw)
        want = out[0::2] + 1j * out[1::2]
        assert want.shape == y[:, k].shape
        err = np.max(np.abs(y[:, k] - want))
        print("rpfb vs ddc k=%d: max=%.3g of the peak" % (k, err / peak))
        assert err <= 2 * TOL * peak, (k, err, peak)


@pytest.mark.gpu
@pytest.mark.parametrize("M,T,D", [(1024, 8189, 385), (128, 2048, 128), (8192, 16383, 8191)])
def test_cuts_and_format_changes_bit_for_bit(gpu_ok, fir, oracle, torch_cuda, M, T, D):
    """the stream in ragged pieces (0-sample and 1-sample calls among them), the input format changed between them, against one
    call: the same bits, and frame_count equals the frames written at every step (run_device)"""
    n = 2 * T + 40 * D + 11
    xi, xf = signal(n, True)
    taps = row_edge_taps(T, M, False)
    pieces = ragged_pieces(n, T, D, np.random.default_rng([M, T, D]))
    formats = [(fir.INPUT_F32, fir.INPUT_I16)[(k // 2) % 2] for k in range(len(pieces))]
    with fir.IfFirRpfb(taps, M, D, max_samples=n) as f:
        one, _ = run_device(torch_cuda, f, xf, [n])
        check(oracle, one, reference(M, T, D, True, n), "cuts M=%d T=%d D=%d" % (M, T, D))
        f.reset()
        y, counts = run_device(torch_cuda, f, {fir.INPUT_F32: xf, fir.INPUT_I16: xi}, pieces, formats=formats)
        assert counts[0] == 0 and 0 in counts[1:] and max(counts) > 1
        assert same_bits(y, one)
        f.reset()
        f.set_input_format(fir.INPUT_I16)
        y, _ = run_device(torch_cuda, f, xi, [n])
        assert same_bits(y, one)


@pytest.mark.gpu
@pytest.mark.parametrize("M,T,D,frames", [(128, 187, 17, 150), (2048, 6139, 1024, 29), (8192, 8201, 8192, 19)])
def test_grid_limits_give_the_same_bits(gpu_ok, fir, oracle, torch_cuda, M, T, D, frames):
    """1 and 2 workgroups walk all runs of frames (more than two runs, the last one short): the bits of the default launch"""
    n = (frames - 1) * D + 1
    raw, _ = signal(n, False)
    with fir.IfFirRpfb(row_edge_taps(T, M, False), M, D, max_samples=n, dev=True) as f:
        group = f.debug_config()
        assert group >= 8 and frames > 2 * group and frames % group
        runs = []
        for limit in (0, 1, 2):
            f.debug_config(grid_limit=limit)
            f.reset()
            runs.append(run_device(torch_cuda, f, raw, [n])[0])
    check(oracle, runs[0], reference(M, T, D, False, n), "grid M=%d T=%d D=%d" % (M, T, D))
    assert runs[0].shape == (frames, M // 2 + 1)
    assert same_bits(runs[0], runs[1]) and same_bits(runs[0], runs[2])


@pytest.mark.gpu
@pytest.mark.parametrize("start", [(1 << 32) - 5, (1 << 40) + 12345])
@pytest.mark.parametrize("M,T,D", [(256, 2047, 255), (128, 187, 17)])
def test_stream_positions_past_2_32(gpu_ok, fir, oracle, torch_cuda, M, T, D, start):
    """through the development hook the context starts at an odd absolute index (so c mod M is odd: the slot pairs of the
    transform's input start on the other parity) that is a multiple of neither D nor M, with a zero history: the frame count is
    the reference's and the outputs are the reference evaluated at that position; a cut (across 2^32 for the first start) gives
    the same bits, and position 0 gives other values"""
    assert start % 2 and start % D and start % M
    n = 30 * D + 3
    for i16 in (False, True):
        raw, _ = signal(n, i16)
        with fir.IfFirRpfb(row_edge_taps(T, M, False), M, D, max_samples=n, dev=True) as f:
            if i16:
                f.set_input_format(fir.INPUT_I16)
            f.debug_config(position=start)
            assert f.frame_count(n) == rpfb_ref.frame_count(start, n, D)
            one, _ = run_device(torch_cuda, f, raw, [n], first=start)
            check(oracle, one, reference(M, T, D, i16, n, start), "position M=%d D=%d start=%d i16=%d" % (M, D, start, i16))
            f.debug_config(position=start)
            y, _ = run_device(torch_cuda, f, raw, [3, 4, 1, n - 8], first=start)
            assert same_bits(y, one)
            f.reset()
            zero, _ = run_device(torch_cuda, f, raw, [n])
            assert zero.shape != one.shape or not np.array_equal(zero, one)


@pytest.mark.gpu
@pytest.mark.filterwarnings("ignore:The CUDA Graph is empty")
def test_refusals_leave_the_stream_where_it_was(gpu_ok, fir, oracle, torch_cuda):
    torch = torch_cuda
    M, T, D, n = 256, 700, 100, 10_000
    raw, _ = signal(n, False)
    taps = row_edge_taps(T, M, False)
    for kw in (dict(channels=96), dict(channels=64), dict(channels=16384), dict(channels=0), dict(taps=np.ones(16 * M + 1, dtype=np.float32)),
               dict(taps=np.zeros(0, dtype=np.float32)), dict(hop=0), dict(hop=M + 1), dict(first_bin=M // 2 + 1, bins=1),
               dict(first_bin=1, bins=M // 2 + 1), dict(bins=0), dict(bins=M // 2 + 2)):
        args = dict(taps=taps, channels=M, hop=D)
        args.update(kw)
        with pytest.raises(fir.IfFirError) as e:
            fir.IfFirRpfb(**args)
        assert "if_fir_rpfb_init" in str(e.value), kw
    bins = M // 2 + 1
    with fir.IfFirRpfb(taps, M, D, max_samples=n) as f:
        whole = f.process(raw)
        f.reset()
        head = f.process(raw[:1001])
        with pytest.raises(fir.IfFirError, match="ullMaxSamples"):
            f.process(np.zeros(n + 1, dtype=np.float32))
        with pytest.raises(fir.IfFirError, match="format"):
            f.set_input_format(5)
        buf = torch.zeros(n + 8, dtype=torch.float32, device="cuda")
        out = torch.zeros(2 * bins * (n // D + 1), dtype=torch.float32, device="cuda")
        with pytest.raises(fir.IfFirError, match="aligned"):
            f.process_device(buf.data_ptr() + 2, out.data_ptr(), 100)
        with pytest.raises(fir.IfFirError, match="aligned"):
            f.process_device(buf.data_ptr(), out.data_ptr() + 4, 100)
        f.set_input_format(fir.INPUT_I16)
        with pytest.raises(fir.IfFirError, match="aligned"):
            f.process_device(buf.data_ptr() + 1, out.data_ptr(), 100)
        f.set_input_format(fir.INPUT_F32)
        with pytest.raises(fir.IfFirError, match="NULL"):
            f.process_device(0, out.data_ptr(), 100)
        with pytest.raises(fir.IfFirError, match="NULL"):
            f.process_device(buf.data_ptr(), 0, 100)
        side = torch.cuda.Stream()
        f.set_stream(side.cuda_stream)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            graph.capture_begin()
            try:
                with pytest.raises(fir.IfFirError, match="captured"):
                    f.process_device(buf.data_ptr(), out.data_ptr(), 100)
            finally:
                graph.capture_end()
        f.set_stream(0)
        # every refused call left the stream where it was
        tail = f.process(raw[1001:])
        assert same_bits(np.concatenate([head, tail]), whole)
    # a call that would carry the position past 2^64 is refused; the stream goes on and ends as an undisturbed one
    start = (1 << 64) - 1000
    with fir.IfFirRpfb(taps, M, D, max_samples=n, dev=True) as f, fir.IfFirRpfb(taps, M, D, max_samples=n, dev=True) as calm:
        for c in (f, calm):
            c.debug_config(position=start)
        a = f.process(raw[:600])
        with pytest.raises(fir.IfFirError, match="2\\^64"):
            f.process(raw[:401])
        assert f.frame_count(401) == 0
        b = f.process(raw[600:999])   # (to 2^64 - 1: a position of 2^64 itself has no representation)
        want = calm.process(raw[:999])
        assert want.shape[0] == rpfb_ref.frame_count(start, 999, D) > 0
        assert same_bits(np.concatenate([a, b]), want)
