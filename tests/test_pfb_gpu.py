"""The polyphase filter bank (if_fir_pfb_t, docs/SPEC.md §13) on the GPU against the float64 fold form of tests/pfb_ref.py (which
tests/test_pfb_host.py holds to the definition and to oracle.fir_nco_f64 at 1e-12), SPEC §3 tolerance over the whole output;
bin spans, stream cuts, grid limits and stream positions past 2^32 bit for bit.  Device output buffers carry a sentinel guard
behind their last value, and the guard is checked."""
import functools

import numpy as np
import pytest

import pfb_ref
from matrix_util import row_edge_taps, signal

TOL = 1e-6          # SPEC §13: §3's bound over all channels of all frames together (the complex64 model stays below 5e-7)
GUARD = 64          # float32 words behind the last output
SENTINEL = 12345.0
# (M, T, D): every M with K = 16 rows at D = M (the longest prototype) and K = 3 rows, T off the multiple of M, at D = M/2; then
# a hop that divides nothing, a hop one short of M, D = 1, a non-divisor hop with T one short of 4 M, a single tap, T < M, and
# T off the multiple at M = 4096
MATRIX = tuple((M, 16 * M, M) for M in pfb_ref.SIZES) + tuple((M, 3 * M - 5, M // 2) for M in pfb_ref.SIZES) + (
    (64, 187, 17), (256, 2047, 255), (512, 1017, 1), (1024, 4095, 768), (2048, 1, 2048), (2048, 2045, 1024), (4096, 32668, 2048))


def stream_len(T, D):
    """24 frames at D > 1 (the last one's hop cut short); at D = 1 a lead-in of T - 1 samples and then 200 frames, so that
    those 200 weigh the whole prototype"""
    return 23 * D + 1 + (D - 1) // 2 if D > 1 else T - 1 + 200


@pytest.fixture(scope="module")
def torch_cuda(gpu_ok):
    import torch
    torch.cuda.set_device(0)
    return torch


def oracle_mod():
    import __graft_entry__ as g
    return g.load_oracle()


@functools.lru_cache(maxsize=None)
def reference(M, T, D, i16, n, first=0):
    ref = pfb_ref.fold_f64(row_edge_taps(T, M, False), signal(oracle_mod(), n, i16)[1], M, D, first=first)
    ref.setflags(write=False)
    return ref


def run_device(torch, f, raw, pieces, first=0, formats=None):
    """feed `raw` from ONE device buffer in consecutive pieces to a context at absolute index `first`; returns ((frames, bins)
    complex64, frames per piece).  With `formats` (one input format per piece, set before that piece) `raw` maps each format
    to the stream in that format: the same values in every one, one device buffer each.  frame_count is checked at every step."""
    both = {None: raw} if formats is None else raw
    n = next(iter(both.values())).size // 2
    assert all(v.size == 2 * n for v in both.values())
    din = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in both.items()}
    D, bins = f.hop, f.bins
    total = pfb_ref.frame_count(first, n, D)
    buf = torch.full((2 * total * bins + GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
    pos = done = 0
    counts = []
    for k, s in enumerate(pieces):
        if formats is not None:
            f.set_input_format(formats[k])
        src = din[None if formats is None else formats[k]]
        want = f.frame_count(s)
        got = f.process_device(src.data_ptr() + 2 * src.element_size() * pos, buf.data_ptr() + 8 * done * bins, s)
        assert got == want == pfb_ref.frame_count(first + pos, s, D), (pos, s, got, want)
        counts.append(got)
        pos += s
        done += got
    f.synchronize()
    assert pos == n and done == total
    h = buf.cpu().numpy()
    assert np.all(h[2 * total * bins:] == SENTINEL), "the guard behind the last output was written"
    return h[:2 * total * bins].view(np.complex64).reshape(total, bins).copy(), counts


def check(oracle, y, ref, what):
    l2, mx = oracle.err_metrics(pfb_ref.iq(y), pfb_ref.iq(ref))
    print("pfb %s: l2=%.3g max=%.3g" % (what, l2, mx))
    assert l2 <= TOL and mx <= TOL, (what, l2, mx)
    return l2, mx


@pytest.mark.gpu
@pytest.mark.parametrize("i16", [False, True])
@pytest.mark.parametrize("M,T,D", MATRIX)
def test_matrix_against_float64(gpu_ok, fir, oracle, torch_cuda, M, T, D, i16):
    """taps loud at both ends of every row; the host path in two calls within tolerance of float64 over the whole output, the
    device path the same bits"""
    n = stream_len(T, D)
    raw, _ = signal(oracle, n, i16)
    taps = row_edge_taps(T, M, False)
    cut = n // 3 + 1
    with fir.IfFirPfb(taps, M, D, max_samples=n) as f:
        if i16:
            f.set_input_format(fir.INPUT_I16)
        y = np.concatenate([f.process(raw[:2 * cut]), f.process(raw[2 * cut:])])
        f.reset()
        yd, _ = run_device(torch_cuda, f, raw, [cut, n - cut])
    ref = reference(M, T, D, i16, n)
    assert y.shape == ref.shape == (24 if D > 1 else n, M)
    check(oracle, y, ref, "matrix M=%d T=%d D=%d i16=%d" % (M, T, D, i16))
    assert np.array_equal(yd.view(np.uint32), y.view(np.uint32))


@pytest.mark.gpu
@pytest.mark.parametrize("M", [1024, 64])
def test_bin_spans_are_columns_of_the_full_result(gpu_ok, fir, oracle, torch_cuda, M):
    """every span -- all bins from 0, all bins from -M/2, a few around DC (wrapping), one bin, two bins across M - 1 -> 0 --
    equals the same columns of the full result bit for bit"""
    T, D = 3 * M - 5, M // 2
    n = stream_len(T, D)
    raw, _ = signal(oracle, n, False)
    taps = row_edge_taps(T, M, False)
    with fir.IfFirPfb(taps, M, D, max_samples=n) as f:
        full, _ = run_device(torch_cuda, f, raw, [n])
    check(oracle, full, reference(M, T, D, False, n), "spans M=%d" % M)
    for first_bin, bins in ((0, M), (-M // 2, M), (-3, 7), (77 % M, 1), (M - 1, 2)):
        with fir.IfFirPfb(taps, M, D, first_bin=first_bin, bins=bins, max_samples=n) as f:
            y, _ = run_device(torch_cuda, f, raw, [n // 2, n - n // 2])
        cols = pfb_ref.channels(M, first_bin, bins)
        assert y.shape == (24, bins)
        assert np.array_equal(y.view(np.uint32), np.ascontiguousarray(full[:, cols]).view(np.uint32)), (first_bin, bins)


def ragged_pieces(n, T, D, rng):
    """0-sample and 1-sample calls, pieces shorter than D, one longer than T, then random ones"""
    head = [0, 1, max(D - 1, 1), 1, 0, T + 5, 3, max(D // 2, 1), 1, D, D + 1]
    rest = n - sum(head)
    assert rest > 4 * D
    cuts = np.sort(rng.integers(0, rest + 1, 5))
    return head + [int(v) for v in np.diff(np.concatenate([[0], cuts, [rest]]))]


@pytest.mark.gpu
@pytest.mark.parametrize("M,T,D", [(1024, 8 * 1024 - 3, 385), (64, 16 * 64, 64), (4096, 2 * 4096 - 1, 4095)])
def test_cuts_and_format_changes_bit_for_bit(gpu_ok, fir, oracle, torch_cuda, M, T, D):
    """the stream in ragged pieces, the input format changed between them, against one call: the same bits, and frame_count
    equals the frames written at every step (run_device)"""
    n = 2 * T + 40 * D + 11
    xi, xf = signal(oracle, n, True)
    taps = row_edge_taps(T, M, False)
    pieces = ragged_pieces(n, T, D, np.random.default_rng([M, T, D]))
    formats = [(fir.INPUT_F32, fir.INPUT_I16)[(k // 2) % 2] for k in range(len(pieces))]
    with fir.IfFirPfb(taps, M, D, max_samples=n) as f:
        one, _ = run_device(torch_cuda, f, xf, [n])
        check(oracle, one, reference(M, T, D, True, n), "cuts M=%d T=%d D=%d" % (M, T, D))
        f.reset()
        y, counts = run_device(torch_cuda, f, {fir.INPUT_F32: xf, fir.INPUT_I16: xi}, pieces, formats=formats)
        assert counts[0] == 0 and 0 in counts[1:] and max(counts) > 1
        assert np.array_equal(y.view(np.uint32), one.view(np.uint32))
        f.reset()
        f.set_input_format(fir.INPUT_I16)
        y, _ = run_device(torch_cuda, f, xi, [n])
        assert np.array_equal(y.view(np.uint32), one.view(np.uint32))


@pytest.mark.gpu
@pytest.mark.parametrize("M,T,D,frames", [(64, 187, 17, 150), (1024, 3 * 1024 - 5, 512, 29), (4096, 4096 + 9, 4096, 19), (128, 300, 1, 200)])
def test_grid_limits_give_the_same_bits(gpu_ok, fir, oracle, torch_cuda, M, T, D, frames):
    """1 and 2 workgroups walk all runs of frames (more than two runs, the last one short): the bits of the default launch"""
    n = (frames - 1) * D + 1
    raw, _ = signal(oracle, n, False)
    with fir.IfFirPfb(row_edge_taps(T, M, False), M, D, max_samples=n, dev=True) as f:
        group = f.debug_config()
        assert group >= 8 and frames > 2 * group and frames % group
        runs = []
        for limit in (0, 1, 2):
            f.debug_config(grid_limit=limit)
            f.reset()
            runs.append(run_device(torch_cuda, f, raw, [n])[0])
    check(oracle, runs[0], reference(M, T, D, False, n), "grid M=%d T=%d D=%d" % (M, T, D))
    assert runs[0].shape == (frames, M)
    assert np.array_equal(runs[0].view(np.uint32), runs[1].view(np.uint32)) and np.array_equal(runs[0].view(np.uint32), runs[2].view(np.uint32))


@pytest.mark.gpu
@pytest.mark.parametrize("start", [(1 << 32) - 5, (1 << 40) + 12345])
@pytest.mark.parametrize("M,T,D", [(256, 2047, 255), (64, 187, 17)])
def test_stream_positions_past_2_32(gpu_ok, fir, oracle, torch_cuda, M, T, D, start):
    """through the development hook the context starts at an absolute index that is a multiple of neither D nor M, with a zero
    history: the frame count is the reference's and the outputs are the reference evaluated at that position; a cut (across
    2^32 for the first start) gives the same bits, and position 0 gives other values"""
    assert start % D and start % M
    n = 30 * D + 3
    for i16 in (False, True):
        raw, _ = signal(oracle, n, i16)
        with fir.IfFirPfb(row_edge_taps(T, M, False), M, D, max_samples=n, dev=True) as f:
            if i16:
                f.set_input_format(fir.INPUT_I16)
            f.debug_config(position=start)
            assert f.frame_count(n) == pfb_ref.frame_count(start, n, D)
            one, _ = run_device(torch_cuda, f, raw, [n], first=start)
            check(oracle, one, reference(M, T, D, i16, n, start), "position M=%d D=%d start=%d i16=%d" % (M, D, start, i16))
            f.debug_config(position=start)
            y, _ = run_device(torch_cuda, f, raw, [3, 4, 1, n - 8], first=start)
            assert np.array_equal(y.view(np.uint32), one.view(np.uint32))
            f.reset()
            zero, _ = run_device(torch_cuda, f, raw, [n])
            assert zero.shape != one.shape or not np.array_equal(zero, one)


@pytest.mark.gpu
@pytest.mark.filterwarnings("ignore:The CUDA Graph is empty")
def test_refusals_leave_the_stream_where_it_was(gpu_ok, fir, oracle, torch_cuda):
    torch = torch_cuda
    M, T, D, n = 256, 700, 100, 10_000
    raw, _ = signal(oracle, n, False)
    taps = row_edge_taps(T, M, False)
    for kw in (dict(channels=96), dict(channels=32), dict(channels=8192), dict(channels=0), dict(taps=np.ones(16 * M + 1, dtype=np.float32)),
               dict(taps=np.zeros(0, dtype=np.float32)), dict(hop=0), dict(hop=M + 1), dict(first_bin=-M // 2 - 1), dict(first_bin=M),
               dict(bins=0), dict(bins=M + 1)):
        args = dict(taps=taps, channels=M, hop=D)
        args.update(kw)
        with pytest.raises(fir.IfFirError) as e:
            fir.IfFirPfb(**args)
        assert "if_fir_pfb_init" in str(e.value), kw
    with fir.IfFirPfb(taps, M, D, max_samples=n) as f:
        whole = f.process(raw)
        f.reset()
        head = f.process(raw[:2 * 1001])
        with pytest.raises(fir.IfFirError, match="ullMaxSamples"):
            f.process(np.zeros(2 * (n + 1), dtype=np.float32))
        with pytest.raises(fir.IfFirError, match="format"):
            f.set_input_format(5)
        buf = torch.zeros(2 * n + 8, dtype=torch.float32, device="cuda")
        out = torch.zeros(2 * M * (n // D + 1), dtype=torch.float32, device="cuda")
        with pytest.raises(fir.IfFirError, match="aligned"):
            f.process_device(buf.data_ptr() + 4, out.data_ptr(), 100)
        with pytest.raises(fir.IfFirError, match="aligned"):
            f.process_device(buf.data_ptr(), out.data_ptr() + 4, 100)
        with pytest.raises(fir.IfFirError, match="NULL"):
            f.process_device(0, out.data_ptr(), 100)
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
        tail = f.process(raw[2 * 1001:])
        assert np.array_equal(np.concatenate([head, tail]).view(np.uint32), whole.view(np.uint32))
    # a call that would carry the position past 2^64 is refused; the stream goes on and ends as an undisturbed one
    start = (1 << 64) - 1000
    with fir.IfFirPfb(taps, M, D, max_samples=n, dev=True) as f, fir.IfFirPfb(taps, M, D, max_samples=n, dev=True) as calm:
        for c in (f, calm):
            c.debug_config(position=start)
        a = f.process(raw[:2 * 600])
        with pytest.raises(fir.IfFirError, match="2\\^64"):
            f.process(raw[:2 * 401])
        assert f.frame_count(401) == 0
        b = f.process(raw[2 * 600:2 * 999])   # (to 2^64 - 1: a position of 2^64 itself has no representation)
        want = calm.process(raw[:2 * 999])
        assert want.shape[0] == pfb_ref.frame_count(start, 999, D) > 0
        assert np.array_equal(np.concatenate([a, b]).view(np.uint32), want.view(np.uint32))
