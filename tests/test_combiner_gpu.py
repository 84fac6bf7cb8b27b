"""The channel combiner (if_fir_combiner_t, docs/SPEC.md §9) on the GPU against the float64 definition (tests/combiner_ref.py)
at SPEC §3's tolerance: both routes over the matrix of combiner_ref.cases() -- taps loud at both ends, a distinct signal per
channel, centres off the grid, streams of three blocks and a ragged one walked by two workgroups --, streaming, set_centres,
reset, output indices past 2^32, the chain of interpolators it replaces, and the refusals."""
import numpy as np
import pytest

import combiner_ref as cr
import matrix_util

TOL = matrix_util.TOL
ROUTES = ("fft", "generic")


@pytest.fixture(scope="module")
def torch_cuda(gpu_ok):
    import torch
    torch.cuda.set_device(0)
    return torch


def make(fir, taps, L, centres, ct, route, n):
    f = fir.IfFirCombiner(taps, L, centres, max_samples=n, complex_taps=ct, dev=True)
    if route == "generic":
        f.set_backend(fir.BACKEND_HIP_GENERIC)
    else:
        assert f.get_backend() == fir.BACKEND_HIP_FFT
    f.debug_config(grid_limit=2)   # one workgroup walks several blocks
    return f


def cut(arrs, a, b):
    return [x[2 * a:2 * b] for x in arrs]


def matrix():
    return [(route,) + c for route in ROUTES for c in cr.cases(route)]


@pytest.mark.gpu
@pytest.mark.parametrize("route,L,C,T,ct,i16", matrix())
def test_combiner_matches_float64_reference(gpu_ok, fir, oracle, route, L, C, T, ct, i16):
    taps, raw, _, centres, words, ref = cr.case_reference(L, C, T, ct, i16)
    n = raw[0].size // 2
    with make(fir, taps, L, centres, ct, route, n) as f:
        if i16:
            f.set_input_format(fir.INPUT_I16)
        assert [cr.phase_word(v) for v in f.get_centres()] == words
        assert f.out_count(n) == n * L
        y = f.process(raw)
    assert y.size == 2 * n * L
    matrix_util.check(oracle, y, ref, "%s rows=%d i16=%d L=%d C=%d T=%d ct=%d" % (route, cr.overlap_rows(T), i16, L, C, T, ct),
                      tag="combiner-matrix")


STREAM_SHAPES = [("fft", 8, 8, 255, False), ("fft", 64, 3, 31, True), ("fft", 4, 2, 3073, False), ("fft", 16, 16, 1023, True),
                 ("generic", 3, 2, 255, True), ("generic", 16, 3, 1023, False),
                 ("fft", 32, 3, 513, True), ("fft", 8, 2, 2049, False)]   # rows 8 and 32 (and L = 32)


@pytest.mark.gpu
@pytest.mark.parametrize("route,L,C,T,ct", STREAM_SHAPES)
def test_streaming_pieces(gpu_ok, fir, oracle, route, L, C, T, ct):
    """process(a || b) == process(a); process(b) within the tolerance: the stream cut in three; pieces shorter than the history
    with a call of 0 samples and calls of 1 sample among them; a change from float32 to int16 in mid-stream.  Every piece is
    held to its part of the whole stream's reference."""
    taps = matrix_util.edge_taps(T, L, ct)
    n = cr.stream_samples(T, L)
    centres = cr.centres_for(L, C)
    words = [cr.phase_word(v) for v in centres]
    raw_f, xs_f = cr.signals(oracle, n, C, False)
    raw_i, xs_i = cr.signals(oracle, n, C, True)
    hist = -(-64 * cr.overlap_rows(T) // L)
    ref_f = cr.reference(taps, xs_f, L, words, ct)
    change = n // 2 + 3
    ref_mixed = cr.reference(taps, [np.concatenate([a[:2 * change], b[2 * change:]]) for a, b in zip(xs_f, xs_i)], L, words, ct)
    small = [1, 0, max(1, hist - 1), 1, max(1, hist // 2), 0, 1, 3]
    plans = (("three", [n // 3, n // 3 + 1], None, ref_f), ("short", small, None, ref_f), ("format", [change], 1, ref_mixed))
    with make(fir, taps, L, centres, ct, route, n) as f:
        for name, sizes, to_i16_at, ref in plans:
            f.reset()
            f.set_input_format(fir.INPUT_F32)
            pos = 0
            for k, s in enumerate(sizes + [n - sum(sizes)]):
                if to_i16_at == k:
                    f.set_input_format(fir.INPUT_I16)
                src = raw_i if (to_i16_at is not None and k >= to_i16_at) else raw_f
                y = f.process(cut(src, pos, pos + s))
                assert y.size == 2 * s * L
                if s:
                    matrix_util.check(oracle, y, ref[2 * pos * L:2 * (pos + s) * L], "%s %s piece %d (%d samples) L=%d C=%d T=%d"
                                      % (route, name, k, s, L, C, T), tag="combiner-stream")
                pos += s
            assert pos == n


@pytest.mark.gpu
@pytest.mark.parametrize("route,L,C,T,ct", [("fft", 8, 8, 255, True), ("generic", 5, 3, 31, False)])
def test_set_centres_between_calls(gpu_ok, fir, oracle, route, L, C, T, ct):
    """new centres hold from the next call as if set since the last reset: the second call against the reference of the new
    centres from n = 0 on"""
    taps = matrix_util.edge_taps(T, L, ct)
    n = cr.stream_samples(T, L)
    raw, xs = cr.signals(oracle, n, C, False)
    first, second = cr.centres_for(L, C), (cr.centres_for(L, C)[::-1] * 0.83 + 0.01)
    second[0] = 64.0 / 4096       # one channel moves onto the grid
    a = n // 2 + 1
    with make(fir, taps, L, first, ct, route, n) as f:
        y0 = f.process(cut(xs, 0, a))
        f.set_centres(second)
        assert [cr.phase_word(v) for v in f.get_centres()] == [cr.phase_word(v) for v in second]
        y1 = f.process(cut(raw, a, n))
        with pytest.raises(fir.IfFirError, match="0.5"):
            f.set_centres(np.where(np.arange(C) == C - 1, 0.51, second))
        assert np.array_equal(f.get_centres(), [((cr.phase_word(v) + (1 << 31)) % (1 << 32) - (1 << 31)) / 2.0 ** 32 for v in second])
    matrix_util.check(oracle, y0, cr.reference(taps, xs, L, [cr.phase_word(v) for v in first], ct)[:2 * a * L],
                      "%s before set_centres" % route, tag="combiner-centres")
    matrix_util.check(oracle, y1, cr.reference(taps, xs, L, [cr.phase_word(v) for v in second], ct)[2 * a * L:],
                      "%s after set_centres" % route, tag="combiner-centres")


@pytest.mark.gpu
@pytest.mark.parametrize("route,L", [("fft", 16), ("generic", 3)])
def test_reset_returns_to_the_start(gpu_ok, fir, oracle, route, L):
    C, T = 3, 255
    taps, raw, _, centres, _, ref = cr.case_reference(L, C, T, False, False)
    n = raw[0].size // 2
    with make(fir, taps, L, centres, False, route, n) as f:
        y0 = f.process(raw)
        f.process(cut(raw, 0, 100))
        f.reset()
        assert np.array_equal(f.process(raw), y0)
    matrix_util.check(oracle, y0, ref, "%s reset" % route, tag="combiner-reset")


@pytest.mark.gpu
@pytest.mark.parametrize("route,L,C,T,ct", [("fft", 16, 3, 255, False), ("fft", 4, 2, 1023, True), ("generic", 5, 2, 31, True)])
@pytest.mark.parametrize("where", ["across", "past"])
def test_output_indices_past_2_32(gpu_ok, fir, oracle, route, L, C, T, ct, where):
    """the rotations are indexed by the absolute output index mod 2^32: after the development seek hook the first output index
    lies just before 2^32 (the call crosses it) or past it; zero history"""
    taps = matrix_util.edge_taps(T, L, ct)
    n = cr.stream_samples(T, L)
    raw, xs = cr.signals(oracle, n, C, False)
    centres = cr.centres_for(L, C)
    words = [cr.phase_word(v) for v in centres]
    first_in = (1 << 32) // L - n // 2 if where == "across" else (1 << 32) // L + 12345
    with make(fir, taps, L, centres, ct, route, n) as f:
        f.debug_seek(first_in)
        y = f.process(raw)
    assert where == "across" or first_in * L > 1 << 32
    matrix_util.check(oracle, y, cr.reference(taps, xs, L, words, ct, first_out=first_in * L), "%s %s 2^32 L=%d" % (route, where, L),
                      tag="combiner-2^32")


@pytest.mark.gpu
@pytest.mark.parametrize("L,C,T,ct", [(8, 8, 255, False), (16, 3, 1023, True)])
def test_same_as_the_chain_of_interpolators(gpu_ok, fir, oracle, L, C, T, ct):
    """the float64 sum of C if_fir_interp_t outputs with set_nco(f_c): each side is within 1e-6 of the same float64 values, so
    they differ by at most 2e-6 of the peak"""
    taps, raw, _, centres, _, ref = cr.case_reference(L, C, T, ct, False)
    n = raw[0].size // 2
    with make(fir, taps, L, centres, ct, "fft", n) as f:
        y = f.process(raw)
    chain = np.zeros(2 * n * L, dtype=np.float64)
    for x, fc in zip(raw, centres):
        with fir.IfFirInterp(taps, L, max_samples=n, complex_taps=ct) as g:
            g.set_nco(fc)
            chain += g.process(x)
    diff = np.max(np.abs(cr.as_c(y) - cr.as_c(chain))) / np.max(np.abs(cr.as_c(chain)))
    print("combiner-chain L=%d C=%d T=%d max difference %.3g of the peak" % (L, C, T, diff))
    assert diff <= 2e-6, diff
    matrix_util.check(oracle, y, ref, "chain shape L=%d C=%d" % (L, C), tag="combiner-chain")


@pytest.mark.gpu
def test_device_pointers_and_canaries(gpu_ok, fir, oracle, torch_cuda):
    torch = torch_cuda
    L, C, T, pad = 8, 3, 1023, 4096
    taps, raw, _, centres, _, ref = cr.case_reference(L, C, T, False, False)
    n = raw[0].size // 2
    with fir.IfFirCombiner(taps, L, centres, max_samples=n, dev=True) as f:
        for route in ROUTES:
            f.reset()
            f.set_backend(fir.BACKEND_HIP_GENERIC if route == "generic" else fir.BACKEND_AUTO)
            dins = [torch.from_numpy(x).cuda() for x in raw]
            buf = torch.full((2 * (n * L + 2 * pad),), 12345.0, dtype=torch.float32, device="cuda")
            m = f.process_device([d.data_ptr() for d in dins], buf.data_ptr() + 8 * pad, n)
            f.synchronize()
            assert m == n * L
            h = buf.cpu().numpy()
            assert np.all(h[:2 * pad] == 12345.0) and np.all(h[-2 * pad:] == 12345.0), route
            matrix_util.check(oracle, h[2 * pad:-2 * pad], ref, "%s device pointers" % route, tag="combiner-device")
        f.set_backend(fir.BACKEND_AUTO)
        with pytest.raises(fir.IfFirError, match="aligned"):
            f.process_device([dins[0].data_ptr(), dins[1].data_ptr() + 4, dins[2].data_ptr()], buf.data_ptr(), 100)
        with pytest.raises(fir.IfFirError, match="aligned"):
            f.process_device([d.data_ptr() for d in dins], buf.data_ptr() + 4, 100)
        with pytest.raises(fir.IfFirError, match="NULL"):
            f.process_device([dins[0].data_ptr(), 0, dins[2].data_ptr()], buf.data_ptr(), 100)


@pytest.mark.gpu
def test_refusals_leave_the_context_usable(gpu_ok, fir, oracle):
    L, C, T = 4, 2, 255
    taps, raw, _, centres, _, ref = cr.case_reference(L, C, T, False, False)
    n = raw[0].size // 2
    for bad_centres in (np.zeros(0), np.zeros(65)):
        with pytest.raises(fir.IfFirError, match="channels"):
            fir.IfFirCombiner(taps, L, bad_centres)
    for f_bad in (0.5001, -0.7, float("nan")):
        with pytest.raises(fir.IfFirError, match="0.5"):
            fir.IfFirCombiner(taps, L, [0.1, f_bad])
    for t, l in ((0, 4), (4097, 4), (31, 0), (31, 65)):
        with pytest.raises(fir.IfFirError):
            fir.IfFirCombiner(np.ones(t, dtype=np.float32), l, [0.1])
    with fir.IfFirCombiner(taps, L, centres, max_samples=n) as f:
        y0 = f.process(raw)
        f.reset()
        f.process(cut(raw, 0, 50))
        for bad, what in ((lambda: f.set_backend(fir.BACKEND_HIP_DIRECT), "does not combine"),
                          (lambda: f.set_backend(fir.BACKEND_HIP_TAPSPLIT), "does not combine"), (lambda: f.set_backend(9), "does not combine"),
                          (lambda: f.set_centres([0.1, 0.6]), "0.5"), (lambda: f.set_input_format(5), "format"),
                          (lambda: f.process([np.zeros(2 * (n + 1), dtype=np.float32)] * C), "exceed")):
            with pytest.raises(fir.IfFirError, match=what):
                bad()
        # nothing of the above moved the stream or the centres: the call after them continues at sample 50
        matrix_util.check(oracle, f.process(cut(raw, 50, n)), ref[2 * 50 * L:], "after the refusals", tag="combiner-refusals")
        f.reset()
        assert np.array_equal(f.process(raw), y0)
    matrix_util.check(oracle, y0, ref, "refusals", tag="combiner-refusals")
    with fir.IfFirCombiner(matrix_util.edge_taps(31, 3, False), 3, [0.1, -0.2], max_samples=10) as f:
        assert f.get_backend() == fir.BACKEND_HIP_GENERIC
        with pytest.raises(fir.IfFirError, match="overlap-save"):
            f.set_backend(fir.BACKEND_HIP_FFT)
        assert f.get_backend() == fir.BACKEND_HIP_GENERIC
        assert f.process([np.zeros(20, dtype=np.float32)] * 2).size == 2 * 10 * 3
    for L2, T2, want in ((4, 255, fir.BACKEND_HIP_FFT), (64, 3073, fir.BACKEND_HIP_FFT), (2, 255, fir.BACKEND_HIP_GENERIC),
                         (4, 3074, fir.BACKEND_HIP_GENERIC), (12, 31, fir.BACKEND_HIP_GENERIC)):
        with fir.IfFirCombiner(np.ones(T2, dtype=np.float32), L2, [0.0], max_samples=16) as f:
            assert f.get_backend() == want, (L2, T2)


@pytest.mark.gpu
@pytest.mark.parametrize("route", ROUTES)
def test_stream_capture_is_refused(gpu_ok, fir, oracle, torch_cuda, route):
    """a call carries host-side streaming state (sample index, history ping-pong): a capturing stream is refused with a message,
    nothing is launched, and the context goes on afterwards (as the interpolator's test of the same name)"""
    torch = torch_cuda
    L, C, T = 4, 2, 255
    taps, raw, _, centres, _, ref = cr.case_reference(L, C, T, False, False)
    n = raw[0].size // 2
    a = n // 4 * 2   # even: the second call's pointers keep the generic backend's 16-byte alignment
    dins = [torch.from_numpy(x).cuda() for x in raw]
    with make(fir, taps, L, centres, False, route, n) as f:
        out = torch.empty(2 * n * L, dtype=torch.float32, device="cuda")
        s = torch.cuda.Stream()
        f.set_stream(s.cuda_stream)
        f.process_device([d.data_ptr() for d in dins], out.data_ptr(), a)
        f.synchronize()
        rest = [d.data_ptr() + 8 * a for d in dins]
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(s):
            g.capture_begin()
            try:
                with pytest.raises(fir.IfFirError, match="captured"):
                    f.process_device(rest, out.data_ptr() + 8 * a * L, n - a)
            finally:
                g.capture_end()
        # the refused call consumed nothing: the stream goes on where it was
        f.process_device(rest, out.data_ptr() + 8 * a * L, n - a)
        f.synchronize()
        y = out.cpu().numpy()
    matrix_util.check(oracle, y, ref, "%s capture refused" % route, tag="combiner-capture")
