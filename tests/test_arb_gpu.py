"""The arbitrary-ratio resampler (if_fir_arb_t, docs/SPEC.md §12) on the GPU against the float64 reference of tests/arb_ref.py,
SPEC §3 tolerance; stream cuts, grid limits, format changes, an unchanged retune and the stream position bit for bit.  Device
output buffers carry a sentinel guard behind their last sample, and the guard is checked.  Every case is a few thousand samples."""
import functools

import numpy as np
import pytest

import arb_ref
import matrix_util
import resamp_ref
from matrix_util import TOL, row_edge_taps

GUARD = 64          # float32 words behind the last output
SENTINEL = 12345.0
# (b, T, R): just below 1 (the rational resampler's 64/63 plus one unit), just below and above 1, K = 512, above 3 with the
# most phases, the smallest ratio with a last row of one tap, the largest ratio, two thirds and three halves off the phase
# grid, T < P (phases without a tap), a short filter, a single tap
MATRIX = ((6, 1537, 63 * 2 ** 26 + 1), (6, 1537, 2 ** 32 - 12345), (4, 8192, 2 ** 32 + 999), (10, 8192, 3 * 2 ** 32 + 1234567),
          (7, 2049, 2 ** 26 + 1), (5, 1000, 2 ** 34 - 1), (8, 4096, 2863311531), (4, 4096, 6442450941), (6, 6, 2 ** 32 + 77),
          (5, 33, 1234567891), (4, 1, 2 ** 32))
# the highest segment and the remainder after the unroll by 8: K = 2, 7, 8, 9, 15, 16, 17, 33 phase taps give a highest segment
# of 2, 7, 8, 9, 15, 16, 1, 1 taps and remainders of 2, 7, 0, 1, 7, 0, 1, 1; the last 5 rows end one tap early
REMAINDERS = tuple((4, 16 * K - 5, 2 ** 32 + 999) for K in (2, 7, 8, 9, 15, 16, 17, 33))


@pytest.fixture(scope="module")
def torch_cuda(gpu_ok):
    import torch
    torch.cuda.set_device(0)
    return torch


def taps_for(T, b, R):
    """windowed-sinc low-pass (Blackman) of gain P = 2^b designed at P times the input rate, cut-off 0.45 / max(1, rho) of the
    input rate; any T (if_bpf_design stops at 4096 taps and makes odd lengths only); T = 1 is the single tap P"""
    P = 1 << b
    cut = 0.45 / (P * max(1.0, R / 2.0 ** 32))
    k = np.arange(T) - (T - 1) / 2.0
    h = 2.0 * cut * np.sinc(2.0 * cut * k) * np.blackman(T)
    return (h * (P / np.sum(h))).astype(np.float32)


def signal(n, i16):
    """matrix_util.signal: (what the context is fed, the same samples as float32); int16 with full-scale samples"""
    import __graft_entry__ as g
    return matrix_util.signal(g.load_oracle(), n, i16)


def make_taps(T, b, R, loud):
    return row_edge_taps(T, 1 << b, False) if loud else taps_for(T, b, R)


@functools.lru_cache(maxsize=None)
def reference(b, T, R, loud, i16, n):
    """(float64 outputs, read-only; count) of the stream of n samples in one call at a fixed step"""
    ref, counts = arb_ref.resample_f64(make_taps(T, b, R, loud), signal(n, i16)[1], b, R)
    ref.setflags(write=False)
    return ref, counts[0]


def run_device(torch, f, raw, pieces, formats=None, steps=None, position=0, time_offset=0):
    """feed `raw` from ONE device buffer in consecutive pieces (sample-aligned offsets); returns (outputs, counts).  With
    `formats` (one input format per piece, set before that piece) `raw` maps each format to the stream in that format; with
    `steps` the step of every piece is set before it.  Every count is held to if_fir_arb_out_count and to arb_ref.out_count
    at (position, position 2^32 + time_offset), where the context must have been put."""
    both = {None: raw} if formats is None else raw
    n = next(iter(both.values())).size // 2
    assert all(v.size == 2 * n for v in both.values()) and sum(pieces) == n
    din = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in both.items()}
    c, tau = position, (position << 32) + time_offset
    wants = []
    for k, s in enumerate(pieces):
        step = f.step if steps is None else steps[k]
        wants.append(arb_ref.out_count(c, tau, s, step))
        c, tau = c + s, tau + wants[-1] * step
    total = sum(wants)
    buf = torch.full((2 * total + GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
    # the context's stream is non-blocking: it does not wait for the fill above, which torch queued on its own stream
    torch.cuda.synchronize()
    pos = done = 0
    for k, s in enumerate(pieces):
        if formats is not None:
            f.set_input_format(formats[k])
        if steps is not None:
            f.set_step(steps[k])
        src = din[None if formats is None else formats[k]]
        in_bytes = 2 * src.element_size()
        want = f.out_count(s)
        got = f.process_device(src.data_ptr() + in_bytes * pos, buf.data_ptr() + 8 * done, s)
        assert got == want == wants[k], (k, pos, s, got, want, wants[k])
        pos += s
        done += got
    f.synchronize()
    assert pos == n and done == total
    h = buf.cpu().numpy()
    assert np.all(h[2 * total:] == SENTINEL), "the guard behind the last output was written"
    return h[:2 * total], wants


def same_bits(y, want, what=""):
    """the two outputs are the same bits; where they are not, how many samples differ, the first of them, and whether the
    buffer's sentinel shows through"""
    if not np.array_equal(y, want):
        bad = np.flatnonzero(y != want) if y.size == want.size else np.zeros(0, dtype=np.int64)
        first = (int(bad[0]), float(y[bad[0]]), float(want[bad[0]])) if bad.size else None
        raise AssertionError("%s: sizes %d / %d, %d floats differ, first (index, got, want) %s, last index %s, sentinels %d"
                             % (what, y.size, want.size, bad.size, first, int(bad[-1]) if bad.size else None, int(np.sum(y == SENTINEL))))


def cases():
    return [pytest.param(b, T, R, loud, i16, id="b%d-T%d-R%d-%s-%s" % (b, T, R, "loud" if loud else "lowpass", "i16" if i16 else "f32"))
            for (b, T, R) in MATRIX + REMAINDERS for loud in (False, True) for i16 in (False, True)]


@pytest.mark.gpu
@pytest.mark.parametrize("b,T,R,loud,i16", cases())
def test_matrix_against_float64(gpu_ok, fir, oracle, torch_cuda, b, T, R, loud, i16):
    """designed low-pass taps, and taps whose first and highest tap of every phase row are the largest of the filter
    (tests/test_arb_host.py: dropping one of them costs more than 1e-2), on the shortest stream with three whole tiles and a
    ragged one.  Host and device path, one cut inside a tile."""
    K, tile_out, _ = arb_ref.tile_shape(T, b, R)
    n = arb_ref.stream_len(T, b, R)
    raw, _ = signal(n, i16)
    ref, outs = reference(b, T, R, loud, i16, n)
    assert outs > 3 * tile_out and outs % tile_out and n >= 2 * K + 17
    cut = n // 3 + 1
    with fir.IfFirArb(make_taps(T, b, R, loud), b, R, max_samples=n, dev=True) as f:
        assert f.tile_outputs() == tile_out and f.step == R
        if i16:
            f.set_input_format(fir.INPUT_I16)
        y = np.concatenate([f.process(raw[:2 * cut]), f.process(raw[2 * cut:])])
        f.reset()
        yd, _ = run_device(torch_cuda, f, raw, [cut, n - cut])
    assert y.size == ref.size == 2 * outs
    l2, mx = oracle.err_metrics(y, ref)
    print("arb b=%d T=%d R=%d loud=%d i16=%d: l2=%.3g max=%.3g" % (b, T, R, loud, i16, l2, mx))
    assert l2 <= TOL and mx <= TOL, (l2, mx)
    assert np.array_equal(yd, y)


@pytest.mark.gpu
@pytest.mark.parametrize("b,T,R,i16", [(6, 1537, 63 * 2 ** 26 + 1, False), (6, 1537, 2 ** 32 - 12345, True), (4, 27, 2 ** 32 + 999, False),
                                       (10, 8192, 3 * 2 ** 32 + 1234567, True), (5, 1000, 2 ** 34 - 1, False)])
def test_order_of_the_spec_bit_for_bit(gpu_ok, fir, b, T, R, i16):
    """the kernel's float32 output equals the float32 model of SPEC §12's order (arb_ref.resample_f32_order): the order that is
    written down is the order that runs"""
    n = arb_ref.stream_len(T, b, R)
    raw, x = signal(n, i16)
    taps = row_edge_taps(T, 1 << b, False)
    with fir.IfFirArb(taps, b, R, max_samples=n) as f:
        if i16:
            f.set_input_format(fir.INPUT_I16)
        y = f.process(raw)
    assert np.array_equal(y, arb_ref.resample_f32_order(taps, x, b, R))


# (b, T, R) of the bit-for-bit tests: below 1 with K = 25, the largest ratio (an output every fourth input: calls of one sample
# mostly emit nothing), the smallest ratio, K = 512
CUT_SHAPES = ((6, 1537, 63 * 2 ** 26 + 1), (4, 255, 2 ** 34), (7, 2049, 2 ** 26 + 1), (4, 8192, 2 ** 32 + 999))


@pytest.mark.gpu
@pytest.mark.parametrize("i16", [False, True])
@pytest.mark.parametrize("b,T,R", CUT_SHAPES)
def test_cuts_grid_limits_formats_and_an_unchanged_retune_bit_for_bit(gpu_ok, fir, oracle, torch_cuda, b, T, R, i16):
    """against the one-call, full-grid result, which meets float64: pieces of 1, 2, 0, K - 1 and 4097 samples, then five of
    one sample (at rho = 4 three of every four of them emit nothing), then the rest; the grid capped at 1 and at 3
    workgroups; the input format switched between the pieces; set_step with the value in force between the pieces"""
    K = arb_ref.tile_shape(T, b, R)[0]
    head = [1, 2, 0, K - 1, 4097] + 5 * [1]
    n = sum(head) + max(arb_ref.stream_len(T, b, R), 300)
    pieces = head + [n - sum(head)]
    raw, x = signal(n, i16)
    xi, xf = signal(n, True)
    taps = row_edge_taps(T, 1 << b, False)
    ref, counts = arb_ref.resample_f64(taps, x, b, R)
    with fir.IfFirArb(taps, b, R, max_samples=n, dev=True) as f:
        if i16:
            f.set_input_format(fir.INPUT_I16)
        one, _ = run_device(torch_cuda, f, raw, [n])
        l2, mx = oracle.err_metrics(one, ref)
        assert one.size == 2 * counts[0] and l2 <= TOL and mx <= TOL, (l2, mx)
        f.reset()
        y, got = run_device(torch_cuda, f, raw, pieces)
        assert got[2] == 0
        same_bits(y, one, "pieces")
        if R == 2 ** 34:
            assert sorted(got[5:10]).count(0) >= 3      # calls with input and without output
        for limit in (1, 3):
            f.debug_config(grid_limit=limit)
            f.reset()
            y, _ = run_device(torch_cuda, f, raw, [n])
            same_bits(y, one, "one call, grid limit %d" % limit)
            f.reset()
            y, _ = run_device(torch_cuda, f, raw, pieces)
            same_bits(y, one, "pieces, grid limit %d" % limit)
        f.debug_config(grid_limit=0)
        f.reset()
        y, _ = run_device(torch_cuda, f, raw, pieces, steps=[R] * len(pieces))
        same_bits(y, one, "set_step unchanged")
        # the same values as int16 throughout, then float32 and int16 in turn
        f.reset()
        f.set_input_format(fir.INPUT_I16)
        one16, _ = run_device(torch_cuda, f, xi, [n])
        if i16:
            same_bits(one16, one, "int16 again")
        f.reset()
        formats = [fir.INPUT_F32 if k % 2 == 0 else fir.INPUT_I16 for k in range(len(pieces))]
        y, _ = run_device(torch_cuda, f, {fir.INPUT_F32: xf, fir.INPUT_I16: xi}, pieces, formats=formats)
        same_bits(y, one16, "formats in turn")


@pytest.mark.gpu
@pytest.mark.parametrize("b,T,R,offset", [(6, 1537, 63 * 2 ** 26 + 1, 0), (6, 1537, 63 * 2 ** 26 + 1, 2 ** 32 - 1), (5, 1000, 2 ** 34 - 1, 2 ** 34 - 2),
                                          (7, 2049, 2 ** 26 + 1, 123456789)])
def test_position_alone_changes_no_bit(gpu_ok, fir, torch_cuda, b, T, R, offset):
    """the same call placed at the positions 0, 2^32 - 5 and 2^40 + 12345 with the same time offset: the counts are those of
    Python-integer arithmetic at each position and the outputs are the same bits"""
    n = arb_ref.stream_len(T, b, R)
    raw, _ = signal(n, False)
    cut = n // 2 + 3
    runs = []
    with fir.IfFirArb(row_edge_taps(T, 1 << b, False), b, R, max_samples=n, dev=True) as f:
        for position in (0, 2 ** 32 - 5, 2 ** 40 + 12345):
            f.reset()
            f.debug_config(position=position, time_offset=offset)
            y, counts = run_device(torch_cuda, f, raw, [cut, n - cut], position=position, time_offset=offset)
            runs.append((y, counts))
    assert sum(runs[0][1]) > 3 * arb_ref.TILE_OUT
    for y, counts in runs[1:]:
        assert counts == runs[0][1]
        same_bits(y, runs[0][0], "another position")


@pytest.mark.gpu
@pytest.mark.parametrize("i16", [False, True])
@pytest.mark.parametrize("b,T,R1,R2", [(6, 1537, 63 * 2 ** 26 + 1, 63 * 2 ** 26 + 12885), (8, 4096, 2863311531, 3 * 2 ** 32 + 5),
                                       (5, 1000, 2 ** 34 - 1, 2 ** 26)])
def test_retune_between_calls(gpu_ok, fir, oracle, torch_cuda, b, T, R1, R2, i16):
    """three pieces at R1, R2, R1: within SPEC §3 of the float64 reference run with the same piecewise steps; the count of
    every piece equals out_count (run_device holds each to the library's and to Python-integer arithmetic)"""
    n1 = arb_ref.stream_len(T, b, R1) // 2 + 1
    n2 = max(arb_ref.stream_len(T, b, R2) // 2, 100)
    pieces, steps = [n1, n2, n1 + 7], [R1, R2, R1]
    n = sum(pieces)
    raw, x = signal(n, i16)
    taps = row_edge_taps(T, 1 << b, False)
    ref, counts = arb_ref.resample_f64(taps, x, b, list(zip(pieces, steps)))
    with fir.IfFirArb(taps, b, R1, max_samples=n) as f:
        if i16:
            f.set_input_format(fir.INPUT_I16)
        y, got = run_device(torch_cuda, f, raw, pieces, steps=steps)
        assert got == counts and min(counts) > 0 and f.step == R1
        # the host-pointer call after a retune to a step that emits more than the step of init
        f.reset()
        parts = []
        for s, step, at in zip(pieces, steps, np.cumsum([0] + pieces[:-1])):
            f.set_step(step)
            parts.append(f.process(raw[2 * at:2 * (at + s)]))
        assert np.array_equal(np.concatenate(parts), y)
    l2, mx = oracle.err_metrics(y, ref)
    print("arb retune b=%d T=%d R1=%d R2=%d i16=%d: counts=%s l2=%.3g max=%.3g" % (b, T, R1, R2, i16, counts, l2, mx))
    assert l2 <= TOL and mx <= TOL, (l2, mx)


@pytest.mark.gpu
@pytest.mark.parametrize("P,M,T", [(64, 63, 1537), (16, 7, 255)])
def test_rational_step_against_the_rational_resampler(gpu_ok, fir, oracle, P, M, T):
    """R = M 2^32 / P puts every output on the phase grid (mu = 0): within SPEC §3 of the rational resampler's float64
    reference, and within twice that of IfFirResamp(h, P, M) on the same data"""
    b = P.bit_length() - 1
    R = M * 2 ** 32 // P
    assert R * P == M * 2 ** 32
    n = arb_ref.stream_len(T, b, R)
    x, _ = signal(n, False)
    for taps in (taps_for(T, b, R), row_edge_taps(T, P, False)):
        ref = resamp_ref.resample_f64(taps, x, P, M)
        with fir.IfFirArb(taps, b, R, max_samples=n) as f:
            y = f.process(x)
        with fir.IfFirResamp(taps, P, M, max_samples=n) as r:
            z = r.process(x)
        assert y.size == z.size == ref.size
        l2, mx = oracle.err_metrics(y, ref)
        l2r, mxr = oracle.err_metrics(y, z.astype(np.float64))
        print("arb rational P=%d M=%d T=%d: l2=%.3g max=%.3g; against IfFirResamp l2=%.3g max=%.3g" % (P, M, T, l2, mx, l2r, mxr))
        assert l2 <= TOL and mx <= TOL, (l2, mx)
        assert l2r <= 2 * TOL and mxr <= 2 * TOL, (l2r, mxr)


@pytest.mark.gpu
def test_degenerate_calls(gpu_ok, fir):
    """no input; calls smaller than one output (rho just below 4: three of four one-sample calls emit nothing)"""
    b, T, R, n = 5, 100, 2 ** 34 - 1, 700
    x, _ = signal(n, False)
    with fir.IfFirArb(taps_for(T, b, R), b, R, max_samples=n) as f:
        one = f.process(x)
        assert one.size == 2 * arb_ref.out_count(0, 0, n, R)
        f.reset()
        assert f.process(x[:0]).size == 0 and f.out_count(0) == 0
        parts = [f.process(x[2 * i:2 * i + 2]) for i in range(n)]
        assert sum(1 for p in parts if p.size == 0) == n - one.size // 2 >= n // 2
        assert np.array_equal(np.concatenate(parts), one)


@pytest.mark.gpu
@pytest.mark.filterwarnings("ignore:The CUDA Graph is empty")
def test_reset_and_rejected_arguments(gpu_ok, fir, torch_cuda):
    torch = torch_cuda
    b, T, R, n = 6, 1537, 63 * 2 ** 26 + 1, 4000
    x, _ = signal(n, False)
    taps = taps_for(T, b, R)
    with fir.IfFirArb(taps, b, R, max_samples=n) as f:
        y0 = f.process(x)
        f.process(x[:2 * 1001])
        f.reset()
        assert f.out_count(n) == y0.size // 2 and np.array_equal(f.process(x), y0)
        f.reset()
        head = f.process(x[:2 * 1001])
        assert np.array_equal(head, y0[:head.size])
        with pytest.raises(fir.IfFirError, match="ullMaxSamples"):
            f.process(np.zeros(2 * (n + 1), dtype=np.float32))
        with pytest.raises(fir.IfFirError, match="format"):
            f.set_input_format(5)
        for step in (2 ** 26 - 1, 2 ** 34 + 1, 0, 2 ** 64 - 1):
            with pytest.raises(fir.IfFirError, match="step"):
                f.set_step(step)
        assert f.step == R
        buf = torch.zeros(2 * n + 8, dtype=torch.float32, device="cuda")
        with pytest.raises(fir.IfFirError, match="aligned"):
            f.process_device(buf.data_ptr() + 4, buf.data_ptr(), 100)
        with pytest.raises(fir.IfFirError, match="aligned"):
            f.process_device(buf.data_ptr(), buf.data_ptr() + 4, 100)
        with pytest.raises(fir.IfFirError, match="NULL"):
            f.process_device(0, buf.data_ptr(), 100)
        with pytest.raises(fir.IfFirError, match="NULL"):
            f.process_device(buf.data_ptr(), 0, 100)
        with pytest.raises(fir.IfFirError, match="too large"):
            f.process_device(buf.data_ptr(), buf.data_ptr(), 2 ** 36 + 1)
        side = torch.cuda.Stream()
        f.set_stream(side.cuda_stream)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            graph.capture_begin()
            try:
                with pytest.raises(fir.IfFirError, match="captured"):
                    f.process_device(buf.data_ptr(), buf.data_ptr(), 100)
            finally:
                graph.capture_end()
        f.set_stream(0)
        # every refused call left c, tau and the history where they were
        assert f.out_count(n - 1001) == (y0.size - head.size) // 2
        assert np.array_equal(f.process(x[2 * 1001:]), y0[head.size:])
    for T, b, R in ((0, 6, 2 ** 32), (8193, 6, 2 ** 32), (31, 3, 2 ** 32), (31, 11, 2 ** 32), (31, 6, 2 ** 26 - 1), (31, 6, 2 ** 34 + 1)):
        with pytest.raises(fir.IfFirError) as e:
            fir.IfFirArb(np.ones(T, dtype=np.float32), b, R)
        assert str(e.value)
    with pytest.raises(fir.IfFirError, match="ullMaxSamples"):
        fir.IfFirArb(np.ones(31, dtype=np.float32), 6, 2 ** 32, max_samples=0)


@pytest.mark.gpu
def test_random_configurations_against_float64(gpu_ok, fir, oracle, torch_cuda):
    """24 seeded draws: b uniform in 4..10, T log-uniform in 1..8192, R log-uniform in 2^26..2^34, int16 input drawn per case,
    taps loud at both ends of every phase row, the stream of arb_ref.stream_len, 2 to 6 pieces with one of 0 samples.  Every
    draw meets float64 within SPEC §3, and its pieces give the bits of the single call."""
    rng = np.random.default_rng(20261019)
    worst = {"l2": (0.0, None), "max": (0.0, None)}
    for draw in range(24):
        b = int(rng.integers(4, 11))
        T = min(8192, max(1, int(round(np.exp(rng.uniform(0.0, np.log(8192.0)))))))
        R = min(2 ** 34, max(2 ** 26, int(round(2.0 ** rng.uniform(26.0, 34.0)))))
        i16 = bool(rng.integers(2))
        n = arb_ref.stream_len(T, b, R)
        cuts = np.sort(rng.choice(np.arange(1, n), int(rng.integers(2, 7)) - 2, replace=False))
        pieces = [int(v) for v in np.diff(np.concatenate([[0], cuts, [n]]))]
        pieces.insert(int(rng.integers(len(pieces) + 1)), 0)
        case = "draw %d: b=%d T=%d R=%d i16=%d n=%d pieces=%s" % (draw, b, T, R, i16, n, pieces)
        assert 2 <= len(pieces) <= 6 and sum(pieces) == n, case
        raw, x = signal(n, i16)
        taps = row_edge_taps(T, 1 << b, False, seed=draw)
        ref, _ = arb_ref.resample_f64(taps, x, b, R)
        with fir.IfFirArb(taps, b, R, max_samples=n) as f:
            if i16:
                f.set_input_format(fir.INPUT_I16)
            one, _ = run_device(torch_cuda, f, raw, [n])
            f.reset()
            y, _ = run_device(torch_cuda, f, raw, pieces)
        l2, mx = oracle.err_metrics(one, ref)
        for name, v in (("l2", l2), ("max", mx)):
            if v > worst[name][0]:
                worst[name] = (v, case)
        assert l2 <= TOL and mx <= TOL, (case, l2, mx)
        same_bits(y, one, case)
    for name in ("l2", "max"):
        print("arb-random worst %s=%.3g at %s" % (name, worst[name][0], worst[name][1]))
