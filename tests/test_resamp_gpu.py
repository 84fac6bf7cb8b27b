"""The rational resampler (if_fir_resamp_t, docs/SPEC.md §7) on the GPU against the float64 reference of tests/resamp_ref.py,
SPEC §3 tolerance; stream cuts, tile and grid edges bit for bit.  Device output buffers carry a sentinel guard behind their
last sample, and the guard is checked."""
import functools

import numpy as np
import pytest

import matrix_util
import resamp_ref
from matrix_util import row_edge_taps

TOL = 1e-6
GUARD = 64          # float32 words behind the last output
SENTINEL = 12345.0
# (L, M, T): ratios above and below 1, a common factor, plain decimator / interpolator / filter, long phase rows, the longest
# filter, T < L (phases without a tap), a call that emits fewer outputs than one period, a single tap
MATRIX = ((3, 2, 95), (2, 3, 63), (5, 7, 255), (4, 6, 33), (1, 4, 255), (4, 1, 255), (1, 1, 31), (64, 63, 1537), (63, 64, 1537),
          (64, 1, 4096), (4, 3, 4096), (1, 3, 1023), (7, 5, 3), (3, 64, 100), (5, 2, 1))

# the rows of test_matrix_with_loud_row_ends (taps of matrix_util.row_edge_taps, streams of resamp_ref.stream_len): MATRIX, then
LOUD_MATRIX = MATRIX + (
    # K = 4096, the longest history: the LDS fit caps the tile to 64 periods = 64 outputs, so 64 lanes of one of the four
    # places work, and the tile's window is 8191 of 8192 samples
    (1, 64, 4096),
    # capped tiles whose output count is no multiple of the lane count W: the mask of a lane's places cuts inside a place
    (2, 64, 4096), (8, 64, 1000),
    # a common factor of 4 with a capped tile; gcd = L, one phase reached
    (4, 64, 4096), (64, 64, 4096),
    # the highest segment and the remainder after the unroll by 8: K = 2, 7, 8, 9, 15, 16, 17, 33 phase taps give a highest
    # segment of 2, 7, 8, 9, 15, 16, 1, 1 taps and remainders of 2, 7, 0, 1, 7, 0, 1, 1
    (3, 2, 6), (3, 2, 21), (3, 2, 24), (3, 2, 27), (3, 2, 45), (3, 2, 48), (3, 2, 51), (3, 2, 99),
    # the last row entries of two of the three phases are padding zeros
    (3, 2, 22), (3, 2, 49))


@pytest.fixture(scope="module")
def torch_cuda(gpu_ok):
    import torch
    torch.cuda.set_device(0)
    return torch


def taps_for(fir, T, L, M, complex_taps):
    """image-rejection low-pass of gain L, cut-off 0.45 / max(L, M) (complex: the shifted design).  if_bpf_design makes odd
    lengths >= 3: an even T is the design of T - 1 taps plus a last tap of an eighth of the centre tap, negated (the last tap
    index is then met by a value that matters, not by a window's zero), T = 1 is the single tap L."""
    w = max(L, M)
    odd = T if T % 2 else T - 1
    if odd < 3:
        h = np.array([L, 0.5 * L] if complex_taps else [L], dtype=np.float32)
    elif complex_taps:
        h = (fir.bpf_design_complex(odd, 0.1 / w, 0.8 / w) * np.float32(L)).astype(np.float32)
    else:
        h = (fir.bpf_design(odd, 0.0, 0.45 / w) * np.float32(L)).astype(np.float32)
    if odd >= 3 and odd != T:
        width = 2 if complex_taps else 1
        mid = h[(odd // 2) * width:(odd // 2) * width + width]
        h = np.concatenate([h, -mid / np.float32(8)]).astype(np.float32)
    assert h.size == T * (2 if complex_taps else 1)
    return h


@functools.lru_cache(maxsize=None)
def signal(n, i16):
    """(what the context is fed, the same samples as float32)"""
    import __graft_entry__ as g
    x = g.load_oracle().synth_iq(n, channel=3)
    if i16:
        xi = np.clip(np.round(x * 14000.0), -32768, 32767).astype(np.int16)
        return xi, xi.astype(np.float32) * np.float32(2.0 ** -15)
    return x, x


@functools.lru_cache(maxsize=None)
def reference(fir, L, M, T, ct, i16, n):
    ref = resamp_ref.resample_f64(taps_for(fir, T, L, M, ct), signal(n, i16)[1], L, M, ct)
    ref.setflags(write=False)
    return ref


def loud_signal(n, i16):
    """matrix_util.signal: (what the context is fed, the same samples as float32); int16 with full-scale samples"""
    import __graft_entry__ as g
    return matrix_util.signal(g.load_oracle(), n, i16)


@functools.lru_cache(maxsize=None)
def loud_reference(L, M, T, ct, i16, n):
    ref = resamp_ref.resample_f64(row_edge_taps(T, L, ct), loud_signal(n, i16)[1], L, M, ct)
    ref.setflags(write=False)
    return ref


def cases():
    """every ratio with {real, complex} taps x {float32, int16}: each row meets all four kernel instantiations"""
    return [(L, M, T, ct, i16) for (L, M, T) in MATRIX for ct in (False, True) for i16 in (False, True)]


def run_device(torch, f, raw, pieces, i16, formats=None):
    """feed `raw` from ONE device buffer in consecutive pieces (sample-aligned offsets); returns (outputs, counts).  With
    `formats` (one input format per piece, set before that piece) `raw` maps each format to the stream in that format: the
    same values in every one, one device buffer each."""
    both = {None: raw} if formats is None else raw
    n = next(iter(both.values())).size // 2
    assert all(v.size == 2 * n for v in both.values())
    din = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in both.items()}
    total = resamp_ref.out_count(0, n, f.interpolation, f.decimation)
    buf = torch.full((2 * total + GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
    pos = done = 0
    counts = []
    for k, s in enumerate(pieces):
        if formats is not None:
            f.set_input_format(formats[k])
        src = din[None if formats is None else formats[k]]
        in_bytes = 2 * src.element_size()
        assert formats is not None or in_bytes == (4 if i16 else 8)
        want = f.out_count(s)
        got = f.process_device(src.data_ptr() + in_bytes * pos, buf.data_ptr() + 8 * done, s)
        assert got == want == resamp_ref.out_count(pos, s, f.interpolation, f.decimation), (pos, s, got, want)
        counts.append(got)
        pos += s
        done += got
    f.synchronize()
    assert pos == n and done == total
    h = buf.cpu().numpy()
    assert np.all(h[2 * total:] == SENTINEL), "the guard behind the last output was written"
    return h[:2 * total], counts


@pytest.mark.gpu
@pytest.mark.parametrize("L,M,T,ct,i16", cases())
def test_matrix_against_float64(gpu_ok, fir, oracle, torch_cuda, L, M, T, ct, i16):
    n = 60_000
    raw, _ = signal(n, i16)
    ref = reference(fir, L, M, T, ct, i16, n)
    with fir.IfFirResamp(taps_for(fir, T, L, M, ct), L, M, max_samples=n, complex_taps=ct) as f:
        if i16:
            f.set_input_format(fir.INPUT_I16)
        cut = n // 3
        y = np.concatenate([f.process(raw[:2 * cut]), f.process(raw[2 * cut:])])
        f.reset()
        yd, _ = run_device(torch_cuda, f, raw, [cut, n - cut], i16)
    assert y.size == ref.size == 2 * resamp_ref.out_count(0, n, L, M)
    l2, mx = oracle.err_metrics(y, ref)
    print("L=%d M=%d T=%d complex=%d i16=%d: l2=%.3g max=%.3g" % (L, M, T, ct, i16, l2, mx))
    assert l2 <= TOL and mx <= TOL, (l2, mx)
    assert np.array_equal(yd, y)


def loud_cases():
    return [(L, M, T, ct, i16) for (L, M, T) in LOUD_MATRIX for ct in (False, True) for i16 in (False, True)]


@pytest.mark.gpu
@pytest.mark.parametrize("L,M,T,ct,i16", loud_cases())
def test_matrix_with_loud_row_ends(gpu_ok, fir, oracle, torch_cuda, L, M, T, ct, i16):
    """every phase's first and highest tap are the largest of the filter (tests/test_resamp_host.py: dropping one of them costs
    more than 1e-2), on the shortest stream with three whole tiles and a ragged one; the int16 stream carries full-scale
    samples.  Host and device path, one cut that is a multiple of neither M (where M > 1) nor the tile's input count."""
    K, tile_out, tile_in = resamp_ref.tile_shape(T, L, M)
    n = resamp_ref.stream_len(T, L, M)
    raw, _ = loud_signal(n, i16)
    ref = loud_reference(L, M, T, ct, i16, n)
    cut = n // 3
    while cut % tile_in == 0 or (M > 1 and cut % M == 0):
        cut += 1
    assert 0 < cut < n
    with fir.IfFirResamp(row_edge_taps(T, L, ct), L, M, max_samples=n, complex_taps=ct, dev=True) as f:
        assert f.tile_outputs() == tile_out
        assert resamp_ref.out_count(0, n, L, M) > 3 * tile_out and resamp_ref.out_count(0, n, L, M) % tile_out
        if i16:
            f.set_input_format(fir.INPUT_I16)
        y = np.concatenate([f.process(raw[:2 * cut]), f.process(raw[2 * cut:])])
        f.reset()
        yd, _ = run_device(torch_cuda, f, raw, [cut, n - cut], i16)
    assert y.size == ref.size == 2 * resamp_ref.out_count(0, n, L, M)
    l2, mx = oracle.err_metrics(y, ref)
    print("loud-rows L=%d M=%d T=%d complex=%d i16=%d: l2=%.3g max=%.3g" % (L, M, T, ct, i16, l2, mx))
    assert l2 <= TOL and mx <= TOL, (l2, mx)
    assert np.array_equal(yd, y)


@pytest.mark.gpu
@pytest.mark.parametrize("ct,i16", [(False, False), (True, True)])
@pytest.mark.parametrize("L,M,T", [(3, 2, 95), (1, 3, 1023), (1, 64, 4096), (63, 64, 1537)])
def test_pieces_around_the_history_with_loud_row_ends(gpu_ok, fir, oracle, torch_cuda, L, M, T, ct, i16):
    """calls one shorter than, as long as and one longer than the K - 1 samples of history, then of 1, 0, forty times 1, M - 1
    and L samples, then the rest: in the short ones the first workgroup builds the next history from the old history and
    the call.  Bit for bit the one-call run, which meets float64.  Then the same stream as float32 and, from a cut inside
    a tile on, as int16: a change of format keeps the stream (csrc/if_fir_stream_ctx.h)."""
    K, tile_out, tile_in = resamp_ref.tile_shape(T, L, M)
    head = [K - 2, K - 1, K, 1, 0] + 40 * [1] + [M - 1, L]
    n = max(resamp_ref.stream_len(T, L, M), sum(head) + tile_in + K + 17)
    raw, _ = loud_signal(n, i16)
    xi, xf = loud_signal(n, True)
    both = {fir.INPUT_F32: xf, fir.INPUT_I16: xi}
    with fir.IfFirResamp(row_edge_taps(T, L, ct), L, M, max_samples=n, complex_taps=ct, dev=True) as f:
        assert f.tile_outputs() == tile_out
        if i16:
            f.set_input_format(fir.INPUT_I16)
        one, _ = run_device(torch_cuda, f, raw, [n], i16)
        l2, mx = oracle.err_metrics(one, loud_reference(L, M, T, ct, i16, n))
        print("loud-pieces L=%d M=%d T=%d complex=%d i16=%d: l2=%.3g max=%.3g" % (L, M, T, ct, i16, l2, mx))
        assert l2 <= TOL and mx <= TOL, (l2, mx)
        f.reset()
        y, counts = run_device(torch_cuda, f, raw, head + [n - sum(head)], i16)
        assert counts[4] == 0 and np.array_equal(y, one)
        # float32 first; int16 from inside the first tile on, in a call shorter than the history, then the rest
        if not i16:
            f.reset()
            one, _ = run_device(torch_cuda, f, xf, [n], False)
        pieces = [tile_in // 2 + 1, 0, K - 2, n - tile_in // 2 - K + 1]
        assert pieces[0] % tile_in and min(pieces) >= 0
        f.reset()
        y, _ = run_device(torch_cuda, f, both, pieces, None, formats=[fir.INPUT_F32, fir.INPUT_F32, fir.INPUT_I16, fir.INPUT_I16])
        assert np.array_equal(y, one)
        f.reset()
        f.set_input_format(fir.INPUT_I16)
        y, _ = run_device(torch_cuda, f, xi, [n], True)
        assert np.array_equal(y, one)


@pytest.mark.gpu
@pytest.mark.parametrize("L,M", [(3, 2), (2, 3), (5, 7), (63, 64)])
def test_split_invariance_bit_for_bit(gpu_ok, fir, torch_cuda, L, M):
    n, T = 20_011, 255
    x, _ = signal(n, False)
    taps = taps_for(fir, T, L, M, False)
    sizes = [1, 2, 0, M - 1, L, 4097]
    sizes.append(n - sum(sizes))
    with fir.IfFirResamp(taps, L, M, max_samples=n) as f:
        assert f.out_count(n) == resamp_ref.out_count(0, n, L, M)
        one = f.process(x)
        f.reset()
        parts, pos = [], 0
        for s in sizes:
            want = f.out_count(s)
            parts.append(f.process(x[2 * pos:2 * (pos + s)]))
            assert parts[-1].size == 2 * want
            pos += s
        assert np.array_equal(np.concatenate(parts), one)
        f.reset()
        y, counts = run_device(torch_cuda, f, x, sizes, False)
        assert sum(counts) == -(-n * L // M) and counts[2] == 0
        assert np.array_equal(y, one)


# (L, M, T, loud, complex taps, int16): the designed filters in real taps and float32; with row_edge_taps the tiles that the LDS
# fit caps (127 periods of 3/64, the 64 outputs of 1/64 with 4096 taps, 126 periods of 8/64: a grid-stride loop over such tiles
# is where tile * tile_in has to stay 64-bit), and the instantiation furthest from the first one on a full and on a capped tile
TILE_EDGES = [pytest.param(3, 2, 95, False, False, False, id="3-2-95"), pytest.param(5, 7, 255, False, False, False, id="5-7-255"),
              pytest.param(1, 3, 1023, False, False, False, id="1-3-1023"),
              pytest.param(3, 64, 100, True, False, False, id="3-64-100-loud"),
              pytest.param(1, 64, 4096, True, False, False, id="1-64-4096-loud"),
              pytest.param(8, 64, 1000, True, False, False, id="8-64-1000-loud"),
              pytest.param(3, 2, 95, True, True, True, id="3-2-95-loud-complex-i16"),
              pytest.param(3, 64, 100, True, True, True, id="3-64-100-loud-complex-i16")]


@pytest.mark.gpu
@pytest.mark.parametrize("L,M,T,loud,ct,i16", TILE_EDGES)
def test_tile_and_grid_edges(gpu_ok, fir, torch_cuda, L, M, T, loud, ct, i16):
    """output counts one less than, equal to and one more than 1 tile and 5 tiles (from a reset, L > M reaches only the counts
    ceil(n L / M): the next one up then stands in); the grid capped to 1 and to 3 workgroups gives the bits of the uncapped run"""
    taps = row_edge_taps(T, L, ct) if loud else taps_for(fir, T, L, M, ct)
    with fir.IfFirResamp(taps, L, M, max_samples=1 << 16, complex_taps=ct, dev=True) as f:
        if i16:
            f.set_input_format(fir.INPUT_I16)
        tile = f.tile_outputs()
        assert tile == resamp_ref.tile_shape(T, L, M)[1]
        assert tile > 0 and tile % L == 0
        n_for = lambda outs: (outs - 1) * M // L + 1          # the fewest inputs that emit `outs` outputs
        n_max = n_for(5 * tile + 1)
        seen = set()
        raw, x = loud_signal(n_max, i16) if loud else signal(n_max, i16)
        ref_all = resamp_ref.resample_f64(taps, x, L, M, ct)
        for want in (tile - 1, tile, tile + 1, 5 * tile - 1, 5 * tile, 5 * tile + 1):
            n = n_for(want)
            outs = resamp_ref.out_count(0, n, L, M)
            assert want <= outs < want + -(-L // M)
            seen.add(outs - want)
            runs = []
            for limit in (0, 1, 3):
                f.debug_config(grid_limit=limit)
                f.reset()
                y, _ = run_device(torch_cuda, f, raw[:2 * n], [n], i16)
                runs.append(y)
            assert np.array_equal(runs[0], runs[1]) and np.array_equal(runs[0], runs[2]), outs
            ref = ref_all[:2 * outs]
            assert np.max(np.abs(runs[0] - ref)) <= TOL * np.max(np.abs(ref)), outs
        assert 0 in seen


@pytest.mark.gpu
def test_degenerate_calls(gpu_ok, fir):
    L, M, T, n = 3, 64, 100, 700
    x, _ = signal(n, False)
    with fir.IfFirResamp(taps_for(fir, T, L, M, False), L, M, max_samples=n) as f:
        one = f.process(x)
        assert one.size == 2 * -(-n * L // M)
        f.reset()
        assert f.process(x[:0]).size == 0 and f.out_count(0) == 0
        parts = [f.process(x[2 * i:2 * i + 2]) for i in range(n)]
        assert sum(1 for p in parts if p.size == 0) == n - one.size // 2   # most calls emit nothing
        assert np.array_equal(np.concatenate(parts), one)


@pytest.mark.gpu
@pytest.mark.filterwarnings("ignore:The CUDA Graph is empty")
def test_reset_and_rejected_arguments(gpu_ok, fir, torch_cuda):
    torch = torch_cuda
    n = 10_000
    x, _ = signal(n, False)
    taps = taps_for(fir, 95, 3, 4, False)
    with fir.IfFirResamp(taps, 3, 4, max_samples=n) as f:
        y0 = f.process(x)
        f.process(x[:2 * 1001])
        f.reset()
        assert np.array_equal(f.process(x), y0)
        f.reset()
        f.process(x[:2 * 1001])
        with pytest.raises(fir.IfFirError, match="ullMaxSamples"):
            f.process(np.zeros(2 * (n + 1), dtype=np.float32))
        with pytest.raises(fir.IfFirError, match="format"):
            f.set_input_format(5)
        buf = torch.zeros(2 * n + 8, dtype=torch.float32, device="cuda")
        with pytest.raises(fir.IfFirError, match="aligned"):
            f.process_device(buf.data_ptr() + 4, buf.data_ptr(), 100)
        with pytest.raises(fir.IfFirError, match="aligned"):
            f.process_device(buf.data_ptr(), buf.data_ptr() + 4, 100)
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
        # every refused call left the stream where it was
        assert np.array_equal(f.process(x[2 * 1001:]), y0[2 * f_count(1001, 3, 4):])
    for T, L, M in ((0, 3, 2), (4097, 3, 2), (31, 0, 2), (31, 65, 2), (31, 3, 0), (31, 3, 65)):
        with pytest.raises(fir.IfFirError) as e:
            fir.IfFirResamp(np.ones(T, dtype=np.float32), L, M)
        assert str(e.value)


def f_count(n, L, M):
    return resamp_ref.out_count(0, n, L, M)


@pytest.mark.gpu
@pytest.mark.parametrize("L,M,T", [(3, 4, 95), (5, 2, 127)])
def test_against_interpolate_then_decimate(gpu_ok, fir, oracle, L, M, T):
    """what users do today: IfFirInterp(h, L), then IfFir([1.0], decimation=M) -- both within SPEC §3 of float64"""
    n = 40_000
    x, _ = signal(n, False)
    taps = taps_for(fir, T, L, M, False)
    ref = resamp_ref.resample_f64(taps, x, L, M)
    with fir.IfFirResamp(taps, L, M, max_samples=n) as f:
        y = f.process(x)
    with fir.IfFirInterp(taps, L, max_samples=n) as up, \
            fir.IfFir(np.ones(1, dtype=np.float32), decimation=M, max_samples=n * L) as down:
        chain = down.process(up.process(x))
    assert y.size == chain.size == ref.size
    for name, got in (("resampler", y), ("chain", chain)):
        l2, mx = oracle.err_metrics(got, ref)
        assert l2 <= TOL and mx <= TOL, (name, l2, mx)


@pytest.mark.gpu
def test_random_configurations_against_float64(gpu_ok, fir, oracle, torch_cuda):
    """40 seeded draws: L and M uniform in 1..64, T log-uniform in 1..4096, complex taps and int16 input drawn per case, taps
    loud at both ends of every phase row, the stream of resamp_ref.stream_len (at most 2^17 samples), 2 to 6 pieces with one
    of 0 samples.  Every draw meets float64 within SPEC §3, and its pieces give the bits of the single call."""
    rng = np.random.default_rng(20261019)
    worst = {"l2": (0.0, None), "max": (0.0, None)}
    for draw in range(40):
        L, M = (int(v) for v in rng.integers(1, 65, 2))
        T = min(4096, max(1, int(round(np.exp(rng.uniform(0.0, np.log(4096.0)))))))
        ct, i16 = bool(rng.integers(2)), bool(rng.integers(2))
        n = min(resamp_ref.stream_len(T, L, M), 1 << 17)
        cuts = np.sort(rng.choice(np.arange(1, n), int(rng.integers(2, 7)) - 2, replace=False))
        pieces = [int(v) for v in np.diff(np.concatenate([[0], cuts, [n]]))]
        pieces.insert(int(rng.integers(len(pieces) + 1)), 0)
        case = "draw %d: L=%d M=%d T=%d complex=%d i16=%d n=%d pieces=%s" % (draw, L, M, T, ct, i16, n, pieces)
        assert 2 <= len(pieces) <= 6 and sum(pieces) == n, case
        raw, x = loud_signal(n, i16)
        taps = row_edge_taps(T, L, ct, seed=draw)
        ref = resamp_ref.resample_f64(taps, x, L, M, ct)
        with fir.IfFirResamp(taps, L, M, max_samples=n, complex_taps=ct) as f:
            if i16:
                f.set_input_format(fir.INPUT_I16)
            one, _ = run_device(torch_cuda, f, raw, [n], i16)
            f.reset()
            y, _ = run_device(torch_cuda, f, raw, pieces, i16)
        l2, mx = oracle.err_metrics(one, ref)
        for name, v in (("l2", l2), ("max", mx)):
            if v > worst[name][0]:
                worst[name] = (v, case)
        assert l2 <= TOL and mx <= TOL, (case, l2, mx)
        assert np.array_equal(y, one), case
    for name in ("l2", "max"):
        print("resamp-random worst %s=%.3g at %s" % (name, worst[name][0], worst[name][1]))
