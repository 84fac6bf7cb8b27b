"""The real-input down-converter (if_fir_ddc_t, docs/SPEC.md §10) on the GPU against the float64 definition of tests/ddc_ref.py,
SPEC §3 tolerance; stream cuts, tile and grid edges, retunes and stream positions past 2^32 bit for bit.  Device output buffers
carry a sentinel guard behind their last sample, and the guard is checked."""
import functools

import numpy as np
import pytest

import ddc_ref
from matrix_util import row_edge_taps

TOL = 1e-6
GUARD = 64          # float32 words behind the last output
SENTINEL = 12345.0
# (T, D)
MATRIX = ((255, 4), (127, 1), (255, 16), (1023, 8), (4096, 64), (4096, 1), (1, 5), (3, 64), (63, 64), (64, 64), (65, 64), (1537, 63),
          (100, 3), (33, 2), (1000, 7))
# each row's own frequency, in the order of MATRIX
FREQS = (0.2, -0.37000001, 0.4999, 1 / 4096, -0.5, 0.123456789, -1 / 4096, 0.2, -0.37000001, 0.4999, 0.25, -0.2, 0.37000001, 1e-9, 0.5)
# the rows of test_matrix_with_loud_row_ends: MATRIX, then
LOUD_MATRIX = MATRIX + (
    # a capped tile whose rows hold 16 taps: one segment per row
    (1000, 64),
    # ceil(T / D) = 2, 7, 8, 9, 15, 16, 17, 33 at D = 3: rows of 4, 8, 8, 12, 16, 16, 20, 36 taps, whole rows per segment up
    # to 16 and cut rows beyond, whose first segment holds 4 taps
    (6, 3), (21, 3), (24, 3), (27, 3), (45, 3), (48, 3), (51, 3), (99, 3),
    # only padding in the last row entry of two of the three phases
    (22, 3), (49, 3))


@pytest.fixture(scope="module")
def torch_cuda(gpu_ok):
    import torch
    torch.cuda.set_device(0)
    return torch


def taps_for(fir, T, D, complex_taps):
    """channel-selection low-pass, cut-off 0.45 / D (complex: the shifted design).  if_bpf_design makes odd lengths >= 3: an
    even T is the design of T - 1 taps plus a last tap of an eighth of the centre tap, negated; T = 1 is a single tap."""
    odd = T if T % 2 else T - 1
    if odd < 3:
        h = np.array([1.0, 0.5] if complex_taps else [1.0], dtype=np.float32)
    elif complex_taps:
        h = fir.bpf_design_complex(odd, 0.1 / D, 0.8 / D)
    else:
        h = fir.bpf_design(odd, 0.0, 0.45 / D)
    if odd >= 3 and odd != T:
        width = 2 if complex_taps else 1
        mid = h[(odd // 2) * width:(odd // 2) * width + width]
        h = np.concatenate([h, -mid / np.float32(8)]).astype(np.float32)
    assert h.size == T * (2 if complex_taps else 1)
    return h


def signal(n, i16):
    """(what the context is fed, the same samples as float32); int16 with full-scale samples"""
    import __graft_entry__ as g
    return ddc_ref.real_signal(g.load_oracle(), n, i16)


@functools.lru_cache(maxsize=None)
def reference(fir, T, D, ct, i16, n, word, loud):
    taps = row_edge_taps(T, D, ct) if loud else taps_for(fir, T, D, ct)
    ref = ddc_ref.ddc_f64(taps, signal(n, i16)[1], D, word, ct)
    ref.setflags(write=False)
    return ref


def run_device(torch, f, raw, pieces, first=0, formats=None):
    """feed `raw` from ONE device buffer in consecutive pieces (sample-aligned offsets) to a context at absolute index `first`;
    returns (outputs, counts).  With `formats` (one input format per piece, set before that piece) `raw` maps each format to
    the stream in that format: the same values in every one, one device buffer each."""
    both = {None: raw} if formats is None else raw
    n = next(iter(both.values())).size
    assert all(v.size == n for v in both.values())
    din = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in both.items()}
    D = f.decimation
    total = ddc_ref.out_count(first, n, D)
    buf = torch.full((2 * total + GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
    pos = done = 0
    counts = []
    for k, s in enumerate(pieces):
        if formats is not None:
            f.set_input_format(formats[k])
        src = din[None if formats is None else formats[k]]
        want = f.out_count(s)
        got = f.process_device(src.data_ptr() + src.element_size() * pos, buf.data_ptr() + 8 * done, s)
        assert got == want == ddc_ref.out_count(first + pos, s, D), (pos, s, got, want)
        counts.append(got)
        pos += s
        done += got
    f.synchronize()
    assert pos == n and done == total
    h = buf.cpu().numpy()
    assert np.all(h[2 * total:] == SENTINEL), "the guard behind the last output was written"
    return h[:2 * total], counts


def matrix_cases(rows):
    return [(T, D, ct, i16) for (T, D) in rows for ct in (False, True) for i16 in (False, True)]


def host_and_device(fir, oracle, torch, T, D, ct, i16, n, cut, loud, tag):
    """the row with the NCO off and at its own frequency: the host path in two calls within tolerance of float64, the device
    path the same bits"""
    raw, _ = signal(n, i16)
    taps = row_edge_taps(T, D, ct) if loud else taps_for(fir, T, D, ct)
    freq = FREQS[LOUD_MATRIX.index((T, D)) % len(FREQS)]
    with fir.IfFirDdc(taps, D, max_samples=n, complex_taps=ct, dev=True) as f:
        assert f.tile_outputs() == ddc_ref.tile_shape(T, D)[1]
        if i16:
            f.set_input_format(fir.INPUT_I16)
        for fr in (0.0, freq):
            f.set_nco(fr)
            word = ddc_ref.phase_word(fr)
            assert f.get_nco() == (word - (1 << 32) if word >= 1 << 31 else word) / 2.0 ** 32
            f.reset()
            y = np.concatenate([f.process(raw[:cut]), f.process(raw[cut:])])
            f.reset()
            yd, _ = run_device(torch, f, raw, [cut, n - cut])
            ref = reference(fir, T, D, ct, i16, n, word, loud)
            assert y.size == ref.size == 2 * ddc_ref.out_count(0, n, D)
            l2, mx = oracle.err_metrics(y, ref)
            print("%s T=%d D=%d complex=%d i16=%d f=%r: l2=%.3g max=%.3g" % (tag, T, D, ct, i16, fr, l2, mx))
            assert l2 <= TOL and mx <= TOL, (fr, l2, mx)
            assert np.array_equal(yd, y)


@pytest.mark.gpu
@pytest.mark.parametrize("T,D,ct,i16", matrix_cases(MATRIX))
def test_matrix_against_float64(gpu_ok, fir, oracle, torch_cuda, T, D, ct, i16):
    n = 60_000
    host_and_device(fir, oracle, torch_cuda, T, D, ct, i16, n, n // 3, False, "ddc-matrix")


@pytest.mark.gpu
@pytest.mark.parametrize("T,D,ct,i16", matrix_cases(LOUD_MATRIX))
def test_matrix_with_loud_row_ends(gpu_ok, fir, oracle, torch_cuda, T, D, ct, i16):
    """every phase row's first and last tap are the largest of the filter (tests/test_ddc_host.py: dropping one costs more
    than 1e-2), on the shortest stream with three whole tiles and a ragged one; the int16 stream carries full-scale samples.
    One cut that is a multiple of neither D (where D > 1) nor the tile's input count."""
    K, tile_out, tile_in = ddc_ref.tile_shape(T, D)
    n = ddc_ref.stream_len(T, D)
    assert n <= 1 << 17 and ddc_ref.out_count(0, n, D) > 3 * tile_out and ddc_ref.out_count(0, n, D) % tile_out
    cut = n // 3
    while cut % tile_in == 0 or (D > 1 and cut % D == 0):
        cut += 1
    assert 0 < cut < n
    host_and_device(fir, oracle, torch_cuda, T, D, ct, i16, n, cut, True, "ddc-loud")


@pytest.mark.gpu
@pytest.mark.parametrize("ct,i16", [(False, False), (True, True)])
@pytest.mark.parametrize("T,D", [(255, 4), (1023, 8), (4096, 64), (1537, 63)])
def test_pieces_around_the_history(gpu_ok, fir, oracle, torch_cuda, T, D, ct, i16):
    """calls of T - 2, T - 1, T, 1, 0, forty times 1 and D - 1 samples, then the rest: in the short ones the first workgroup
    builds the next history from the old history and the call.  Bit for bit the one-call run, which meets float64.  Then the
    same stream as float32 and, from a cut inside the first tile on, as int16: a change of format keeps the stream."""
    K, tile_out, tile_in = ddc_ref.tile_shape(T, D)
    head = [T - 2, T - 1, T, 1, 0] + 40 * [1] + [D - 1]
    n = max(ddc_ref.stream_len(T, D), sum(head) + tile_in + T + 17)
    raw, _ = signal(n, i16)
    xi, xf = signal(n, True)
    both = {fir.INPUT_F32: xf, fir.INPUT_I16: xi}
    freq = -0.37000001
    with fir.IfFirDdc(row_edge_taps(T, D, ct), D, max_samples=n, complex_taps=ct) as f:
        f.set_nco(freq)
        if i16:
            f.set_input_format(fir.INPUT_I16)
        one, _ = run_device(torch_cuda, f, raw, [n])
        l2, mx = oracle.err_metrics(one, reference(fir, T, D, ct, i16, n, ddc_ref.phase_word(freq), True))
        print("ddc-pieces T=%d D=%d complex=%d i16=%d: l2=%.3g max=%.3g" % (T, D, ct, i16, l2, mx))
        assert l2 <= TOL and mx <= TOL, (l2, mx)
        f.reset()
        y, counts = run_device(torch_cuda, f, raw, head + [n - sum(head)])
        assert counts[4] == 0 and np.array_equal(y, one)
        if not i16:   # (the int16 values as float32: the stream the mixed run carries)
            f.reset()
            one, _ = run_device(torch_cuda, f, xf, [n])
        pieces = [tile_in // 2 + 1, 0, T - 2, n - tile_in // 2 - T + 1]
        assert pieces[0] % tile_in and min(pieces) >= 0 and pieces[0] < tile_in
        f.reset()
        y, _ = run_device(torch_cuda, f, both, pieces, formats=[fir.INPUT_F32, fir.INPUT_F32, fir.INPUT_I16, fir.INPUT_I16])
        assert np.array_equal(y, one)
        f.reset()
        f.set_input_format(fir.INPUT_I16)
        y, _ = run_device(torch_cuda, f, xi, [n])
        assert np.array_equal(y, one)


# (T, D, loud, complex taps, int16): designed and loud taps; the tiles the LDS fit caps, (4096, 64) to 188 and (1000, 64) to 236
# outputs; the other input format on a full and on a capped tile
TILE_EDGES = [pytest.param(255, 4, False, False, False, id="255-4"), pytest.param(1023, 8, False, False, False, id="1023-8"),
              pytest.param(100, 3, True, False, False, id="100-3-loud"),
              pytest.param(4096, 64, True, False, False, id="4096-64-loud"),
              pytest.param(1000, 64, True, False, False, id="1000-64-loud"),
              pytest.param(255, 16, True, True, True, id="255-16-loud-complex-i16"),
              pytest.param(1000, 64, True, True, True, id="1000-64-loud-complex-i16")]


@pytest.mark.gpu
@pytest.mark.parametrize("T,D,loud,ct,i16", TILE_EDGES)
def test_tile_and_grid_edges(gpu_ok, fir, oracle, torch_cuda, T, D, loud, ct, i16):
    """output counts one less than, equal to and one more than 1 tile and 5 tiles; the grid capped to 1 and to 3 workgroups
    gives the bits of the uncapped run"""
    taps = row_edge_taps(T, D, ct) if loud else taps_for(fir, T, D, ct)
    freq = 0.2
    with fir.IfFirDdc(taps, D, max_samples=1 << 19, complex_taps=ct, dev=True) as f:
        f.set_nco(freq)
        if i16:
            f.set_input_format(fir.INPUT_I16)
        tile = f.tile_outputs()
        assert tile == ddc_ref.tile_shape(T, D)[1] and tile > 0 and tile % 4 == 0
        n_for = lambda outs: (outs - 1) * D + 1          # the fewest inputs that emit `outs` outputs
        n_max = n_for(5 * tile + 1)
        raw, x = signal(n_max, i16)
        ref_all = ddc_ref.ddc_f64(taps, x, D, ddc_ref.phase_word(freq), ct)
        for want in (tile - 1, tile, tile + 1, 5 * tile - 1, 5 * tile, 5 * tile + 1):
            n = n_for(want)
            assert ddc_ref.out_count(0, n, D) == want
            runs = []
            for limit in (0, 1, 3):
                f.debug_config(grid_limit=limit)
                f.reset()
                y, _ = run_device(torch_cuda, f, raw[:n], [n])
                runs.append(y)
            assert np.array_equal(runs[0], runs[1]) and np.array_equal(runs[0], runs[2]), want
            l2, mx = oracle.err_metrics(runs[0], ref_all[:2 * want])
            assert l2 <= TOL and mx <= TOL, (want, l2, mx)


@pytest.mark.gpu
@pytest.mark.parametrize("T,D,ct,i16", [(255, 4, False, False), (1023, 8, True, True), (63, 64, False, True)])
def test_retune_is_as_if_set_since_the_reset(gpu_ok, fir, oracle, torch_cuda, T, D, ct, i16):
    """feed a, set_nco(f2), feed b: the outputs of b are, bit for bit, those of a fresh context at f2 fed a || b; get_nco
    returns the quantised value"""
    n, cut = 30_011, 12_345
    f1, f2 = 0.2, -0.37000001
    raw, x = signal(n, i16)
    taps = row_edge_taps(T, D, ct)
    with fir.IfFirDdc(taps, D, max_samples=n, complex_taps=ct) as f, fir.IfFirDdc(taps, D, max_samples=n, complex_taps=ct) as fresh:
        for c in (f, fresh):
            if i16:
                c.set_input_format(fir.INPUT_I16)
        assert f.get_nco() == 0.0
        f.set_nco(f1)
        assert f.get_nco() == round(f1 * 2 ** 32) / 2.0 ** 32 != f1
        ya = f.process(raw[:cut])
        f.set_nco(f2)
        assert f.get_nco() == round(f2 * 2 ** 32) / 2.0 ** 32
        yb = f.process(raw[cut:])
        fresh.set_nco(f2)
        whole = fresh.process(raw)
        assert np.array_equal(yb, whole[ya.size:])
        assert not np.array_equal(ya, whole[:ya.size])
        l2, mx = oracle.err_metrics(whole, ddc_ref.ddc_f64(taps, x, D, ddc_ref.phase_word(f2), ct))
        assert l2 <= TOL and mx <= TOL, (l2, mx)
        l2, mx = oracle.err_metrics(ya, ddc_ref.ddc_f64(taps, x[:cut], D, ddc_ref.phase_word(f1), ct))
        assert l2 <= TOL and mx <= TOL, (l2, mx)


@pytest.mark.gpu
@pytest.mark.parametrize("D", [3, 64])
@pytest.mark.parametrize("start", [(1 << 32) - 1000, (1 << 40) + 3])
def test_stream_positions_past_2_32(gpu_ok, fir, oracle, torch_cuda, D, start):
    """through the development hook the context starts at an absolute index near 2^32 and past 2^40 with a zero history: the
    outputs are the definition evaluated with that offset (which output indices a call emits, and every output's phase, come
    from the 64-bit index), and a cut across 2^32 gives the bits of the uncut run"""
    T, n, freq = 255, 20_000, 0.123456789
    for ct, i16 in ((False, False), (True, True)):
        raw, x = signal(n, i16)
        taps = row_edge_taps(T, D, ct)
        ref = ddc_ref.ddc_f64(taps, x, D, ddc_ref.phase_word(freq), ct, first=start)
        with fir.IfFirDdc(taps, D, max_samples=n, complex_taps=ct, dev=True) as f:
            f.set_nco(freq)
            if i16:
                f.set_input_format(fir.INPUT_I16)
            f.debug_config(position=start)
            one, _ = run_device(torch_cuda, f, raw, [n], first=start)
            assert one.size == ref.size == 2 * ddc_ref.out_count(start, n, D)
            l2, mx = oracle.err_metrics(one, ref)
            print("ddc-position D=%d start=%d complex=%d i16=%d: l2=%.3g max=%.3g" % (D, start, ct, i16, l2, mx))
            assert l2 <= TOL and mx <= TOL, (l2, mx)
            f.debug_config(position=start)
            y, _ = run_device(torch_cuda, f, raw, [997, 5, 1, n - 1003], first=start)   # 2^32 lies inside the second piece
            assert np.array_equal(y, one)
            # the position is not the index modulo 2^32: from 0 the same samples give other outputs
            f.reset()
            zero, _ = run_device(torch_cuda, f, raw, [n])
            assert zero.size != one.size or not np.array_equal(zero, one)


@pytest.mark.gpu
@pytest.mark.parametrize("T,D", [(255, 4), (1023, 8)])
def test_against_widening_and_the_decimator(gpu_ok, fir, oracle, T, D):
    """what users do today: IfFir with set_nco fed (r, 0) -- both within SPEC §3 of float64"""
    n, freq = 40_000, 0.2
    _, x = signal(n, False)
    taps = taps_for(fir, T, D, False)
    ref = ddc_ref.ddc_f64(taps, x, D, ddc_ref.phase_word(freq))
    with fir.IfFirDdc(taps, D, max_samples=n) as f:
        f.set_nco(freq)
        y = f.process(x)
    with fir.IfFir(taps, decimation=D, max_samples=n) as chain:
        chain.set_nco(freq)
        wide = chain.process(np.stack([x, np.zeros_like(x)], axis=1).reshape(-1))
    assert y.size == wide.size == ref.size
    for name, got in (("down-converter", y), ("chain", wide)):
        l2, mx = oracle.err_metrics(got, ref)
        assert l2 <= TOL and mx <= TOL, (name, l2, mx)


@pytest.mark.gpu
def test_degenerate_calls(gpu_ok, fir):
    T, D, n = 100, 64, 700
    _, x = signal(n, False)
    with fir.IfFirDdc(taps_for(fir, T, D, False), D, max_samples=n) as f:
        f.set_nco(0.2)
        one = f.process(x)
        assert one.size == 2 * -(-n // D)
        f.reset()
        assert f.process(x[:0]).size == 0 and f.out_count(0) == 0
        parts = [f.process(x[i:i + 1]) for i in range(n)]
        assert sum(1 for p in parts if p.size == 0) == n - one.size // 2   # most calls emit nothing
        assert np.array_equal(np.concatenate(parts), one)


@pytest.mark.gpu
@pytest.mark.filterwarnings("ignore:The CUDA Graph is empty")
def test_reset_and_rejected_arguments(gpu_ok, fir, torch_cuda):
    torch = torch_cuda
    n, D = 10_000, 4
    _, x = signal(n, False)
    xi, _ = signal(n, True)
    taps = taps_for(fir, 95, D, False)
    with fir.IfFirDdc(taps, D, max_samples=n) as f:
        f.set_nco(0.2)
        y0 = f.process(x)
        f.process(x[:1001])
        f.reset()
        assert f.get_nco() == round(0.2 * 2 ** 32) / 2.0 ** 32   # a reset keeps the frequency
        assert np.array_equal(f.process(x), y0)
        f.reset()
        f.process(x[:1001])
        with pytest.raises(fir.IfFirError, match="ullMaxSamples"):
            f.process(np.zeros(n + 1, dtype=np.float32))
        with pytest.raises(fir.IfFirError, match="format"):
            f.set_input_format(5)
        for bad in (0.5000001, -0.6, float("nan")):
            with pytest.raises(fir.IfFirError, match="0.5"):
                f.set_nco(bad)
        buf = torch.zeros(2 * n + 8, dtype=torch.float32, device="cuda")
        with pytest.raises(fir.IfFirError, match="aligned"):
            f.process_device(buf.data_ptr() + 2, buf.data_ptr(), 100)
        with pytest.raises(fir.IfFirError, match="aligned"):
            f.process_device(buf.data_ptr(), buf.data_ptr() + 4, 100)
        f.set_input_format(fir.INPUT_I16)
        with pytest.raises(fir.IfFirError, match="aligned"):
            f.process_device(buf.data_ptr() + 1, buf.data_ptr(), 100)
        f.set_input_format(fir.INPUT_F32)
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
        assert np.array_equal(f.process(x[1001:]), y0[2 * ddc_ref.out_count(0, 1001, D):])
    for T, D in ((0, 4), (4097, 4), (31, 0), (31, 65)):
        with pytest.raises(fir.IfFirError) as e:
            fir.IfFirDdc(np.ones(T, dtype=np.float32), D)
        assert str(e.value)


@pytest.mark.gpu
def test_random_configurations_against_float64(gpu_ok, fir, oracle, torch_cuda):
    """40 seeded draws: T log-uniform in 1..4096, D uniform in 1..64, complex taps, int16 input and the frequency drawn per
    case, taps loud at both ends of every phase row, the stream of ddc_ref.stream_len, 2 to 6 pieces with one of 0 samples.
    Every draw meets float64 within SPEC §3, and its pieces give the bits of the single call."""
    rng = np.random.default_rng(20261019)
    worst = {"l2": (0.0, None), "max": (0.0, None)}
    for draw in range(40):
        D = int(rng.integers(1, 65))
        T = min(4096, max(1, int(round(np.exp(rng.uniform(0.0, np.log(4096.0)))))))
        ct, i16 = bool(rng.integers(2)), bool(rng.integers(2))
        freq = (0.0, 0.2, 1 / 4096, float(rng.uniform(-0.5, 0.5)), float(rng.uniform(-0.5, 0.5)))[int(rng.integers(5))]
        n = min(ddc_ref.stream_len(T, D), 1 << 17)
        cuts = np.sort(rng.choice(np.arange(1, n), int(rng.integers(2, 7)) - 2, replace=False))
        pieces = [int(v) for v in np.diff(np.concatenate([[0], cuts, [n]]))]
        pieces.insert(int(rng.integers(len(pieces) + 1)), 0)
        case = "draw %d: T=%d D=%d complex=%d i16=%d f=%r n=%d pieces=%s" % (draw, T, D, ct, i16, freq, n, pieces)
        assert 2 <= len(pieces) <= 6 and sum(pieces) == n, case
        raw, x = signal(n, i16)
        taps = row_edge_taps(T, D, ct, seed=draw)
        ref = ddc_ref.ddc_f64(taps, x, D, ddc_ref.phase_word(freq), ct)
        with fir.IfFirDdc(taps, D, max_samples=n, complex_taps=ct) as f:
            f.set_nco(freq)
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
        assert np.array_equal(y, one), case
    for name in ("l2", "max"):
        print("ddc-random worst %s=%.3g at %s" % (name, worst[name][0], worst[name][1]))


# (T, D): rows of 4, 8 and 16 taps (4, 2 and 1 whole rows per segment, the last segment of an output short), cut rows of 20, 36
# and 64 taps, a capped tile, a single tap, D = 1
ORDER_ROWS = ((1, 5), (22, 3), (45, 3), (255, 16), (63, 64), (1000, 64), (51, 3), (99, 3), (255, 4), (127, 1), (1537, 63))


@pytest.mark.gpu
@pytest.mark.parametrize("ct,i16", [(False, False), (True, True), (True, False), (False, True)])
@pytest.mark.parametrize("T,D", ORDER_ROWS)
def test_order_of_the_spec_bit_for_bit(gpu_ok, fir, oracle, torch_cuda, T, D, ct, i16):
    """With the NCO off (no table of mixed taps, no rotation) the kernel's output equals, bit for bit, the float32 model of
    SPEC §10's arithmetic order (ddc_ref.ddc_f32_order): the rows, the segments and the compensated joins are the ones the
    SPEC states.  Taps loud at both ends of every row, more than one tile, a cut inside the first tile."""
    K, tile_out, tile_in = ddc_ref.tile_shape(T, D)
    n = min(ddc_ref.stream_len(T, D), tile_in + 2 * T + 37 * D + 5)
    raw, x = signal(n, i16)
    taps = row_edge_taps(T, D, ct)
    model = ddc_ref.ddc_f32_order(taps, x, D, 0, ct)
    with fir.IfFirDdc(taps, D, max_samples=n, complex_taps=ct) as f:
        if i16:
            f.set_input_format(fir.INPUT_I16)
        y, _ = run_device(torch_cuda, f, raw, [tile_in // 3 + 1, n - tile_in // 3 - 1])
    assert y.size == model.size
    differ = np.flatnonzero(y != model)
    assert differ.size == 0, (differ.size, differ[:4], y[differ[:4]], model[differ[:4]])
