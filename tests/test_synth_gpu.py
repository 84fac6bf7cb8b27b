"""The polyphase synthesis bank (if_fir_synth_t, docs/SPEC.md §14) on the GPU against the float64 fold form of tests/synth_ref.py
(which tests/test_synth_host.py holds to the definition at 1e-12), SPEC §3 tolerance over the whole output of a run; stream
cuts, format changes, the two routes, grid limits, workspace chunks, bin spans and frame positions past 2^32 bit for bit; the analysis bank's
device output fed straight back against the float64 transfer formula.  Device output buffers carry a sentinel guard behind
their last value, and the guard is checked."""
import functools

import numpy as np
import pytest

import synth_ref
from matrix_util import row_edge_taps, signal

TOL = 1e-6          # SPEC §14: §3's bound over the whole output of a run (the complex64 model stays below 5e-7)
GUARD = 64          # float32 words behind the last output
SENTINEL = 12345.0
# (M, T, L): every M with the longest prototype at L = M (J = 16) and T off the multiple of M at L = M/2 (J = 6); then a hop that
# divides nothing, J = 30, J = 32 with T < M, a non-divisor hop with T three short of 8 M, T just past M at M = 4096 (J = 2), and
# a hop one short of M
MATRIX = tuple((M, 16 * M, M) for M in synth_ref.SIZES) + tuple((M, 3 * M - 5, M // 2) for M in synth_ref.SIZES) + (
    (64, 187, 17), (128, 300, 10), (64, 32, 1), (1024, 8 * 1024 - 3, 385), (4096, 4096 + 9, 4096), (256, 2047, 255))


def stream_frames(M, T, L):
    """3 J + 2 batches of frames, the last one ragged where a batch has several frames"""
    B = synth_ref.batch(M)
    return (3 * synth_ref.terms(T, L) + 2) * B - B // 3


@pytest.fixture(scope="module")
def torch_cuda(gpu_ok):
    import torch
    torch.cuda.set_device(0)
    return torch


def oracle_mod():
    import __graft_entry__ as g
    return g.load_oracle()


def frames_signal(oracle, frames, bins, i16):
    """(what the library is given, flat; the same values as a (frames, bins) complex array)"""
    raw, x = signal(oracle, frames * bins, i16)
    return raw, synth_ref.as_frames(x, bins)


@functools.lru_cache(maxsize=None)
def reference(M, T, L, i16, frames, first=0, first_bin=0, bins=None):
    X = frames_signal(oracle_mod(), frames, M if bins is None else bins, i16)[1]
    ref = synth_ref.fold_f64(row_edge_taps(T, L, False), X, M, L, first_bin, bins, first)
    ref.setflags(write=False)
    return ref


def run_device(torch, f, raw, pieces, formats=None):
    """feed the frames of `raw` from ONE device buffer in consecutive pieces (frame counts); returns (complex64 outputs, outputs
    per piece).  With `formats` (one input format per piece, set before that piece) `raw` maps each format to the frames in
    that format: the same values in every one, one device buffer each.  sample_count is checked at every step."""
    both = {None: raw} if formats is None else raw
    F = next(iter(both.values())).size // (2 * f.bins)
    assert all(v.size == 2 * F * f.bins for v in both.values())
    din = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in both.items()}
    L, bins = f.hop, f.bins
    buf = torch.full((2 * F * L + GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()   # the context works on a stream of its own
    pos = 0
    counts = []
    for k, s in enumerate(pieces):
        if formats is not None:
            f.set_input_format(formats[k])
        src = din[None if formats is None else formats[k]]
        want = f.sample_count(s)
        got = f.process_device(src.data_ptr() + 2 * src.element_size() * pos * bins, buf.data_ptr() + 8 * pos * L, s)
        assert got == want == s * L, (pos, s, got, want)
        counts.append(got)
        pos += s
    f.synchronize()
    assert pos == F
    h = buf.cpu().numpy()
    assert np.all(h[2 * F * L:] == SENTINEL), "the guard behind the last output was written"
    return h[:2 * F * L].view(np.complex64).copy(), counts


def check(oracle, y, ref, what):
    l2, mx = oracle.err_metrics(synth_ref.iq(y), synth_ref.iq(ref))
    print("synth %s: l2=%.3g max=%.3g" % (what, l2, mx))
    assert l2 <= TOL and mx <= TOL, (what, l2, mx)
    return l2, mx


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


@pytest.mark.gpu
@pytest.mark.parametrize("i16", [False, True])
@pytest.mark.parametrize("M,T,L", MATRIX)
def test_matrix_against_float64(gpu_ok, fir, oracle, torch_cuda, M, T, L, i16):
    """taps loud at both ends of every row; the host path in two calls within tolerance of float64 over the whole output, the
    device path the same bits"""
    F = stream_frames(M, T, L)
    raw, _ = frames_signal(oracle, F, M, i16)
    taps = row_edge_taps(T, L, False)
    cut = F // 3 + 1
    with fir.IfFirSynth(taps, M, L, max_frames=F) as f:
        if i16:
            f.set_input_format(fir.INPUT_I16)
        y = np.concatenate([f.process(raw[:2 * cut * M]), f.process(raw[2 * cut * M:])]).view(np.complex64)
        f.reset()
        yd, _ = run_device(torch_cuda, f, raw, [cut, F - cut])
    ref = reference(M, T, L, i16, F)
    assert y.shape == ref.shape == (F * L,)
    check(oracle, y, ref, "matrix M=%d T=%d L=%d i16=%d" % (M, T, L, i16))
    assert same_bits(yd, y)


RING_CASES = tuple(c for c in MATRIX if synth_ref.lds_route_fits(*c))


@pytest.mark.gpu
@pytest.mark.parametrize("M,T,L", RING_CASES)
def test_routes_agree_bit_for_bit(gpu_ok, fir, oracle, torch_cuda, M, T, L):
    """every matrix case where the LDS ring fits, float32 and int16, in two calls: the workspace route and the ring route give
    the same bits; the plan's own choice is the ring where four workgroups of it fit a CU"""
    torch = torch_cuda
    F = stream_frames(M, T, L)
    cut = F // 3 + 1
    with fir.IfFirSynth(row_edge_taps(T, L, False), M, L, max_frames=F, dev=True) as f:
        assert f.debug_config() == (fir.IfFirSynth.ROUTE_LDS if synth_ref.lds_route_fits(M, T, L, 4) else fir.IfFirSynth.ROUTE_WORKSPACE)
        for i16 in (False, True):
            raw, _ = frames_signal(oracle, F, M, i16)
            f.set_input_format(fir.INPUT_I16 if i16 else fir.INPUT_F32)
            runs = []
            for route in (fir.IfFirSynth.ROUTE_WORKSPACE, fir.IfFirSynth.ROUTE_LDS):
                assert f.debug_config(route=route) == route
                f.reset()
                runs.append(run_device(torch, f, raw, [cut, F - cut])[0])
            assert torch.equal(torch.from_numpy(runs[0].view(np.uint32)), torch.from_numpy(runs[1].view(np.uint32))), i16
            check(oracle, runs[1], reference(M, T, L, i16, F), "routes M=%d T=%d L=%d i16=%d" % (M, T, L, i16))


def test_the_matrix_has_cases_on_both_sides_of_the_ring_fit():
    assert 8 <= len(RING_CASES) < len(MATRIX) and {c[0] for c in RING_CASES} >= {64, 128, 256, 512, 1024}
    assert {synth_ref.lds_route_fits(*c, 4) for c in RING_CASES} == {True, False}


def ragged_pieces(F, J, rng):
    """calls of 0 and 1 frame, pieces shorter than the history, one longer, then random ones"""
    head = [0, 1, 1, 0, 2, max(J - 2, 1), 1, J + 3, 3, 0, 1]
    rest = F - sum(head)
    assert rest > 2 * J
    cuts = np.sort(rng.integers(0, rest + 1, 5))
    return head + [int(v) for v in np.diff(np.concatenate([[0], cuts, [rest]]))]


@pytest.mark.gpu
@pytest.mark.parametrize("M,T,L", [(1024, 8 * 1024 - 3, 385), (64, 16 * 64, 64), (4096, 2 * 4096 - 1, 4095)])
def test_cuts_and_format_changes_bit_for_bit(gpu_ok, fir, oracle, torch_cuda, M, T, L):
    """the frames in ragged pieces, the input format changed between them, against one call: the same bits"""
    F = stream_frames(M, T, L) + 2 * synth_ref.terms(T, L) + 20
    xi, _ = frames_signal(oracle, F, M, True)
    xf = xi.astype(np.float32) * np.float32(2.0 ** -15)
    pieces = ragged_pieces(F, synth_ref.terms(T, L), np.random.default_rng([M, T, L]))
    formats = [(fir.INPUT_F32, fir.INPUT_I16)[(k // 2) % 2] for k in range(len(pieces))]
    with fir.IfFirSynth(row_edge_taps(T, L, False), M, L, max_frames=F) as f:
        one, _ = run_device(torch_cuda, f, xf, [F])
        check(oracle, one, reference(M, T, L, True, F), "cuts M=%d T=%d L=%d" % (M, T, L))
        f.reset()
        y, counts = run_device(torch_cuda, f, {fir.INPUT_F32: xf, fir.INPUT_I16: xi}, pieces, formats=formats)
        assert counts[0] == 0 and 0 in counts[1:] and L in counts and max(counts) > L
        assert same_bits(y, one)
        f.reset()
        f.set_input_format(fir.INPUT_I16)
        y, _ = run_device(torch_cuda, f, xi, [F])
        assert same_bits(y, one)


@pytest.mark.gpu
@pytest.mark.parametrize("M,T,L", [(64, 187, 17), (1024, 3 * 1024 - 5, 512), (4096, 4096 + 9, 4096), (128, 32, 1)])
def test_grid_limits_give_the_same_bits(gpu_ok, fir, oracle, torch_cuda, M, T, L):
    """1, 2 and 3 workgroups walk all batches of frames and all outputs (workspace route) or take the whole call in one, two
    and three runs (ring route, where it fits: every case but M = 4096): the bits of the workspace route's default
    launch"""
    F = stream_frames(M, T, L)
    raw, _ = frames_signal(oracle, F, M, False)
    assert -(-(F + synth_ref.terms(T, L) - 1) // synth_ref.batch(M)) > 6 and F * L > 3 * 256
    routes = [fir.IfFirSynth.ROUTE_WORKSPACE] + ([fir.IfFirSynth.ROUTE_LDS] if synth_ref.lds_route_fits(M, T, L) else [])
    with fir.IfFirSynth(row_edge_taps(T, L, False), M, L, max_frames=F, dev=True) as f:
        runs = []
        for route in routes:
            for limit in (0, 1, 2, 3):
                assert f.debug_config(grid_limit=limit, route=route) == route
                f.reset()
                runs.append(run_device(torch_cuda, f, raw, [F])[0])
    check(oracle, runs[0], reference(M, T, L, False, F), "grid M=%d T=%d L=%d" % (M, T, L))
    for r in runs[1:]:
        assert same_bits(r, runs[0])


@pytest.mark.gpu
@pytest.mark.parametrize("M,T,L", [(64, 187, 17), (1024, 3 * 1024 - 5, 512), (4096, 4096 + 9, 4096)])
def test_chunks_of_a_tiny_workspace_give_the_same_bits(gpu_ok, fir, oracle, torch_cuda, M, T, L):
    """a workspace of J frames (one frame of the call per chunk) and one of J + 5 (six per chunk, a ragged last chunk) against
    the default, which holds the whole call"""
    F = stream_frames(M, T, L)
    J = synth_ref.terms(T, L)
    raw, _ = frames_signal(oracle, F, M, True)
    with fir.IfFirSynth(row_edge_taps(T, L, False), M, L, max_frames=F, dev=True) as f:
        f.set_input_format(fir.INPUT_I16)
        f.debug_config(route=fir.IfFirSynth.ROUTE_WORKSPACE)   # the route that has chunks
        assert f.debug_workspace() >= F
        whole, _ = run_device(torch_cuda, f, raw, [F])
        check(oracle, whole, reference(M, T, L, True, F), "chunks M=%d T=%d L=%d" % (M, T, L))
        for nbytes, per in ((1, 1), (8 * M * (J + 5), 6)):
            assert f.debug_workspace(nbytes) == per and (per == 1 or F % per)
            f.reset()
            y, _ = run_device(torch_cuda, f, raw, [F // 2, F - F // 2])
            assert same_bits(y, whole), nbytes


@pytest.mark.gpu
@pytest.mark.parametrize("M", [1024, 64])
def test_a_bin_span_is_the_full_width_call_with_zeros_elsewhere(gpu_ok, fir, oracle, torch_cuda, M):
    """spans -- all bins from -M/2, a few around DC (wrapping), one bin, two bins across M - 1 -> 0 -- against the full-width
    call whose other channels hold +0: the same bits; and the wrapped span against float64"""
    T, L = 3 * M - 5, M // 2
    F = stream_frames(M, T, L)
    taps = row_edge_taps(T, L, False)
    for first_bin, bins in ((-M // 2, M), (-3, 7), (77 % M, 1), (M - 1, 2)):
        raw, _ = frames_signal(oracle, F, bins, False)
        full = np.zeros((F, M, 2), dtype=np.float32)
        full[:, synth_ref.channels(M, first_bin, bins)] = raw.reshape(F, bins, 2)
        with fir.IfFirSynth(taps, M, L, first_bin=first_bin, bins=bins, max_frames=F) as f:
            y, _ = run_device(torch_cuda, f, raw, [F // 2, F - F // 2])
        with fir.IfFirSynth(taps, M, L, max_frames=F) as f:
            want, _ = run_device(torch_cuda, f, full.reshape(-1), [F])
        assert same_bits(y, want), (first_bin, bins)
        if bins == 7:
            check(oracle, y, reference(M, T, L, False, F, 0, first_bin, bins), "span M=%d first=%d bins=%d" % (M, first_bin, bins))


@pytest.mark.gpu
@pytest.mark.parametrize("start", [(1 << 32) - 5, (1 << 40) + 12345])
@pytest.mark.parametrize("M,T,L", [(256, 2047, 255), (64, 187, 17)])
def test_frame_positions_past_2_32(gpu_ok, fir, oracle, torch_cuda, M, T, L, start):
    """through the development hook the context starts at an absolute frame index whose first output is no multiple of M, with
    a zero history: the outputs are the reference evaluated at that position; a cut (across frame 2^32 for the first start)
    gives the same bits, and position 0 gives other values"""
    assert (start * L) % M
    F = stream_frames(M, T, L)
    for i16 in (False, True):
        raw, _ = frames_signal(oracle, F, M, i16)
        with fir.IfFirSynth(row_edge_taps(T, L, False), M, L, max_frames=F, dev=True) as f:
            if i16:
                f.set_input_format(fir.INPUT_I16)
            f.debug_config(position=start)
            assert f.sample_count(F) == F * L
            one, _ = run_device(torch_cuda, f, raw, [F])
            check(oracle, one, reference(M, T, L, i16, F, start), "position M=%d L=%d start=%d i16=%d" % (M, L, start, i16))
            f.debug_config(position=start)
            y, _ = run_device(torch_cuda, f, raw, [3, 2, 1, F - 6])
            assert same_bits(y, one)
            f.reset()
            zero, _ = run_device(torch_cuda, f, raw, [F])
            assert not np.array_equal(zero, one)


@pytest.mark.gpu
@pytest.mark.parametrize("M,L,Th,Tg", [(64, 32, 4 * 64 + 3, 5 * 64 - 1), (1024, 1024, 3 * 1024 - 5, 2 * 1024 + 7)])
def test_analysis_then_synthesis_on_the_device(gpu_ok, fir, oracle, torch_cuda, M, L, Th, Tg):
    """the frames IfFirPfb (hop L) leaves on the device go straight into IfFirSynth.process_device; the result against the
    float64 transfer formula of SPEC §14 under its bound"""
    torch = torch_cuda
    n = 40 * L + 5
    F = -(-n // L)
    x = signal(oracle, n, False)[1]
    h, g = row_edge_taps(Th, M, False), row_edge_taps(Tg, L, False, seed=1)
    din = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    mid = torch.full((2 * F * M + GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
    out = torch.full((2 * F * L + GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()   # the contexts work on streams of their own
    with fir.IfFirPfb(h, M, L, max_samples=n) as a, fir.IfFirSynth(g, M, L, max_frames=F) as s:
        assert a.process_device(din.data_ptr(), mid.data_ptr(), n) == F
        a.synchronize()
        assert s.process_device(mid.data_ptr(), out.data_ptr(), F) == F * L
        s.synchronize()
    got = out.cpu().numpy()
    assert np.all(got[2 * F * L:] == SENTINEL) and np.all(mid.cpu().numpy()[2 * F * M:] == SENTINEL)
    xc = x.astype(np.float64).reshape(-1, 2)
    want = synth_ref.transfer_f64(h, g, xc[:, 0] + 1j * xc[:, 1], M, L)
    check(oracle, got[:2 * F * L].view(np.complex64), want, "round trip M=%d L=%d" % (M, L))


@pytest.mark.gpu
@pytest.mark.filterwarnings("ignore:The CUDA Graph is empty")
def test_refusals_leave_the_stream_where_it_was(gpu_ok, fir, oracle, torch_cuda):
    torch = torch_cuda
    M, T, L, F = 256, 700, 100, 60
    raw, _ = frames_signal(oracle, F, M, False)
    taps = row_edge_taps(T, L, False)
    for kw in (dict(channels=96), dict(channels=32), dict(channels=8192), dict(channels=0), dict(taps=np.ones(16 * M + 1, dtype=np.float32)),
               dict(taps=np.zeros(0, dtype=np.float32)), dict(hop=0), dict(hop=M + 1), dict(hop=21), dict(taps=np.ones(33, dtype=np.float32), hop=1),
               dict(first_bin=-M // 2 - 1), dict(first_bin=M), dict(bins=0), dict(bins=M + 1), dict(max_frames=0)):
        args = dict(taps=taps, channels=M, hop=L)
        args.update(kw)
        with pytest.raises(fir.IfFirError) as e:
            fir.IfFirSynth(**args)
        assert "if_fir_synth_init" in str(e.value), kw
    with fir.IfFirSynth(np.ones(32, dtype=np.float32), M, 1, max_frames=4):      # J = 32 is the most
        pass
    with fir.IfFirSynth(taps, M, L, max_frames=F, dev=True) as f, fir.IfFirSynth(taps, M, L, max_frames=F, dev=True) as calm:
        state = {"at": 0}

        def undisturbed(what):
            """after a refusal: the next frame through both contexts, the same bits"""
            k = state["at"]
            a, b = f.process(raw[2 * k * M:2 * (k + 1) * M]), calm.process(raw[2 * k * M:2 * (k + 1) * M])
            assert a.size == 2 * L and same_bits(a, b), what
            state["at"] = k + 1

        undisturbed("nothing yet")
        with pytest.raises(fir.IfFirError, match="ullMaxFrames"):
            f.process(np.zeros(2 * (F + 1) * M, dtype=np.float32))
        undisturbed("F > max")
        with pytest.raises(fir.IfFirError, match="format"):
            f.set_input_format(5)
        undisturbed("format")
        with pytest.raises(fir.IfFirError, match="route 7"):
            f.debug_config(route=7)
        undisturbed("unknown route")
        buf = torch.zeros(2 * F * M + 8, dtype=torch.float32, device="cuda")
        out = torch.zeros(2 * F * L + 8, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        with pytest.raises(fir.IfFirError, match="aligned"):
            f.process_device(buf.data_ptr() + 4, out.data_ptr(), 5)
        undisturbed("input alignment")
        with pytest.raises(fir.IfFirError, match="aligned"):
            f.process_device(buf.data_ptr(), out.data_ptr() + 4, 5)
        undisturbed("output alignment")
        with pytest.raises(fir.IfFirError, match="NULL"):
            f.process_device(0, out.data_ptr(), 5)
        undisturbed("NULL")
        side = torch.cuda.Stream()
        f.set_stream(side.cuda_stream)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            graph.capture_begin()
            try:
                with pytest.raises(fir.IfFirError, match="captured"):
                    f.process_device(buf.data_ptr(), out.data_ptr(), 5)
            finally:
                graph.capture_end()
        f.set_stream(0)
        undisturbed("captured stream")
        # the rest of the stream in one call each
        k = state["at"]
        assert same_bits(f.process(raw[2 * k * M:]), calm.process(raw[2 * k * M:]))
    # route 2 where two workgroups of the ring do not fit a CU: refused, and the stream goes on
    Mb, Tb = 4096, 4096 + 9
    rawb, _ = frames_signal(oracle, 4, Mb, False)
    tb = row_edge_taps(Tb, Mb, False)
    assert not synth_ref.lds_route_fits(Mb, Tb, Mb)
    with fir.IfFirSynth(tb, Mb, Mb, max_frames=4, dev=True) as f, fir.IfFirSynth(tb, Mb, Mb, max_frames=4, dev=True) as calm:
        a0, b0 = f.process(rawb[:2 * 2 * Mb]), calm.process(rawb[:2 * 2 * Mb])
        with pytest.raises(fir.IfFirError, match="route 2"):
            f.debug_config(route=fir.IfFirSynth.ROUTE_LDS)
        assert f.debug_config() == fir.IfFirSynth.ROUTE_WORKSPACE
        assert same_bits(a0, b0) and same_bits(f.process(rawb[2 * 2 * Mb:]), calm.process(rawb[2 * 2 * Mb:]))
    # a call that would carry the output position past 2^64 is refused; the stream goes on and ends as an undisturbed one
    start = ((1 << 64) - 1) // L - 50
    with fir.IfFirSynth(taps, M, L, max_frames=F, dev=True) as f, fir.IfFirSynth(taps, M, L, max_frames=F, dev=True) as calm:
        for c in (f, calm):
            c.debug_config(position=start)
        a = f.process(raw[:2 * 30 * M])
        with pytest.raises(fir.IfFirError, match="2\\^64"):
            f.process(raw[:2 * 21 * M])
        assert f.sample_count(21) == 0 and f.sample_count(20) == 20 * L
        b = f.process(raw[2 * 30 * M:2 * 50 * M])
        want = calm.process(raw[:2 * 50 * M])
        assert want.size == 2 * 50 * L
        assert same_bits(np.concatenate([a, b]), want)
