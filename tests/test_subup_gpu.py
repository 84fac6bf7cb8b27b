"""The per-bin interpolating FIR stage over frames (if_fir_subup_t, docs/SPEC.md §16) on the GPU against the float64 interpolator
it is defined by (tests/subup_ref.py channel_f64: combiner_ref.reference per bin), SPEC §3 tolerance over the whole output; with
all words 0 the bits of the float32 order model; stream cuts, grid limits, input formats, positions past 2^32 and retunes bit
for bit; the library's own interpolator per bin; the chain filter bank -> decimating stage -> this stage -> synthesis bank on
device pointers.  Device output buffers carry a sentinel guard behind their last value, and the guard is checked."""
import functools

import numpy as np
import pytest

import sub_ref
import subup_ref
from matrix_util import edge_taps, row_edge_taps, signal

TOL = 1e-6          # SPEC §16: §3's bound over all bins of all frames together (the complex64 model stays below 5e-7)
GUARD = 64          # float32 words behind the last output
SENTINEL = 12345.0
# (B, T, rows, R): one bin, one tap; B one short of a wave; R that does not divide T (a ragged last tap row, J = 6); J = 32;
# T < R: phases without a tap; a row per bin at a B that no tile divides; the longest row; the widest frame
MATRIX = ((1, 1, 1, 1), (63, 16, 1, 2), (65, 17, 65, 3), (200, 224, 1, 7), (64, 33, 64, 64), (130, 48, 130, 5), (64, 2048, 1, 64),
          (4096, 2, 1, 1))


def stream_frames(B, R):
    return 97 if B == 4096 or R == 64 else 701


def oracle_mod():
    import __graft_entry__ as g
    return g.load_oracle()


@functools.lru_cache(maxsize=None)
def taps_of(B, T, rows, R):
    """every phase's first and last tap loud (matrix_util.row_edge_taps); a row per bin: another seed per row"""
    h = row_edge_taps(T, R, False) if rows == 1 else np.stack([row_edge_taps(T, R, False, seed=j) for j in range(B)])
    h = np.ascontiguousarray(h, dtype=np.float32)
    h.setflags(write=False)
    return h


@functools.lru_cache(maxsize=None)
def words_of(B, mixed):
    return tuple(sub_ref.phase_word(f) for f in sub_ref.mixed_words(B)) if mixed else (0,) * B


def freqs_of(B, mixed):
    return sub_ref.mixed_words(B) if mixed else None


@functools.lru_cache(maxsize=None)
def reference(B, T, rows, R, i16, mixed, F, first=0):
    X = subup_ref.as_frames(signal(oracle_mod(), F * B, i16)[1], B)
    ref = subup_ref.channel_f64(taps_of(B, T, rows, R), X, R, words_of(B, mixed), first)
    ref.setflags(write=False)
    return ref


@functools.lru_cache(maxsize=None)
def model(B, T, rows, R, i16, F):
    xf = signal(oracle_mod(), F * B, i16)[1]
    y = subup_ref.model_c64(taps_of(B, T, rows, R), xf.view(np.complex64).reshape(F, B), R, words_of(B, False))
    y.setflags(write=False)
    return y


@pytest.fixture(scope="module")
def torch_cuda(gpu_ok):
    import torch
    torch.cuda.set_device(0)
    return torch


def run_device(torch, f, raw, pieces, formats=None):
    """feed `raw` (frames of f.bins elements) from ONE device buffer in consecutive pieces of frames; returns the (frames out,
    bins) complex64 array.  With `formats` (one input format per piece, set before that piece) `raw` maps each format to the
    stream in that format.  frame_count is checked at every step."""
    both = {None: raw} if formats is None else raw
    B, R = f.bins, f.interpolation
    F = next(iter(both.values())).size // (2 * B)
    assert all(v.size == 2 * F * B for v in both.values())
    din = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in both.items()}
    total = F * R
    buf = torch.full((2 * total * B + GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()   # the buffers are filled on torch's stream, the context works on its own
    pos = 0
    for k, s in enumerate(pieces):
        if formats is not None:
            f.set_input_format(formats[k])
        src = din[None if formats is None else formats[k]]
        want = f.frame_count(s)
        got = f.process_device(src.data_ptr() + 2 * src.element_size() * pos * B, buf.data_ptr() + 8 * pos * R * B, s)
        assert got == want == s * R, (pos, s, got, want)
        pos += s
    f.synchronize()
    assert pos == F
    h = buf.cpu().numpy()
    assert np.all(h[2 * total * B:] == SENTINEL), "the guard behind the last output was written"
    return h[:2 * total * B].view(np.complex64).reshape(total, B).copy()


def check(oracle, y, ref, what, tol=TOL):
    l2, mx = oracle.err_metrics(subup_ref.iq(y), subup_ref.iq(ref))
    print("subup %s: l2=%.3g max=%.3g" % (what, l2, mx))
    assert l2 <= tol and mx <= tol, (what, l2, mx)
    return l2, mx


def same_bits(a, b):
    if a.shape != b.shape:
        print("subup shapes differ: %r, %r" % (a.shape, b.shape))
        return False
    wa, wb = np.ascontiguousarray(a).view(np.uint32).reshape(-1), np.ascontiguousarray(b).view(np.uint32).reshape(-1)
    d = np.flatnonzero(wa != wb)
    if d.size:
        fa, fb = wa.view(np.float32), wb.view(np.float32)
        print("subup bits differ in %d of %d words, first at %d (%r, %r), largest difference %g" % (
            d.size, wa.size, d[0], fa[d[0]], fb[d[0]], np.max(np.abs(fa[d].astype(np.float64) - fb[d]))))
    return d.size == 0


@pytest.mark.gpu
@pytest.mark.parametrize("mixed", [False, True])
@pytest.mark.parametrize("i16", [False, True])
@pytest.mark.parametrize("B,T,rows,R", MATRIX)
def test_matrix_against_float64(gpu_ok, fir, oracle, torch_cuda, B, T, rows, R, i16, mixed):
    """every phase's taps loud at both ends; the host path in two calls within tolerance of the float64 interpolator per bin
    over the whole output, the device path the same bits; all words 0: the bits of the float32 order model"""
    F = stream_frames(B, R)
    raw, _ = signal(oracle, F * B, i16)
    cut = F // 3 + 1
    with fir.IfFirSubUp(taps_of(B, T, rows, R), B, R, max_frames=F) as f:
        if i16:
            f.set_input_format(fir.INPUT_I16)
        f.set_nco(freqs_of(B, mixed))
        y = np.concatenate([f.process(raw[:2 * cut * B]), f.process(raw[2 * cut * B:])])
        f.reset()
        yd = run_device(torch_cuda, f, raw, [cut, F - cut])
    ref = reference(B, T, rows, R, i16, mixed, F)
    assert y.shape == ref.shape == (F * R, B)
    check(oracle, y, ref, "matrix B=%d T=%d rows=%d R=%d i16=%d mixed=%d" % (B, T, rows, R, i16, mixed))
    assert same_bits(yd, y)
    if not mixed:
        m = model(B, T, rows, R, i16, F)
        assert same_bits(y, m), np.max(np.abs(y - m))
    if T < R:
        # the phases p >= T have no tap: exactly zero
        assert not np.any(y.reshape(F, R, B)[:, T:, :])


@pytest.mark.gpu
def test_every_pair_of_cuts_bit_for_bit(gpu_ok, fir, oracle, torch_cuda):
    """(65, 17, 65, 3), mixed words, 24 frames: a three-call split at every pair of cut points (calls of 0 frames and calls
    shorter than the history of 5 frames among them) gives the bits of one call"""
    torch = torch_cuda
    B, T, rows, R, F = 65, 17, 65, 3, 24
    raw, _ = signal(oracle, F * B, False)
    total = F * R
    src = torch.from_numpy(np.ascontiguousarray(raw)).cuda()
    with fir.IfFirSubUp(taps_of(B, T, rows, R), B, R, max_frames=F) as f:
        f.set_nco(freqs_of(B, True))
        one = run_device(torch, f, raw, [F])
        check(oracle, one, reference(B, T, rows, R, False, True, F), "cuts")
        bad = []
        for a in range(F + 1):
            outs = [torch.full((2 * total * B + GUARD,), SENTINEL, dtype=torch.float32, device="cuda") for _ in range(a, F + 1)]
            torch.cuda.synchronize()   # (filled on torch's stream, written on the context's)
            for b, buf in zip(range(a, F + 1), outs):
                f.reset()
                pos = 0
                for s in (a, b - a, F - b):
                    assert f.process_device(src.data_ptr() + 8 * pos * B, buf.data_ptr() + 8 * pos * R * B, s) == s * R
                    pos += s
            f.synchronize()
            for b, buf in zip(range(a, F + 1), outs):
                h = buf.cpu().numpy()
                if not (np.all(h[2 * total * B:] == SENTINEL) and same_bits(h[:2 * total * B].view(np.complex64).reshape(total, B), one)):
                    bad.append((a, b))
        assert not bad, bad[:10]


@pytest.mark.gpu
@pytest.mark.parametrize("B,T,rows,R", [(65, 17, 65, 3), (200, 224, 1, 7)])
def test_one_frame_per_call_with_empty_calls_between(gpu_ok, fir, oracle, torch_cuda, B, T, rows, R):
    F = 2 * subup_ref.ceil_div(T, R) + 17
    raw, _ = signal(oracle, F * B, False)
    with fir.IfFirSubUp(taps_of(B, T, rows, R), B, R, max_frames=F) as f:
        f.set_nco(freqs_of(B, True))
        one = run_device(torch_cuda, f, raw, [F])
        check(oracle, one, reference(B, T, rows, R, False, True, F), "frame by frame B=%d" % B)
        f.reset()
        assert same_bits(run_device(torch_cuda, f, raw, [1, 0] * F), one)


@pytest.mark.gpu
def test_formats_are_the_same_stream(gpu_ok, fir, oracle, torch_cuda):
    """int16 input == float32 input of the converted values, bit for bit; a format switch mid-stream changes no bit"""
    B, T, rows, R, F = 130, 48, 130, 5, 300
    xi, xf = signal(oracle, F * B, True)
    with fir.IfFirSubUp(taps_of(B, T, rows, R), B, R, max_frames=F) as f:
        f.set_nco(freqs_of(B, True))
        one = run_device(torch_cuda, f, xf, [F])
        check(oracle, one, reference(B, T, rows, R, True, True, F), "formats")
        f.reset()
        f.set_input_format(fir.INPUT_I16)
        assert same_bits(run_device(torch_cuda, f, xi, [F]), one)
        f.reset()
        pieces = [7, 1, 40, 0, 3, 100, 149]
        formats = [(fir.INPUT_F32, fir.INPUT_I16)[k % 2] for k in range(len(pieces))]
        assert same_bits(run_device(torch_cuda, f, {fir.INPUT_F32: xf, fir.INPUT_I16: xi}, pieces, formats=formats), one)


@pytest.mark.gpu
@pytest.mark.parametrize("B,T,rows,R", [(200, 224, 1, 7), (65, 17, 65, 3)])
def test_grid_limits_give_the_same_bits(gpu_ok, fir, oracle, torch_cuda, B, T, rows, R):
    """1 and 3 workgroups walk all tiles (more than three, the last one ragged): the bits of the default launch"""
    F = stream_frames(B, R)
    raw, _ = signal(oracle, F * B, False)
    with fir.IfFirSubUp(taps_of(B, T, rows, R), B, R, max_frames=F, dev=True) as f:
        f.set_nco(freqs_of(B, True))
        tile = f.debug_config()
        # a tile is 256 items of 32 input frames each; the calls below deal ceil(frames / 32) R B items
        assert tile == 256 * 32
        for frames in (F // 2, F - F // 2):
            items = subup_ref.ceil_div(frames, 32) * R * B
            assert items > 3 * 256 and items % 256
        runs = []
        for limit in (0, 1, 3):
            f.debug_config(grid_limit=limit)
            f.reset()
            runs.append(run_device(torch_cuda, f, raw, [F // 2, F - F // 2]))
    check(oracle, runs[0], reference(B, T, rows, R, False, True, F), "grid B=%d" % B)
    assert same_bits(runs[0], runs[1]) and same_bits(runs[0], runs[2])


@pytest.mark.gpu
@pytest.mark.parametrize("where", ["2^32-3", "2^63/R", "last"])
def test_stream_positions(gpu_ok, fir, oracle, torch_cuda, where):
    """through the development hook the context starts at an absolute input frame index with a zero history: the outputs are
    the float64 interpolator's at that position; a cut gives the same bits; position 0 gives other values"""
    B, T, rows, R, F = 130, 48, 130, 5, 101
    start = {"2^32-3": (1 << 32) - 3, "2^63/R": (1 << 63) // R, "last": subup_ref.last_start(F, R)}[where]
    raw, _ = signal(oracle, F * B, False)
    with fir.IfFirSubUp(taps_of(B, T, rows, R), B, R, max_frames=F, dev=True) as f:
        f.set_nco(freqs_of(B, True))
        f.debug_config(position=start)
        assert f.frame_count(F) == subup_ref.frame_count(start, F, R) == F * R
        one = run_device(torch_cuda, f, raw, [F])
        check(oracle, one, reference(B, T, rows, R, False, True, F, start), "position %s" % where)
        if where == "last":
            assert f.frame_count(1) == 0   # the stream has reached its end
        f.debug_config(position=start)
        assert same_bits(run_device(torch_cuda, f, raw, [2, 1, 0, 50, F - 53]), one)
        f.reset()
        assert not np.array_equal(run_device(torch_cuda, f, raw, [F]), one)


@pytest.mark.gpu
def test_positions_2_32_apart_agree(gpu_ok, fir, oracle, torch_cuda):
    """the kernel is given call-relative frames and (c R) mod 2^32: c and c + 2^32 give the same bits"""
    B, T, rows, R, F = 65, 17, 65, 3, 40
    raw, _ = signal(oracle, F * B, False)
    with fir.IfFirSubUp(taps_of(B, T, rows, R), B, R, max_frames=F, dev=True) as f:
        f.set_nco(freqs_of(B, True))
        runs = []
        for c in (12345, 12345 + (1 << 32), 12345 + (5 << 32)):
            f.debug_config(position=c)
            runs.append(run_device(torch_cuda, f, raw, [F]))
    check(oracle, runs[0], reference(B, T, rows, R, False, True, F, 12345), "position 12345")
    assert same_bits(runs[0], runs[1]) and same_bits(runs[0], runs[2])


@pytest.mark.gpu
def test_retunes(gpu_ok, fir, oracle, torch_cuda):
    """the same words set again: no bit changed; W1 for call a then W2 for call b: b's output is that of a context that had
    W2 from the start; get_nco returns the quantised values; refused frequencies leave the words in force"""
    B, T, rows, R, F = 130, 48, 130, 5, 200
    cut = 83
    raw, _ = signal(oracle, F * B, False)
    w1 = sub_ref.mixed_words(B)
    w2 = sub_ref.mixed_words(B, seed=1)[::-1].copy()
    with fir.IfFirSubUp(taps_of(B, T, rows, R), B, R, max_frames=F, dev=True) as f:
        assert np.array_equal(f.get_nco(), np.zeros(B))
        f.set_nco(w1)
        quantised = np.array([sub_ref.word_freq(sub_ref.phase_word(v)) for v in w1])
        assert np.array_equal(f.get_nco(), quantised) and np.max(np.abs(quantised - np.where(w1 == 0.5, -0.5, w1))) <= 2.0 ** -33
        one = run_device(torch_cuda, f, raw, [F])
        f.reset()
        a1 = run_device(torch_cuda, f, raw[:2 * cut * B], [cut])
        f.set_nco(w1)
        f.set_nco(f.get_nco())
        b1 = run_device(torch_cuda, f, raw[2 * cut * B:], [F - cut])
        assert same_bits(np.concatenate([a1, b1]), one)
        for bad, said in ((0.5000001, "0.5"), (-0.6, "-0.6"), (float("nan"), "nan"), (float("inf"), "inf")):
            w = w2.copy()
            w[B - 1] = bad
            with pytest.raises(fir.IfFirError) as e:
                f.set_nco(w)
            assert str(e.value) == "if_fir_subup_set_nco: frequency must be within +-0.5 cycles/sample (got %s)" % said
            assert np.array_equal(f.get_nco(), quantised)
        # W1 for call a, W2 for call b
        f.reset()
        run_device(torch_cuda, f, raw[:2 * cut * B], [cut])
        f.set_nco(w2)
        b2 = run_device(torch_cuda, f, raw[2 * cut * B:], [F - cut])
        f.reset()
        want = run_device(torch_cuda, f, raw, [cut, F - cut])
        assert same_bits(b2, want[cut * R:]) and not np.array_equal(b2, b1)
        f.set_nco(None)
        assert np.array_equal(f.get_nco(), np.zeros(B))


@pytest.mark.gpu
def test_every_bin_is_the_library_interpolator(gpu_ok, fir, oracle, torch_cuda):
    """(3, 48, 3, 5): every bin against an IfFirInterp context of the same taps, L = R and set_nco(f_j), fed that bin's stream;
    each side is within 1e-6 of float64, so the pair is within the sum"""
    B, T, rows, R, F = 3, 48, 3, 5, 701
    raw, xf = signal(oracle, F * B, False)
    taps = taps_of(B, T, rows, R)
    freqs = freqs_of(B, True)
    with fir.IfFirSubUp(taps, B, R, max_frames=F) as f:
        f.set_nco(freqs)
        y = f.process(raw)
    check(oracle, y, reference(B, T, rows, R, False, True, F), "interp pair, the stage")
    X = xf.view(np.complex64).reshape(F, B)
    for j in range(B):
        with fir.IfFirInterp(taps[j], R, max_samples=F) as ip:
            ip.set_nco(freqs[j])
            z = ip.process(np.ascontiguousarray(X[:, j]))
        z = np.asarray(z, dtype=np.float32).view(np.complex64)
        assert z.shape == (F * R,)
        check(oracle, y[:, j], z.astype(np.complex128), "interp pair, bin %d" % j, tol=2e-6)


@pytest.mark.gpu
def test_chain_bank_stage_stage_synthesis_on_device(gpu_ok, fir, oracle, torch_cuda):
    """IfFirPfb(M=64, D=32, first bin -12, 24 bins) -> IfFirSub(R=2) -> IfFirSubUp(R=2, T=33, a row per bin, mixed words) ->
    IfFirSynth(M=64, L=64, same span) on one side stream, device pointers only: the new stage's output against the float64
    interpolator fed its actual input; the synthesis bank takes the result"""
    torch = torch_cuda
    M, D, first_bin, B, R, T = 64, 32, -12, 24, 2, 33
    n = 32 * 400
    raw, _ = signal(oracle, n, False)
    proto = row_edge_taps(4 * M, M, False)
    down = np.ascontiguousarray(np.stack([edge_taps(T, 1, False, seed=j) for j in range(B)]), dtype=np.float32)
    side = torch.cuda.Stream()
    frames = n // D
    with fir.IfFirPfb(proto, M, D, first_bin=first_bin, bins=B, max_samples=n) as bank, \
            fir.IfFirSub(down, B, R, max_frames=frames) as stage, \
            fir.IfFirSubUp(taps_of(B, T, B, R), B, R, max_frames=frames // R) as up, \
            fir.IfFirSynth(proto, M, M, first_bin=first_bin, bins=B, max_frames=frames) as synth:
        up.set_nco(freqs_of(B, True))
        for c in (bank, stage, up, synth):
            c.set_stream(side.cuda_stream)
        with torch.cuda.stream(side):
            x = torch.from_numpy(np.ascontiguousarray(raw)).cuda()
            mid = torch.zeros(2 * frames * B, dtype=torch.float32, device="cuda")
            low = torch.zeros(2 * (frames // R) * B, dtype=torch.float32, device="cuda")
            fine = torch.full((2 * frames * B + GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
            wide = torch.zeros(2 * frames * M, dtype=torch.float32, device="cuda")
        side.synchronize()
        assert bank.process_device(x.data_ptr(), mid.data_ptr(), n) == frames
        assert stage.process_device(mid.data_ptr(), low.data_ptr(), frames) == frames // R
        assert up.frame_count(frames // R) == frames
        assert up.process_device(low.data_ptr(), fine.data_ptr(), frames // R) == frames
        assert synth.process_device(fine.data_ptr(), wide.data_ptr(), frames) == (frames // 2) * 2 * 64
        synth.synchronize()
        X = low.cpu().numpy().view(np.complex64).reshape(frames // R, B)
        h = fine.cpu().numpy()
        w = wide.cpu().numpy()
    assert np.all(h[2 * frames * B:] == SENTINEL), "the guard behind the last output was written"
    y = h[:2 * frames * B].view(np.complex64).reshape(frames, B)
    check(oracle, y, subup_ref.channel_f64(taps_of(B, T, B, R), X, R, words_of(B, True)), "chain")
    assert w.size == 2 * (frames // 2) * 2 * 64 and np.all(np.isfinite(w)) and np.max(np.abs(w)) > 0.0


@pytest.mark.gpu
@pytest.mark.filterwarnings("ignore:The CUDA Graph is empty")
def test_refusals_leave_the_stream_where_it_was(gpu_ok, fir, oracle, torch_cuda):
    torch = torch_cuda
    B, T, rows, R, F = 65, 17, 65, 3, 120
    raw, _ = signal(oracle, F * B, False)
    taps = taps_of(B, T, rows, R)
    with fir.IfFirSubUp(taps, B, R, max_frames=F) as f:
        f.set_nco(freqs_of(B, True))
        whole = f.process(raw)
        f.reset()
        head = f.process(raw[:2 * 50 * B])
        said = lambda e: str(e.value)
        with pytest.raises(fir.IfFirError) as e:
            f.process(np.zeros(2 * (F + 1) * B, dtype=np.float32))
        assert said(e) == "if_fir_subup_process: %d frames exceed ullMaxFrames %d of init" % (F + 1, F)
        with pytest.raises(fir.IfFirError) as e:
            f.set_input_format(5)
        assert said(e) == "if_fir_subup_set_input_format: unknown format 5"
        buf = torch.zeros(2 * (F + 1) * B + 8, dtype=torch.float32, device="cuda")
        out = torch.zeros(2 * (F + 1) * R * B + 8, dtype=torch.float32, device="cuda")
        aligned = "if_fir_subup_process_device: device pointers must be aligned to one element: 8-byte (input) and 8-byte (output)"
        with pytest.raises(fir.IfFirError) as e:
            f.process_device(buf.data_ptr() + 4, out.data_ptr(), 10)
        assert said(e) == aligned
        with pytest.raises(fir.IfFirError) as e:
            f.process_device(buf.data_ptr(), out.data_ptr() + 4, 10)
        assert said(e) == aligned
        with pytest.raises(fir.IfFirError) as e:
            f.process_device(0, out.data_ptr(), 10)
        assert said(e) == "if_fir_subup_process_device: NULL device pointer"
        with pytest.raises(fir.IfFirError) as e:
            f.process_device(buf.data_ptr(), 0, 10)
        assert said(e) == "if_fir_subup_process_device: NULL device pointer"
        with pytest.raises(fir.IfFirError) as e:
            f.process_device(buf.data_ptr(), out.data_ptr(), F + 1)
        assert said(e) == "if_fir_subup_process_device: %d frames exceed ullMaxFrames %d of init" % (F + 1, F)
        side = torch.cuda.Stream()
        f.set_stream(side.cuda_stream)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            graph.capture_begin()
            try:
                with pytest.raises(fir.IfFirError) as e:
                    f.process_device(buf.data_ptr(), out.data_ptr(), 10)
            finally:
                graph.capture_end()
        assert said(e).startswith("if_fir_subup_process_device: the context's stream is being captured into a hipGraph")
        f.set_stream(0)
        # every refused call left the stream where it was
        tail = f.process(raw[2 * 50 * B:])
        assert same_bits(np.concatenate([head, tail]), whole)
    # a call whose last output index would pass 2^64 - 1 is refused; the stream goes on and ends as an undisturbed one
    start = subup_ref.last_start(99, R)
    with fir.IfFirSubUp(taps, B, R, max_frames=F, dev=True) as f, fir.IfFirSubUp(taps, B, R, max_frames=F, dev=True) as calm:
        for c in (f, calm):
            c.set_nco(freqs_of(B, True))
            c.debug_config(position=start)
        a = f.process(raw[:2 * 60 * B])
        with pytest.raises(fir.IfFirError) as e:
            f.process(raw[:2 * 40 * B])
        assert str(e.value) == "if_fir_subup_process: frame count too large: the stream position would pass 2^64"
        assert f.frame_count(40) == 0 and f.frame_count(39) == 39 * R
        b = f.process(raw[2 * 60 * B:2 * 99 * B])
        want = calm.process(raw[:2 * 99 * B])
        assert want.shape[0] == 99 * R
        assert same_bits(np.concatenate([a, b]), want)
