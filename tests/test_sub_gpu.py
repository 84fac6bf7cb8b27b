"""The per-channel FIR stage over filter-bank frames (if_fir_sub_t, docs/SPEC.md §15) on the GPU against the float64 decimator it
is defined by (tests/sub_ref.py channel_f64: oracle.fir_nco_f64 per bin), SPEC §3 tolerance over the whole output; with all
words 0 the bits of the float32 order model; stream cuts, grid limits, input formats, positions past 2^32 and retunes bit for
bit; the chain filter bank -> stage -> synthesis bank on device pointers.  Device output buffers carry a sentinel guard behind
their last value, and the guard is checked."""
import functools

import numpy as np
import pytest

import sub_ref
from matrix_util import edge_taps, row_edge_taps, signal

TOL = 1e-6          # SPEC §15: §3's bound over all bins of all frames together (the complex64 model stays below 5e-7)
GUARD = 64          # float32 words behind the last output
SENTINEL = 12345.0
# (B, T, rows, R): one bin, one tap; B one short of a wave and one past it; a tile that wraps bins (200); R > T: frames nobody
# weighs; the longest row; a row per bin at a B that no tile divides; the widest frame
MATRIX = ((1, 1, 1, 1), (63, 16, 1, 2), (65, 17, 65, 3), (200, 128, 1, 7), (64, 33, 64, 64), (130, 48, 130, 5), (4096, 2, 1, 1))


def stream_frames(B):
    return 97 if B == 4096 else 701


def oracle_mod():
    import __graft_entry__ as g
    return g.load_oracle()


@functools.lru_cache(maxsize=None)
def taps_of(B, T, rows):
    """loud at both ends of every row; a row per bin: another seed per row"""
    h = edge_taps(T, 1, False) if rows == 1 else np.stack([edge_taps(T, 1, False, seed=j) for j in range(B)])
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
    oracle = oracle_mod()
    X = sub_ref.as_frames(signal(oracle, F * B, i16)[1], B)
    ref = sub_ref.channel_f64(oracle, taps_of(B, T, rows), X, R, words_of(B, mixed), first)
    ref.setflags(write=False)
    return ref


@pytest.fixture(scope="module")
def torch_cuda(gpu_ok):
    import torch
    torch.cuda.set_device(0)
    return torch


def run_device(torch, f, raw, pieces, first=0, formats=None):
    """feed `raw` (frames of f.bins elements) from ONE device buffer in consecutive pieces of frames to a context at absolute
    frame index `first`; returns ((frames out, bins) complex64, frames out per piece).  With `formats` (one input format per
    piece, set before that piece) `raw` maps each format to the stream in that format.  frame_count is checked at every step."""
    both = {None: raw} if formats is None else raw
    B, R = f.bins, f.decimation
    F = next(iter(both.values())).size // (2 * B)
    assert all(v.size == 2 * F * B for v in both.values())
    din = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in both.items()}
    total = sub_ref.frame_count(first, F, R)
    buf = torch.full((2 * total * B + GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()   # the buffers are filled on torch's stream, the context works on its own
    pos = done = 0
    counts = []
    for k, s in enumerate(pieces):
        if formats is not None:
            f.set_input_format(formats[k])
        src = din[None if formats is None else formats[k]]
        want = f.frame_count(s)
        got = f.process_device(src.data_ptr() + 2 * src.element_size() * pos * B, buf.data_ptr() + 8 * done * B, s)
        assert got == want == sub_ref.frame_count(first + pos, s, R), (pos, s, got, want)
        counts.append(got)
        pos += s
        done += got
    f.synchronize()
    assert pos == F and done == total
    h = buf.cpu().numpy()
    assert np.all(h[2 * total * B:] == SENTINEL), "the guard behind the last output was written"
    return h[:2 * total * B].view(np.complex64).reshape(total, B).copy(), counts


def check(oracle, y, ref, what):
    l2, mx = oracle.err_metrics(sub_ref.iq(y), sub_ref.iq(ref))
    print("sub %s: l2=%.3g max=%.3g" % (what, l2, mx))
    assert l2 <= TOL and mx <= TOL, (what, l2, mx)
    return l2, mx


def same_bits(a, b):
    if a.shape != b.shape:
        print("sub shapes differ: %r, %r" % (a.shape, b.shape))
        return False
    wa, wb = np.ascontiguousarray(a).view(np.uint32).reshape(-1), np.ascontiguousarray(b).view(np.uint32).reshape(-1)
    d = np.flatnonzero(wa != wb)
    if d.size:
        fa, fb = wa.view(np.float32), wb.view(np.float32)
        print("sub bits differ in %d of %d words, first at %d (%r, %r), largest difference %g" % (
            d.size, wa.size, d[0], fa[d[0]], fb[d[0]], np.max(np.abs(fa[d].astype(np.float64) - fb[d]))))
    return d.size == 0


@pytest.mark.gpu
@pytest.mark.parametrize("mixed", [False, True])
@pytest.mark.parametrize("i16", [False, True])
@pytest.mark.parametrize("B,T,rows,R", MATRIX)
def test_matrix_against_float64(gpu_ok, fir, oracle, torch_cuda, B, T, rows, R, i16, mixed):
    """taps loud at both ends of every row; the host path in two calls within tolerance of the float64 decimator per bin over
    the whole output, the device path the same bits; all words 0: the bits of the float32 order model"""
    F = stream_frames(B)
    raw, xf = signal(oracle, F * B, i16)
    cut = F // 3 + 1
    with fir.IfFirSub(taps_of(B, T, rows), B, R, max_frames=F) as f:
        if i16:
            f.set_input_format(fir.INPUT_I16)
        f.set_nco(freqs_of(B, mixed))
        y = np.concatenate([f.process(raw[:2 * cut * B]), f.process(raw[2 * cut * B:])])
        f.reset()
        yd, _ = run_device(torch_cuda, f, raw, [cut, F - cut])
    ref = reference(B, T, rows, R, i16, mixed, F)
    assert y.shape == ref.shape == (sub_ref.frame_count(0, F, R), B)
    check(oracle, y, ref, "matrix B=%d T=%d rows=%d R=%d i16=%d mixed=%d" % (B, T, rows, R, i16, mixed))
    assert same_bits(yd, y)
    if not mixed:
        model = sub_ref.model_c64(taps_of(B, T, rows), xf.view(np.complex64).reshape(F, B), R, words_of(B, False))
        assert same_bits(y, model), np.max(np.abs(y - model))


@pytest.mark.gpu
def test_every_pair_of_cuts_bit_for_bit(gpu_ok, fir, oracle, torch_cuda):
    """(65, 17, 65, 3), mixed words, 40 frames: a three-call split at every pair of cut points (calls of 0 frames and calls
    shorter than the history among them) gives the bits of one call"""
    torch = torch_cuda
    B, T, rows, R, F = 65, 17, 65, 3, 40
    raw, _ = signal(oracle, F * B, False)
    total = sub_ref.frame_count(0, F, R)
    src = torch.from_numpy(np.ascontiguousarray(raw)).cuda()
    with fir.IfFirSub(taps_of(B, T, rows), B, R, max_frames=F) as f:
        f.set_nco(freqs_of(B, True))
        one, _ = run_device(torch, f, raw, [F])
        check(oracle, one, reference(B, T, rows, R, False, True, F), "cuts")
        bad = []
        for a in range(F + 1):
            outs = [torch.full((2 * total * B + GUARD,), SENTINEL, dtype=torch.float32, device="cuda") for _ in range(a, F + 1)]
            torch.cuda.synchronize()   # (filled on torch's stream, written on the context's)
            for b, buf in zip(range(a, F + 1), outs):
                f.reset()
                pos = done = 0
                for s in (a, b - a, F - b):
                    done += f.process_device(src.data_ptr() + 8 * pos * B, buf.data_ptr() + 8 * done * B, s)
                    pos += s
                assert done == total
            f.synchronize()
            for b, buf in zip(range(a, F + 1), outs):
                h = buf.cpu().numpy()
                if not (np.all(h[2 * total * B:] == SENTINEL) and same_bits(h[:2 * total * B].view(np.complex64).reshape(total, B), one)):
                    bad.append((a, b))
        assert not bad, bad[:10]


@pytest.mark.gpu
@pytest.mark.parametrize("B,T,rows,R", [(65, 17, 65, 3), (200, 128, 1, 7)])
def test_one_frame_per_call_with_empty_calls_between(gpu_ok, fir, oracle, torch_cuda, B, T, rows, R):
    F = 2 * T
    raw, _ = signal(oracle, F * B, False)
    with fir.IfFirSub(taps_of(B, T, rows), B, R, max_frames=F) as f:
        f.set_nco(freqs_of(B, True))
        one, _ = run_device(torch_cuda, f, raw, [F])
        check(oracle, one, reference(B, T, rows, R, False, True, F), "frame by frame B=%d" % B)
        f.reset()
        y, counts = run_device(torch_cuda, f, raw, [1, 0] * F)
        assert set(counts) == {0, 1}
        assert same_bits(y, one)


@pytest.mark.gpu
def test_formats_are_the_same_stream(gpu_ok, fir, oracle, torch_cuda):
    """int16 input == float32 input of the converted values, bit for bit; a format switch mid-stream changes no bit"""
    B, T, rows, R, F = 130, 48, 130, 5, 300
    xi, xf = signal(oracle, F * B, True)
    with fir.IfFirSub(taps_of(B, T, rows), B, R, max_frames=F) as f:
        f.set_nco(freqs_of(B, True))
        one, _ = run_device(torch_cuda, f, xf, [F])
        check(oracle, one, reference(B, T, rows, R, True, True, F), "formats")
        f.reset()
        f.set_input_format(fir.INPUT_I16)
        y, _ = run_device(torch_cuda, f, xi, [F])
        assert same_bits(y, one)
        f.reset()
        pieces = [7, 1, 40, 0, 3, 100, 149]
        formats = [(fir.INPUT_F32, fir.INPUT_I16)[k % 2] for k in range(len(pieces))]
        y, _ = run_device(torch_cuda, f, {fir.INPUT_F32: xf, fir.INPUT_I16: xi}, pieces, formats=formats)
        assert same_bits(y, one)


@pytest.mark.gpu
@pytest.mark.parametrize("B,T,rows,R", [(200, 128, 1, 7), (65, 17, 65, 3)])
def test_grid_limits_give_the_same_bits(gpu_ok, fir, oracle, torch_cuda, B, T, rows, R):
    """1 and 3 workgroups walk all tiles (more than three, the last one ragged): the bits of the default launch"""
    F = stream_frames(B)
    raw, _ = signal(oracle, F * B, False)
    with fir.IfFirSub(taps_of(B, T, rows), B, R, max_frames=F, dev=True) as f:
        f.set_nco(freqs_of(B, True))
        tile = f.debug_config()
        values = sub_ref.frame_count(0, F, R) * B
        assert tile == 1024 and values > 3 * tile and values % tile
        runs = []
        for limit in (0, 1, 3):
            f.debug_config(grid_limit=limit)
            f.reset()
            runs.append(run_device(torch_cuda, f, raw, [F // 2, F - F // 2])[0])
    check(oracle, runs[0], reference(B, T, rows, R, False, True, F), "grid B=%d" % B)
    assert same_bits(runs[0], runs[1]) and same_bits(runs[0], runs[2])


@pytest.mark.gpu
@pytest.mark.parametrize("where", ["2^32-3", "2^63", "2^64-F-1"])
def test_stream_positions(gpu_ok, fir, oracle, torch_cuda, where):
    """through the development hook the context starts at an absolute frame index with a zero history: the outputs are the
    float64 decimator's at that position; a cut gives the same bits; position 0 gives other values"""
    B, T, rows, R, F = 130, 48, 130, 5, 101
    start = {"2^32-3": (1 << 32) - 3, "2^63": 1 << 63, "2^64-F-1": (1 << 64) - F - 1}[where]
    raw, _ = signal(oracle, F * B, False)
    with fir.IfFirSub(taps_of(B, T, rows), B, R, max_frames=F, dev=True) as f:
        f.set_nco(freqs_of(B, True))
        f.debug_config(position=start)
        assert f.frame_count(F) == sub_ref.frame_count(start, F, R)
        one, _ = run_device(torch_cuda, f, raw, [F], first=start)
        check(oracle, one, reference(B, T, rows, R, False, True, F, start), "position %s" % where)
        f.debug_config(position=start)
        y, _ = run_device(torch_cuda, f, raw, [2, 1, 0, 50, F - 53], first=start)
        assert same_bits(y, one)
        f.reset()
        zero, _ = run_device(torch_cuda, f, raw, [F])
        assert zero.shape != one.shape or not np.array_equal(zero, one)


@pytest.mark.gpu
def test_positions_a_multiple_of_r_2_32_apart_agree(gpu_ok, fir, oracle, torch_cuda):
    """the kernel is given the first output's offset and the low 32 bits of its index: c and c + R 2^32 give the same bits"""
    B, T, rows, R, F = 65, 17, 65, 3, 40
    raw, _ = signal(oracle, F * B, False)
    with fir.IfFirSub(taps_of(B, T, rows), B, R, max_frames=F, dev=True) as f:
        f.set_nco(freqs_of(B, True))
        runs = []
        for c in (12345, 12345 + (R << 32), 12345 + 5 * (R << 32)):
            f.debug_config(position=c)
            runs.append(run_device(torch_cuda, f, raw, [F], first=c)[0])
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
    with fir.IfFirSub(taps_of(B, T, rows), B, R, max_frames=F) as f:
        assert np.array_equal(f.get_nco(), np.zeros(B))
        f.set_nco(w1)
        quantised = np.array([sub_ref.word_freq(sub_ref.phase_word(v)) for v in w1])
        assert np.array_equal(f.get_nco(), quantised) and np.max(np.abs(quantised - np.where(w1 == 0.5, -0.5, w1))) <= 2.0 ** -33
        one, _ = run_device(torch_cuda, f, raw, [F])
        f.reset()
        a1 = run_device(torch_cuda, f, raw[:2 * cut * B], [cut])[0]
        f.set_nco(w1)
        f.set_nco(f.get_nco())
        b1 = run_device(torch_cuda, f, raw[2 * cut * B:], [F - cut], first=cut)[0]
        assert same_bits(np.concatenate([a1, b1]), one)
        for bad, said in ((0.5000001, "0.5"), (-0.6, "-0.6"), (float("nan"), "nan"), (float("inf"), "inf")):
            w = w2.copy()
            w[B - 1] = bad
            with pytest.raises(fir.IfFirError) as e:
                f.set_nco(w)
            assert str(e.value) == "if_fir_sub_set_nco: frequency must be within +-0.5 cycles/sample (got %s)" % said
            assert np.array_equal(f.get_nco(), quantised)
        # W1 for call a, W2 for call b
        f.reset()
        run_device(torch_cuda, f, raw[:2 * cut * B], [cut])
        f.set_nco(w2)
        b2 = run_device(torch_cuda, f, raw[2 * cut * B:], [F - cut], first=cut)[0]
        f.reset()
        want, counts = run_device(torch_cuda, f, raw, [cut, F - cut])
        assert same_bits(b2, want[counts[0]:]) and not np.array_equal(b2, b1)
        f.set_nco(None)
        assert np.array_equal(f.get_nco(), np.zeros(B))


@pytest.mark.gpu
def test_chain_filter_bank_stage_synthesis_on_device(gpu_ok, fir, oracle, torch_cuda):
    """IfFirPfb(M=64, D=32, first bin -12, 24 bins) -> IfFirSub(B=24, R=2, mixed words) -> IfFirSynth(M=64, L=64, same span)
    on one stream, device pointers only: the stage's output against the float64 decimator fed the filter bank's actual
    output; the synthesis bank takes the result"""
    torch = torch_cuda
    M, D, first_bin, B, R, T = 64, 32, -12, 24, 2, 33
    n = 32 * 400
    raw, _ = signal(oracle, n, False)
    proto = row_edge_taps(4 * M, M, False)
    side = torch.cuda.Stream()
    with fir.IfFirPfb(proto, M, D, first_bin=first_bin, bins=B, max_samples=n) as bank, \
            fir.IfFirSub(taps_of(B, T, B), B, R, max_frames=n // D) as stage, \
            fir.IfFirSynth(proto, M, M, first_bin=first_bin, bins=B, max_frames=n // D) as synth:
        stage.set_nco(freqs_of(B, True))
        for c in (bank, stage, synth):
            c.set_stream(side.cuda_stream)
        with torch.cuda.stream(side):
            x = torch.from_numpy(np.ascontiguousarray(raw)).cuda()
            frames = bank.frame_count(n)
            mid = torch.zeros(2 * frames * B, dtype=torch.float32, device="cuda")
            out_frames = stage.frame_count(frames)
            fine = torch.zeros(2 * out_frames * B, dtype=torch.float32, device="cuda")
            wide = torch.zeros(2 * out_frames * M, dtype=torch.float32, device="cuda")
        side.synchronize()
        assert bank.process_device(x.data_ptr(), mid.data_ptr(), n) == frames == n // D
        assert stage.process_device(mid.data_ptr(), fine.data_ptr(), frames) == out_frames == frames // R
        assert synth.process_device(fine.data_ptr(), wide.data_ptr(), out_frames) == out_frames * M
        synth.synchronize()
        X = mid.cpu().numpy().view(np.complex64).reshape(frames, B)
        y = fine.cpu().numpy().view(np.complex64).reshape(out_frames, B)
        w = wide.cpu().numpy()
    ref = sub_ref.channel_f64(oracle, taps_of(B, T, B), X, R, words_of(B, True))
    check(oracle, y, ref, "chain")
    assert np.all(np.isfinite(w)) and np.max(np.abs(w)) > 0.0


@pytest.mark.gpu
@pytest.mark.filterwarnings("ignore:The CUDA Graph is empty")
def test_refusals_leave_the_stream_where_it_was(gpu_ok, fir, oracle, torch_cuda):
    torch = torch_cuda
    B, T, rows, R, F = 65, 17, 65, 3, 120
    raw, _ = signal(oracle, F * B, False)
    taps = taps_of(B, T, rows)
    with fir.IfFirSub(taps, B, R, max_frames=F) as f:
        f.set_nco(freqs_of(B, True))
        whole = f.process(raw)
        f.reset()
        head = f.process(raw[:2 * 50 * B])
        said = lambda e: str(e.value)
        with pytest.raises(fir.IfFirError) as e:
            f.process(np.zeros(2 * (F + 1) * B, dtype=np.float32))
        assert said(e) == "if_fir_sub_process: %d frames exceed ullMaxFrames %d of init" % (F + 1, F)
        with pytest.raises(fir.IfFirError) as e:
            f.set_input_format(5)
        assert said(e) == "if_fir_sub_set_input_format: unknown format 5"
        buf = torch.zeros(2 * (F + 1) * B + 8, dtype=torch.float32, device="cuda")
        out = torch.zeros(2 * (F + 1) * B + 8, dtype=torch.float32, device="cuda")
        aligned = "if_fir_sub_process_device: device pointers must be aligned to one element: 8-byte (input) and 8-byte (output)"
        with pytest.raises(fir.IfFirError) as e:
            f.process_device(buf.data_ptr() + 4, out.data_ptr(), 10)
        assert said(e) == aligned
        with pytest.raises(fir.IfFirError) as e:
            f.process_device(buf.data_ptr(), out.data_ptr() + 4, 10)
        assert said(e) == aligned
        with pytest.raises(fir.IfFirError) as e:
            f.process_device(0, out.data_ptr(), 10)
        assert said(e) == "if_fir_sub_process_device: NULL device pointer"
        with pytest.raises(fir.IfFirError) as e:
            f.process_device(buf.data_ptr(), 0, 10)
        assert said(e) == "if_fir_sub_process_device: NULL device pointer"
        with pytest.raises(fir.IfFirError) as e:
            f.process_device(buf.data_ptr(), out.data_ptr(), F + 1)
        assert said(e) == "if_fir_sub_process_device: %d frames exceed ullMaxFrames %d of init" % (F + 1, F)
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
        assert said(e).startswith("if_fir_sub_process_device: the context's stream is being captured into a hipGraph")
        f.set_stream(0)
        # every refused call left the stream where it was
        tail = f.process(raw[2 * 50 * B:])
        assert same_bits(np.concatenate([head, tail]), whole)
    # a call that would carry the position past 2^64 is refused; the stream goes on and ends as an undisturbed one
    start = (1 << 64) - 100
    with fir.IfFirSub(taps, B, R, max_frames=F, dev=True) as f, fir.IfFirSub(taps, B, R, max_frames=F, dev=True) as calm:
        for c in (f, calm):
            c.set_nco(freqs_of(B, True))
            c.debug_config(position=start)
        a = f.process(raw[:2 * 60 * B])
        with pytest.raises(fir.IfFirError) as e:
            f.process(raw[:2 * 41 * B])
        assert str(e.value) == "if_fir_sub_process: frame count too large: the stream position would pass 2^64"
        assert f.frame_count(41) == 0
        b = f.process(raw[2 * 60 * B:2 * 99 * B])   # (to 2^64 - 1: a position of 2^64 itself has no representation)
        want = calm.process(raw[:2 * 99 * B])
        assert want.shape[0] == sub_ref.frame_count(start, 99, R) > 0
        assert same_bits(np.concatenate([a, b]), want)
