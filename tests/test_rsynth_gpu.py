"""The real-output polyphase synthesis bank (if_fir_rsynth_t, docs/SPEC.md §18) on the GPU against float64: §14's fold form of
tests/synth_ref.py on the Hermitian-extended frames, real part (tests/test_rsynth_host.py holds the half-size form to it at
1e-12), SPEC §18's tolerance over the whole output of a run; the int16 output, bin spans and the edge bins, the route it replaces,
stream cuts with format changes, workspace chunks, grid limits and frame positions past 2^32 bit for bit; the real-input
analysis bank's device output fed straight back against the float64 transfer formula.  Device output buffers carry a sentinel
guard behind their last value, and the guard is checked."""
import functools

import numpy as np
import pytest

import rsynth_ref
import synth_ref
from matrix_util import row_edge_taps, signal

# SPEC §18's bound over the whole output of a run: twice the worst of the float32 model of tests/rsynth_ref.py over the matrix of
# tests/test_rsynth_host.py (l2 8.62e-7 at (1024, 5, 17), max 4.00e-6 of the peak at (8192, 2730, 8192): a single term of a
# 4096-point float32 transform; the model does not stay under 5e-7 there, and neither does §14's on the extended frame)
TOL_L2 = 1.8e-6
TOL_MAX = 8.2e-6
GUARD = 64          # elements behind the last output
SENTINEL = 12345.0
SENTINEL_I16 = 12345
OUTPUT_I16 = 1     # fir.OUTPUT_I16 (include/if_fir.h)
# (M, T, L): the longest prototype at M = 128 (J = 16); a hop that divides nothing (J = 18); T one short of 8 M at L = 3 M / 4;
# T off the multiple at L = M / 2; T just past M at L = M (J = 2); a hop one short of M at M = 8192; L = 1 with J = 32; and
# J = 32 at an odd hop with T short of J L
MATRIX = ((128, 2048, 128), (128, 300, 17), (256, 2047, 192), (1024, 3067, 512), (4096, 4097, 4096), (8192, 16383, 8191),
          (256, 32, 1), (512, 7912, 255))


def stream_frames(M, T, L):
    """8 .. 40 frames: more than the history and, where a batch has several frames, batches with a ragged last one"""
    return {128: 40, 256: 40, 512: 38, 1024: 24, 4096: 12, 8192: 8}[M]


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
    X = frames_signal(oracle_mod(), frames, M // 2 + 1 - first_bin if bins is None else bins, i16)[1]
    ref = rsynth_ref.full_f64(row_edge_taps(T, L, False), X, M, L, first_bin, bins, first)
    ref.setflags(write=False)
    return ref


def run_device(torch, f, raw, pieces, formats=None, out_formats=None):
    """feed the frames of `raw` from ONE device buffer in consecutive pieces (frame counts); returns (outputs, outputs per
    piece).  With `formats` (one input format per piece, set before that piece) `raw` maps each format to the frames in that
    format: the same values in every one, one device buffer each.  With `out_formats` (one output format per piece) the
    pieces go to a float32 and an int16 buffer, each at its own place, and the result is the list of the pieces' arrays.
    sample_count is checked at every step, and the guards behind the last output after the last."""
    both = {None: raw} if formats is None else raw
    F = next(iter(both.values())).size // (2 * f.bins)
    assert all(v.size == 2 * F * f.bins for v in both.values())
    din = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in both.items()}
    L, bins = f.hop, f.bins
    o16 = bool(f._o16)
    buf32 = torch.full((F * L + GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
    buf16 = torch.full((F * L + GUARD,), SENTINEL_I16, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()   # the context works on a stream of its own
    pos = 0
    counts, kinds = [], []
    for k, s in enumerate(pieces):
        if formats is not None:
            f.set_input_format(formats[k])
        if out_formats is not None:
            f.set_output_format(out_formats[k])
            o16 = out_formats[k] == OUTPUT_I16
        src = din[None if formats is None else formats[k]]
        dst = buf16.data_ptr() + 2 * pos * L if o16 else buf32.data_ptr() + 4 * pos * L
        want = f.sample_count(s)
        got = f.process_device(src.data_ptr() + 2 * src.element_size() * pos * bins, dst, s)
        assert got == want == s * L, (pos, s, got, want)
        counts.append(got)
        kinds.append(o16)
        pos += s
    f.synchronize()
    assert pos == F
    h32, h16 = buf32.cpu().numpy(), buf16.cpu().numpy()
    assert np.all(h32[F * L:] == SENTINEL) and np.all(h16[F * L:] == SENTINEL_I16), "the guard behind the last output was written"
    if out_formats is None:
        return (h16 if o16 else h32)[:F * L].copy(), counts
    at = np.concatenate([[0], np.cumsum(counts)])
    return [(h16 if kinds[k] else h32)[at[k]:at[k + 1]].copy() for k in range(len(pieces))], counts


def check(oracle, y, ref, what):
    l2, mx = oracle.err_metrics(y, ref)
    print("rsynth %s: l2=%.3g max=%.3g" % (what, l2, mx))
    assert l2 <= TOL_L2 and mx <= TOL_MAX, (what, l2, mx)
    return l2, mx


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("i16", [False, True])
@pytest.mark.parametrize("M,T,L", MATRIX)
def test_matrix_against_float64(gpu_ok, fir, oracle, torch_cuda, M, T, L, i16):
    """taps loud at both ends of every row; the host path in two calls within tolerance of float64 over the whole output, the
    device path the same bits"""
    F = stream_frames(M, T, L)
    bins = M // 2 + 1
    raw, _ = frames_signal(oracle, F, bins, i16)
    taps = row_edge_taps(T, L, False)
    cut = F // 3 + 1
    with fir.IfFirRsynth(taps, M, L, max_frames=F) as f:
        if i16:
            f.set_input_format(fir.INPUT_I16)
        y = np.concatenate([f.process(raw[:2 * cut * bins]), f.process(raw[2 * cut * bins:])])
        f.reset()
        yd, _ = run_device(torch_cuda, f, raw, [cut, F - cut])
    ref = reference(M, T, L, i16, F)
    assert y.dtype == np.float32 and y.shape == ref.shape == (F * L,)
    check(oracle, y, ref, "matrix M=%d T=%d L=%d i16=%d" % (M, T, L, i16))
    assert same_bits(yd, y)


def test_the_matrix_has_the_shapes_of_the_issue():
    assert all(8 <= stream_frames(*c) <= 40 for c in MATRIX)
    assert {rsynth_ref.terms(T, L) for _, T, L in MATRIX} >= {2, 16, 18, 32} and any(T % L for _, T, L in MATRIX)
    assert {M for M, _, _ in MATRIX} >= {128, 256, 1024, 4096, 8192}


@pytest.mark.gpu
@pytest.mark.parametrize("M,T,L", [(256, 2047, 192), (128, 300, 17)])
def test_int16_output_is_the_float32_output_converted(gpu_ok, fir, oracle, torch_cuda, M, T, L):
    """the taps scaled so that the float32 output passes 1.25 on either side: the int16 output of the same call is SPEC §11's conversion of
    it value for value, samples saturate at both rails and most do not; on the host path and the device path, float32 and
    int16 input"""
    F = stream_frames(M, T, L)
    bins = M // 2 + 1
    for i16 in (False, True):
        raw, _ = frames_signal(oracle, F, bins, i16)
        taps = row_edge_taps(T, L, False)
        ref = reference(M, T, L, i16, F)
        with fir.IfFirRsynth(taps * np.float32(1.25 / min(ref.max(), -ref.min())), M, L, max_frames=F) as f:
            if i16:
                f.set_input_format(fir.INPUT_I16)
            y = f.process(raw)
            f.reset()
            f.set_output_format(fir.OUTPUT_I16)
            q = f.process(raw)
            f.reset()
            qd, _ = run_device(torch_cuda, f, raw, [F // 2, F - F // 2])
            with pytest.raises(fir.IfFirError, match="unknown format 2"):
                f.set_output_format(2)
        assert y.dtype == np.float32 and q.dtype == qd.dtype == np.int16
        assert y.max() > 1.0 and y.min() < -1.0 and np.mean(np.abs(y) < 1.0) > 0.5
        want = rsynth_ref.to_i16(y)
        assert want.max() == 32767 and want.min() == -32768 and np.sum(want == 32767) >= 1 and np.sum(want == -32768) >= 1
        assert np.array_equal(q, want) and same_bits(qd, q)


@pytest.mark.gpu
@pytest.mark.parametrize("M", [1024, 128])
def test_a_bin_span_is_the_full_width_call_with_zeros_elsewhere(gpu_ok, fir, oracle, torch_cuda, M):
    """spans -- all bins, channel 0 alone, channel M/2 alone, an inner span -- against the full-width call whose other channels
    hold +0: the same bits; imaginary parts on channels 0 and M/2 change no bit; the inner span against float64"""
    T, L = 3 * M - 5, M // 2
    H = M // 2
    F = stream_frames(M, T, L)
    taps = row_edge_taps(T, L, False)
    for first_bin, bins in ((0, H + 1), (0, 1), (H, 1), (H // 2 - 3, 7)):
        raw, _ = frames_signal(oracle, F, bins, False)
        full = np.zeros((F, H + 1, 2), dtype=np.float32)
        full[:, first_bin:first_bin + bins] = raw.reshape(F, bins, 2)
        with fir.IfFirRsynth(taps, M, L, first_bin=first_bin, bins=bins, max_frames=F) as f:
            y, _ = run_device(torch_cuda, f, raw, [F // 2, F - F // 2])
        with fir.IfFirRsynth(taps, M, L, max_frames=F) as f:
            want, _ = run_device(torch_cuda, f, full.reshape(-1), [F])
            assert same_bits(y, want), (first_bin, bins)
            # the same frames with the imaginary parts of channels 0 and M/2 zeroed: nothing moves
            real_edges = full.copy()
            assert np.any(real_edges[:, 0, 1]) or first_bin > 0
            real_edges[:, 0, 1] = 0
            real_edges[:, H, 1] = 0
            f.reset()
            again, _ = run_device(torch_cuda, f, real_edges.reshape(-1), [F])
            assert same_bits(again, want), (first_bin, bins)
        if bins == 7:
            check(oracle, y, reference(M, T, L, False, F, 0, first_bin, bins), "span M=%d first=%d bins=%d" % (M, first_bin, bins))


@pytest.mark.gpu
@pytest.mark.parametrize("M,T,L", [(128, 300, 17), (1024, 3067, 512)])
def test_a_frame_of_channel_0_or_channel_half_alone(gpu_ok, fir, torch_cuda, M, T, L):
    """one frame that holds 0.75 (and an imaginary part, ignored) in channel 0 and nothing else, then zero frames: the outputs
    are 0.75 h[n], each one product; in channel M/2: 0.75 (-1)^n h[n]; through a one-bin span and through the full width"""
    H, J = M // 2, rsynth_ref.terms(T, L)
    F = J + 2
    taps = row_edge_taps(T, L, False)
    want = np.zeros(F * L, dtype=np.float32)
    want[:T] = taps * np.float32(0.75)
    sign = np.where(np.arange(F * L) % 2 == 0, np.float32(1), np.float32(-1))
    for k, expect in ((0, want), (H, want * sign)):
        one = np.zeros((F, 1, 2), dtype=np.float32)
        one[0, 0] = (0.75, 0.3)
        full = np.zeros((F, H + 1, 2), dtype=np.float32)
        full[:, k:k + 1] = one
        with fir.IfFirRsynth(taps, M, L, first_bin=k, bins=1, max_frames=F) as f:
            y, _ = run_device(torch_cuda, f, one.reshape(-1), [F])
        with fir.IfFirRsynth(taps, M, L, max_frames=F) as f:
            yf, _ = run_device(torch_cuda, f, full.reshape(-1), [1, F - 1])
        assert np.array_equal(y, expect) and np.array_equal(yf, expect), k


@pytest.mark.gpu
@pytest.mark.parametrize("M,T,L", [(128, 300, 17), (1024, 3067, 512), (4096, 4097, 4096)])
def test_against_the_route_it_replaces(gpu_ok, fir, oracle, torch_cuda, M, T, L):
    """IfFirSynth fed the Hermitian extension of the same frames: its real part under the bound of float64 as this bank's
    output is, its imaginary part under 1e-6 of the peak"""
    F = stream_frames(M, T, L)
    raw, X = frames_signal(oracle, F, M // 2 + 1, False)
    taps = row_edge_taps(T, L, False)
    ext = rsynth_ref.extend(X, M).astype(np.complex64)
    with fir.IfFirSynth(taps, M, L, max_frames=F) as s:
        old = s.process(ext).view(np.complex64)
    with fir.IfFirRsynth(taps, M, L, max_frames=F) as f:
        y = f.process(raw)
    ref = reference(M, T, L, False, F)
    check(oracle, y, ref, "replaces M=%d T=%d L=%d" % (M, T, L))
    check(oracle, np.ascontiguousarray(old.real), ref, "replaced M=%d T=%d L=%d" % (M, T, L))
    peak = np.max(np.abs(ref))
    print("rsynth replaced route: max imaginary part %.3g of the peak" % (np.max(np.abs(old.imag)) / peak))
    assert np.max(np.abs(old.imag)) <= 1e-6 * peak


def ragged_pieces(F, J, rng):
    """calls of 0 and 1 frame, pieces shorter than the history, one longer, then random ones"""
    head = [0, 1, 1, 0, 2, max(J - 2, 1), 1, J + 3, 3, 0, 1]
    rest = F - sum(head)
    assert rest > 2 * J
    cuts = np.sort(rng.integers(0, rest + 1, 5))
    return head + [int(v) for v in np.diff(np.concatenate([[0], cuts, [rest]]))]


@pytest.mark.gpu
@pytest.mark.parametrize("M,T,L", [(1024, 3067, 512), (128, 300, 17)])
def test_cuts_and_format_changes_bit_for_bit(gpu_ok, fir, oracle, torch_cuda, M, T, L):
    """the frames in ragged pieces, the input format and the output format changed between them, against one call: the same
    bits, an int16 piece being SPEC §11's conversion of the float32 one (the taps scaled to a peak of 1.25)"""
    J = rsynth_ref.terms(T, L)
    F = stream_frames(M, T, L) + 3 * J + 20
    bins = M // 2 + 1
    xi, _ = frames_signal(oracle, F, bins, True)
    xf = xi.astype(np.float32) * np.float32(2.0 ** -15)
    peak = np.max(np.abs(reference(M, T, L, True, F)))
    taps = row_edge_taps(T, L, False) * np.float32(1.25 / peak)
    pieces = ragged_pieces(F, J, np.random.default_rng([M, T, L]))
    formats = [(fir.INPUT_F32, fir.INPUT_I16)[(k // 2) % 2] for k in range(len(pieces))]
    out_formats = [(fir.OUTPUT_F32, fir.OUTPUT_I16)[(k // 3) % 2] for k in range(len(pieces))]
    with fir.IfFirRsynth(taps, M, L, max_frames=F) as f:
        one, _ = run_device(torch_cuda, f, xf, [F])
        f.reset()
        got, counts = run_device(torch_cuda, f, {fir.INPUT_F32: xf, fir.INPUT_I16: xi}, pieces, formats=formats, out_formats=out_formats)
        assert counts[0] == 0 and 0 in counts[1:] and L in counts and max(counts) > L and min(c for c in counts if c) < (J - 1) * L
        at = np.concatenate([[0], np.cumsum(counts)])
        for k, piece in enumerate(got):
            want = one[at[k]:at[k + 1]]
            assert same_bits(piece, rsynth_ref.to_i16(want) if out_formats[k] == fir.OUTPUT_I16 else want), k
        f.reset()
        f.set_input_format(fir.INPUT_I16)
        f.set_output_format(fir.OUTPUT_F32)
        y, _ = run_device(torch_cuda, f, xi, [F])
        assert same_bits(y, one)
    # every cut of a short run, both pieces through the host path
    Fs = J + 3
    with fir.IfFirRsynth(taps, M, L, max_frames=Fs) as f:
        whole = f.process(xf[:2 * Fs * bins])
        for cut in range(Fs + 1):
            f.reset()
            two = np.concatenate([f.process(xf[:2 * cut * bins]), f.process(xf[2 * cut * bins:2 * Fs * bins])])
            assert same_bits(two, whole), cut


@pytest.mark.gpu
@pytest.mark.parametrize("M,T,L,F,odd", [(128, 300, 17, 35, 6), (1024, 3067, 512, 23, 5), (4096, 4097, 4096, 9, 5)])
def test_chunks_of_a_tiny_workspace_give_the_same_bits(gpu_ok, fir, oracle, torch_cuda, M, T, L, F, odd):
    """workspaces that put a chunk boundary after every frame of the call, after every J frames and after every `odd` frames (no
    multiple of a batch of 16 or 2 frames), the last chunk ragged, against the default, which holds the whole call"""
    J = rsynth_ref.terms(T, L)
    assert odd % rsynth_ref.batch(M) or rsynth_ref.batch(M) == 1
    raw, _ = frames_signal(oracle, F, M // 2 + 1, True)
    with fir.IfFirRsynth(row_edge_taps(T, L, False), M, L, max_frames=F, dev=True) as f:
        f.set_input_format(fir.INPUT_I16)
        assert f.debug_workspace() >= F
        whole, _ = run_device(torch_cuda, f, raw, [F])
        check(oracle, whole, reference(M, T, L, True, F), "chunks M=%d T=%d L=%d" % (M, T, L))
        for nbytes, per in ((1, 1), (4 * M * (2 * J - 1), J), (4 * M * (J - 1 + odd), odd)):
            assert f.debug_workspace(nbytes) == per and J > 1
            chunks = -(-F // per)
            assert -(-F // chunks) == per and (per == 1 or F % per), (F, per)   # the launcher's even split keeps that length
            f.reset()
            y, _ = run_device(torch_cuda, f, raw, [F // 2, F - F // 2])
            assert same_bits(y, whole), nbytes


@pytest.mark.gpu
@pytest.mark.parametrize("M,T,L", [(128, 300, 17), (1024, 3067, 512), (4096, 4097, 4096), (256, 32, 1)])
def test_grid_limits_give_the_same_bits(gpu_ok, fir, oracle, torch_cuda, M, T, L):
    """1, 2 and 7 workgroups walk all batches of frames and all outputs: the bits of the default launch"""
    F = stream_frames(M, T, L)
    raw, _ = frames_signal(oracle, F, M // 2 + 1, False)
    with fir.IfFirRsynth(row_edge_taps(T, L, False), M, L, max_frames=F, dev=True) as f:
        runs = []
        for limit in (0, 1, 2, 7):
            f.debug_config(grid_limit=limit)
            f.reset()
            runs.append(run_device(torch_cuda, f, raw, [F])[0])
    check(oracle, runs[0], reference(M, T, L, False, F), "grid M=%d T=%d L=%d" % (M, T, L))
    for r in runs[1:]:
        assert same_bits(r, runs[0])


@pytest.mark.gpu
@pytest.mark.parametrize("start", [(1 << 32) - 5, (1 << 40) + 12345])
@pytest.mark.parametrize("M,T,L", [(256, 2047, 255), (128, 300, 17)])
def test_frame_positions_past_2_32(gpu_ok, fir, oracle, torch_cuda, M, T, L, start):
    """through the development hook the context starts at an absolute frame index whose first output is no multiple of M, with
    a zero history: the outputs are the reference evaluated at that position; a cut (across frame 2^32 for the first start)
    gives the same bits, and position 0 gives other values"""
    assert (start * L) % M
    F = stream_frames(M, T, L)
    for i16 in (False, True):
        raw, _ = frames_signal(oracle, F, M // 2 + 1, i16)
        with fir.IfFirRsynth(row_edge_taps(T, L, False), M, L, max_frames=F, dev=True) as f:
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
@pytest.mark.parametrize("M,L,Th,Tg", [(128, 17, 4 * 128 + 3, 300), (1024, 1024, 3 * 1024 - 5, 2 * 1024 + 7), (256, 128, 700, 1000)])
def test_analysis_then_synthesis_on_the_device(gpu_ok, fir, oracle, torch_cuda, M, L, Th, Tg):
    """the frames IfFirRpfb (hop L) leaves on the device go straight into IfFirRsynth.process_device; the result against the
    real part of the float64 transfer formula of SPEC §14 under the bound"""
    import ddc_ref
    torch = torch_cuda
    n = 40 * L + 5
    F = -(-n // L)
    bins = M // 2 + 1
    r = ddc_ref.real_signal(oracle, n, False)[1]
    h, g = row_edge_taps(Th, M, False), row_edge_taps(Tg, L, False, seed=1)
    din = torch.from_numpy(np.ascontiguousarray(r)).cuda()
    mid = torch.full((2 * F * bins + GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
    out = torch.full((F * L + GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()   # the contexts work on streams of their own
    with fir.IfFirRpfb(h, M, L, max_samples=n) as a, fir.IfFirRsynth(g, M, L, max_frames=F) as s:
        assert a.process_device(din.data_ptr(), mid.data_ptr(), n) == F
        a.synchronize()
        assert s.process_device(mid.data_ptr(), out.data_ptr(), F) == F * L
        s.synchronize()
    got = out.cpu().numpy()
    assert np.all(got[F * L:] == SENTINEL) and np.all(mid.cpu().numpy()[2 * F * bins:] == SENTINEL)
    want = synth_ref.transfer_f64(h, g, r.astype(np.float64), M, L)
    assert np.max(np.abs(want.imag)) <= 1e-12 * np.max(np.abs(want.real))
    check(oracle, got[:F * L], np.ascontiguousarray(want.real), "round trip M=%d L=%d" % (M, L))


@pytest.mark.gpu
@pytest.mark.filterwarnings("ignore:The CUDA Graph is empty")
def test_refusals_leave_the_stream_where_it_was(gpu_ok, fir, oracle, torch_cuda):
    torch = torch_cuda
    M, T, L, F = 256, 700, 100, 60
    bins = M // 2 + 1
    raw, _ = frames_signal(oracle, F, bins, False)
    taps = row_edge_taps(T, L, False)
    for kw in (dict(channels=64), dict(channels=16384), dict(channels=96), dict(channels=0), dict(taps=np.ones(16 * M + 1, dtype=np.float32)),
               dict(taps=np.zeros(0, dtype=np.float32)), dict(hop=0), dict(hop=M + 1), dict(hop=21), dict(taps=np.ones(33, dtype=np.float32), hop=1),
               dict(first_bin=1, bins=bins), dict(first_bin=0, bins=bins + 1), dict(first_bin=M // 2 + 1, bins=1), dict(bins=0),
               dict(max_frames=0)):
        args = dict(taps=taps, channels=M, hop=L)
        args.update(kw)
        with pytest.raises(fir.IfFirError) as e:
            fir.IfFirRsynth(**args)
        assert "if_fir_rsynth_init" in str(e.value), kw
    with fir.IfFirRsynth(np.ones(32, dtype=np.float32), M, 1, max_frames=4):      # J = 32 is the most
        pass
    with fir.IfFirRsynth(taps, M, L, max_frames=F, dev=True) as f, fir.IfFirRsynth(taps, M, L, max_frames=F, dev=True) as calm:
        state = {"at": 0}

        def undisturbed(what):
            """after a refusal: the next frame through both contexts, the same bits"""
            k = state["at"]
            a, b = f.process(raw[2 * k * bins:2 * (k + 1) * bins]), calm.process(raw[2 * k * bins:2 * (k + 1) * bins])
            assert a.size == L and same_bits(a, b), what
            assert f.sample_count(3) == 3 * L
            state["at"] = k + 1

        undisturbed("nothing yet")
        with pytest.raises(fir.IfFirError, match="ullMaxFrames"):
            f.process(np.zeros(2 * (F + 1) * bins, dtype=np.float32))
        undisturbed("F > max")
        with pytest.raises(fir.IfFirError, match="format"):
            f.set_input_format(5)
        undisturbed("input format")
        with pytest.raises(fir.IfFirError, match="format"):
            f.set_output_format(5)
        undisturbed("output format")
        buf = torch.zeros(2 * F * bins + 8, dtype=torch.float32, device="cuda")
        out = torch.zeros(F * L + 8, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        with pytest.raises(fir.IfFirError, match="aligned"):
            f.process_device(buf.data_ptr() + 4, out.data_ptr(), 5)
        undisturbed("input alignment")
        with pytest.raises(fir.IfFirError, match="aligned"):
            f.process_device(buf.data_ptr(), out.data_ptr() + 2, 5)
        undisturbed("output alignment")
        f.set_output_format(fir.OUTPUT_I16)
        with pytest.raises(fir.IfFirError, match="aligned"):
            f.process_device(buf.data_ptr(), out.data_ptr() + 1, 5)
        f.set_output_format(fir.OUTPUT_F32)
        undisturbed("int16 output alignment")
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
        assert same_bits(f.process(raw[2 * k * bins:]), calm.process(raw[2 * k * bins:]))
    # a call that would carry the output position past 2^64 is refused; the stream goes on and ends as an undisturbed one
    start = ((1 << 64) - 1) // L - 50
    with fir.IfFirRsynth(taps, M, L, max_frames=F, dev=True) as f, fir.IfFirRsynth(taps, M, L, max_frames=F, dev=True) as calm:
        for c in (f, calm):
            c.debug_config(position=start)
        a = f.process(raw[:2 * 30 * bins])
        with pytest.raises(fir.IfFirError, match="2\\^64"):
            f.process(raw[:2 * 21 * bins])
        assert f.sample_count(21) == 0 and f.sample_count(20) == 20 * L
        b = f.process(raw[2 * 30 * bins:2 * 50 * bins])
        want = calm.process(raw[:2 * 50 * bins])
        assert want.size == 50 * L
        assert same_bits(np.concatenate([a, b]), want)
