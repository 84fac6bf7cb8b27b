"""The real-output up-converter (if_fir_duc_t, docs/SPEC.md §11) on the GPU against the float64 definition of tests/duc_ref.py,
SPEC §3 tolerance (int16 output: 1 LSB); the arithmetic order, stream cuts, tile and grid edges, output alignments, retunes and
stream positions past 2^32 bit for bit.  Every device output buffer lies between two canaries, and both are checked."""
import functools

import numpy as np
import pytest

import duc_ref
from matrix_util import row_edge_taps

TOL = 1e-6
GUARD = 64          # canary bytes in front of and behind every device output
CANARY = 0xA5
# (T, L)
MATRIX = ((1, 1), (5, 1), (17, 1), (3, 7), (24, 7), (255, 3), (255, 4), (1023, 8), (63, 64), (64, 64), (65, 64), (1537, 63), (4096, 64),
          (4096, 1))
# each row's own frequency, in the order of MATRIX
FREQS = (0.2, -0.37000001, 0.4999, 1 / 4096, -0.5, 0.123456789, -1 / 4096, 0.2, -0.37000001, 0.4999, 0.25, -0.2, 0.37000001, 1e-9)
# every row with real taps and float32 input and with complex taps and int16 input; two rows with all four combinations
CASES = [(T, L, ct, i16) for (T, L) in MATRIX for (ct, i16) in ((False, False), (True, True))] + \
        [(T, L, ct, i16) for (T, L) in ((255, 4), (63, 64)) for (ct, i16) in ((True, False), (False, True))]


@pytest.fixture(scope="module")
def torch_cuda(gpu_ok):
    import torch
    torch.cuda.set_device(0)
    return torch


def taps_for(fir, T, L, complex_taps):
    """image-rejection low-pass of gain L, cut-off 0.45 / L (complex: the shifted design).  if_bpf_design makes odd lengths >= 3:
    an even T is the design of T - 1 taps plus a last tap of an eighth of the centre tap, negated; T = 1 is a single tap."""
    odd = T if T % 2 else T - 1
    if odd < 3:
        h = np.array([1.0, 0.5] if complex_taps else [1.0], dtype=np.float32)
    elif complex_taps:
        h = fir.bpf_design_complex(odd, 0.1 / L, 0.8 / L)
    else:
        h = fir.bpf_design(odd, 0.0, 0.45 / L)
    if odd >= 3 and odd != T:
        width = 2 if complex_taps else 1
        mid = h[(odd // 2) * width:(odd // 2) * width + width]
        h = np.concatenate([h, -mid / np.float32(8)]).astype(np.float32)
    assert h.size == T * (2 if complex_taps else 1)
    return (h * np.float32(L)).astype(np.float32)


def signal(n, i16):
    """(what the context is fed, the same samples as float32 I/Q); int16 with full-scale samples"""
    import __graft_entry__ as g
    return duc_ref.signal(g.load_oracle(), n, i16)


@functools.lru_cache(maxsize=None)
def scaled_case(fir, T, L, ct, i16, n, word, loud, peak=0.9):
    """(taps, float64 reference): the row's taps scaled (in float32) so that the float64 reference of this stream and frequency
    peaks at `peak`, and the reference of those scaled taps"""
    taps = row_edge_taps(T, L, ct) if loud else taps_for(fir, T, L, ct)
    x = signal(n, i16)[1]
    first = duc_ref.duc_f64(taps, x, L, word, ct)
    taps = (taps.astype(np.float64) * (peak / np.max(np.abs(first)))).astype(np.float32)
    ref = duc_ref.duc_f64(taps, x, L, word, ct)
    taps.setflags(write=False)
    ref.setflags(write=False)
    return taps, ref


def check(y, ref, o16, what):
    """float32 output: SPEC §3's two metrics within 1e-6; int16 output: at most 1 LSB from clip(rint(ref 2^15))"""
    assert y.size == ref.size, (what, y.size, ref.size)
    if o16:
        assert y.dtype == np.int16
        lsb = int(np.max(np.abs(y.astype(np.int64) - duc_ref.to_i16(ref).astype(np.int64)))) if y.size else 0
        print("%s int16: %d LSB" % (what, lsb))
        assert lsb <= 1, (what, lsb)
        return lsb
    assert y.dtype == np.float32
    l2, mx = duc_ref.metrics(y, ref)
    print("%s float32: l2=%.3g max=%.3g" % (what, l2, mx))
    assert l2 <= TOL and mx <= TOL, (what, l2, mx)
    return l2, mx


def run_device(torch, f, raw, pieces, in_fmts=None, out_fmts=None, out_off=0, in_off=0):
    """feed `raw` in consecutive pieces from ONE device buffer per input format (raw: an array, or {format: array} with
    in_fmts, one format per piece); every piece writes a device buffer of its own, its first element out_off ELEMENTS behind
    a 256-byte boundary, between two canaries.  in_off: the input's first sample lies that many samples behind such a boundary.
    Returns the pieces' outputs (float32 or int16 arrays) joined when they are of one format, else as a list."""
    both = raw if isinstance(raw, dict) else {None: raw}
    din, n = {}, None
    for k, v in both.items():
        v = np.ascontiguousarray(v).reshape(-1)
        per = v.itemsize * 2
        n = v.size // 2
        buf = torch.zeros(in_off * per + v.nbytes + 256, dtype=torch.uint8, device="cuda")
        buf[in_off * per:in_off * per + v.nbytes] = torch.from_numpy(v.view(np.uint8)).cuda()
        assert buf.data_ptr() % 256 == 0
        din[k] = (buf, in_off * per, per)
    L = f.interpolation
    pos, outs = 0, []
    for k, s in enumerate(pieces):
        if in_fmts is not None:
            f.set_input_format(in_fmts[k])
        if out_fmts is not None:
            f.set_output_format(out_fmts[k])
        o16 = f._o16
        esz = 2 if o16 else 4
        buf, base, per = din[None if in_fmts is None else in_fmts[k]]
        want = f.out_count(s)
        assert want == s * L
        front = 256 + out_off * esz   # (the canary in front: everything up to the output's first byte)
        out = torch.full((front + want * esz + GUARD,), CANARY, dtype=torch.uint8, device="cuda")
        assert out.data_ptr() % 256 == 0
        got = f.process_device(buf.data_ptr() + base + per * pos, out.data_ptr() + front, s)
        assert got == want, (pos, s, got, want)
        f.synchronize()
        h = out.cpu().numpy()
        assert np.all(h[:front] == CANARY), "the canary in front of the output was written"
        assert np.all(h[front + want * esz:] == CANARY), "the canary behind the output was written"
        outs.append(h[front:front + want * esz].copy().view(np.int16 if o16 else np.float32))
        pos += s
    assert pos == n
    return np.concatenate(outs) if len({o.dtype for o in outs}) == 1 else outs


def host_and_device(fir, torch, T, L, ct, i16, loud, tag):
    """the row with the NCO off and at its own frequency, in both output formats: the host path in two calls within tolerance
    of float64, the device path in two other calls the same bits"""
    K, KP, Q = duc_ref.tile_shape(T, L)
    n = duc_ref.stream_len(T, L)
    raw, _ = signal(n, i16)
    freq = FREQS[MATRIX.index((T, L))]
    cut = n // 3
    ctx = None
    try:
        for fr in (0.0, freq):
            word = duc_ref.phase_word(fr)
            taps, ref = scaled_case(fir, T, L, ct, i16, n, word, loud)
            ctx = fir.IfFirDuc(taps, L, max_samples=n, complex_taps=ct, dev=True)
            assert ctx.tile_inputs() == Q
            if i16:
                ctx.set_input_format(fir.INPUT_I16)
            ctx.set_nco(fr)
            assert ctx.get_nco() == (word - (1 << 32) if word >= 1 << 31 else word) / 2.0 ** 32
            for o16 in (False, True):
                ctx.set_output_format(fir.OUTPUT_I16 if o16 else fir.OUTPUT_F32)
                ctx.reset()
                y = np.concatenate([ctx.process(raw[:2 * cut]), ctx.process(raw[2 * cut:])])
                check(y, ref, o16, "%s T=%d L=%d complex=%d i16=%d f=%r" % (tag, T, L, ct, i16, fr))
                ctx.reset()
                yd = run_device(torch, ctx, raw, [Q + 1, n - Q - 1])
                assert np.array_equal(yd, y)
            ctx.close()
    finally:
        if ctx is not None:
            ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("T,L,ct,i16", CASES)
def test_matrix_against_float64(gpu_ok, fir, torch_cuda, T, L, ct, i16):
    """designed image-rejection taps scaled to a float64 peak of 0.9; (3, 7) has phases without any tap: those outputs are 0"""
    host_and_device(fir, torch_cuda, T, L, ct, i16, False, "duc-matrix")


@pytest.mark.gpu
@pytest.mark.parametrize("T,L,ct,i16", CASES)
def test_matrix_with_loud_row_ends(gpu_ok, fir, torch_cuda, T, L, ct, i16):
    """every phase row's first and last tap are the largest of the filter (tests/test_duc_host.py: dropping one costs more
    than 1e-2); the int16 stream carries full-scale samples"""
    host_and_device(fir, torch_cuda, T, L, ct, i16, True, "duc-loud")


# (T, L): rows of 4, 8, 15 (padded to 16), 16, 17, 33, 64 and 1 phase taps, a row of 25 at L = 63, L = 1 with 127, the capped tile
ORDER_ROWS = ((16, 4), (22, 3), (45, 3), (255, 16), (51, 3), (99, 3), (255, 4), (63, 64), (1537, 63), (127, 1), (4096, 64))


@pytest.mark.gpu
@pytest.mark.parametrize("ct,i16", [(False, False), (True, True), (True, False), (False, True)])
@pytest.mark.parametrize("T,L", ORDER_ROWS)
def test_order_of_the_spec_bit_for_bit(gpu_ok, fir, torch_cuda, T, L, ct, i16):
    """With the NCO off (no table of mixed taps, no rotation) the float32 output equals, bit for bit, the float32 model of SPEC
    §11's arithmetic order (duc_ref.duc_f32_order): the two chains, the segments and the compensated joins are the ones the
    SPEC states.  Taps loud at both ends of every row, more than one tile, a cut inside the first tile."""
    K, KP, Q = duc_ref.tile_shape(T, L)
    n = min(duc_ref.stream_len(T, L), Q + 2 * K + 37)
    raw, x = signal(n, i16)
    taps = row_edge_taps(T, L, ct)
    model = duc_ref.duc_f32_order(taps, x, L, 0, ct)
    with fir.IfFirDuc(taps, L, max_samples=n, complex_taps=ct) as f:
        if i16:
            f.set_input_format(fir.INPUT_I16)
        y = run_device(torch_cuda, f, raw, [Q // 3 + 1, n - Q // 3 - 1])
    assert y.size == model.size
    differ = np.flatnonzero(y != model)
    assert differ.size == 0, (differ.size, differ[:4], y[differ[:4]], model[differ[:4]])


@pytest.mark.gpu
@pytest.mark.parametrize("T,L,ct,i16", [(255, 4, False, False), (1023, 8, True, True), (63, 64, False, True), (255, 3, True, False)])
def test_int16_is_the_rounding_of_the_float32_result(gpu_ok, fir, torch_cuda, T, L, ct, i16):
    """the int16 output equals clip(rint(float32 output 2^15)) EXACTLY, with the NCO off and on; with taps scaled to a peak of
    1.7 both rails are hit and nothing wraps"""
    n = duc_ref.stream_len(T, L)
    raw, x = signal(n, i16)
    for fr in (0.0, 0.2):
        for peak in (0.9, 1.7):
            taps, ref = scaled_case(fir, T, L, ct, i16, n, duc_ref.phase_word(fr), True, peak)
            with fir.IfFirDuc(taps, L, max_samples=n, complex_taps=ct) as f:
                if i16:
                    f.set_input_format(fir.INPUT_I16)
                f.set_nco(fr)
                y32 = run_device(torch_cuda, f, raw, [n])
                f.reset()
                f.set_output_format(fir.OUTPUT_I16)
                y16 = run_device(torch_cuda, f, raw, [n])
            assert y32.dtype == np.float32 and y16.dtype == np.int16
            assert np.array_equal(y16, duc_ref.to_i16(y32)), (fr, peak)
            check(y32, ref, False, "duc-int16 T=%d L=%d f=%r peak=%r" % (T, L, fr, peak))
            if peak > 1:
                clipped = np.abs(ref) >= 1.0
                assert y16.max() == 32767 and y16.min() == -32768 and clipped.sum() > 10
                assert np.all(y16[ref >= 1.0] == 32767) and np.all(y16[ref < -1.0] == -32768)   # nothing wraps
            else:
                check(y16, ref, True, "duc-int16 T=%d L=%d f=%r" % (T, L, fr))


@pytest.mark.gpu
@pytest.mark.parametrize("ct,i16", [(False, False), (True, True)])
@pytest.mark.parametrize("T,L", [(255, 4), (1023, 8), (4096, 64), (1537, 63)])
def test_pieces_around_the_history(gpu_ok, fir, torch_cuda, T, L, ct, i16):
    """calls of 1, 2, 0, K - 1, K, L and 4097 inputs, then the rest: in the short ones the first workgroup builds the next
    history from the old history and the call.  Bit for bit the one-call run, which meets float64.  Then the int16-valued
    stream with the input format switched mid-stream and the output format switched at every cut: the float32 pieces are the
    one-call bits, the int16 pieces their rounding."""
    K, KP, Q = duc_ref.tile_shape(T, L)
    head = [1, 2, 0, K - 1, K, L, 4097]
    n = max(duc_ref.stream_len(T, L), sum(head) + Q + 17)
    raw, _ = signal(n, i16)
    xi, xf = signal(n, True)
    freq = -0.37000001
    taps, ref = scaled_case(fir, T, L, ct, i16, n, duc_ref.phase_word(freq), True)
    with fir.IfFirDuc(taps, L, max_samples=n, complex_taps=ct) as f:
        f.set_nco(freq)
        if i16:
            f.set_input_format(fir.INPUT_I16)
        one = run_device(torch_cuda, f, raw, [n])
        check(one, ref, False, "duc-pieces T=%d L=%d complex=%d i16=%d" % (T, L, ct, i16))
        f.reset()
        y = run_device(torch_cuda, f, raw, head + [n - sum(head)])
        assert np.array_equal(y, one)
        if not i16:   # (the int16 values as float32: the stream the mixed run carries)
            f.reset()
            one = run_device(torch_cuda, f, xf, [n])
        pieces = [Q // 2 + 1, 0, K + 1, L, n - Q // 2 - K - L - 2]
        assert min(pieces) >= 0 and sum(pieces) == n
        f.reset()
        F32, I16, O32, O16 = fir.INPUT_F32, fir.INPUT_I16, fir.OUTPUT_F32, fir.OUTPUT_I16
        outs = run_device(torch_cuda, f, {F32: xf, I16: xi}, pieces, in_fmts=[F32, F32, I16, I16, F32],
                          out_fmts=[O32, O16, O16, O32, O16])
        at = 0
        for s, fmt, got in zip(pieces, [O32, O16, O16, O32, O16], outs):
            want = one[at * L:(at + s) * L]
            assert np.array_equal(got, duc_ref.to_i16(want) if fmt == O16 else want), (at, s, fmt)
            at += s


# (T, L, complex taps, int16 input)
TILE_EDGES = [pytest.param(255, 4, False, False, id="255-4"), pytest.param(1023, 8, True, True, id="1023-8-complex-i16"),
              pytest.param(100, 3, False, True, id="100-3-i16"), pytest.param(4096, 64, False, False, id="4096-64"),
              pytest.param(255, 17, True, False, id="255-17-complex")]


@pytest.mark.gpu
@pytest.mark.parametrize("T,L,ct,i16", TILE_EDGES)
def test_tile_and_grid_edges(gpu_ok, fir, torch_cuda, T, L, ct, i16):
    """input counts one less than, equal to and one more than 1 tile and 5 tiles; the grid capped to 1 and to 3 workgroups
    gives the bits of the uncapped run, in both output formats"""
    taps0 = row_edge_taps(T, L, ct)
    freq = 0.2
    Q = duc_ref.tile_shape(T, L)[2]
    n_max = 5 * Q + 1
    raw, x = signal(n_max, i16)
    first = duc_ref.duc_f64(taps0, x, L, duc_ref.phase_word(freq), ct)
    taps = (taps0.astype(np.float64) * (0.9 / np.max(np.abs(first)))).astype(np.float32)
    ref_all = duc_ref.duc_f64(taps, x, L, duc_ref.phase_word(freq), ct)
    with fir.IfFirDuc(taps, L, max_samples=n_max, complex_taps=ct, dev=True) as f:
        f.set_nco(freq)
        if i16:
            f.set_input_format(fir.INPUT_I16)
        assert f.tile_inputs() == Q
        for n in (Q - 1, Q, Q + 1, 5 * Q - 1, 5 * Q, 5 * Q + 1):
            for o16 in (False, True):
                f.set_output_format(fir.OUTPUT_I16 if o16 else fir.OUTPUT_F32)
                runs = []
                for limit in (0, 1, 3):
                    f.debug_config(grid_limit=limit)
                    f.reset()
                    runs.append(run_device(torch_cuda, f, raw[:2 * n], [n]))
                assert np.array_equal(runs[0], runs[1]) and np.array_equal(runs[0], runs[2]), n
                check(runs[0], ref_all[:n * L], o16, "duc-edges T=%d L=%d n=%d" % (T, L, n))


@pytest.mark.gpu
@pytest.mark.parametrize("T,L,ct,i16", [(255, 3, False, False), (255, 4, True, True), (63, 64, False, True)])
def test_output_alignment(gpu_ok, fir, torch_cuda, T, L, ct, i16):
    """the output pointer at element offsets 0, 1, 2 and 3 behind a 256-byte boundary, both formats, an odd and an even count:
    the bits of offset 0, the canaries on both sides intact (run_device checks them); the input pointer at an odd element offset"""
    Q = duc_ref.tile_shape(T, L)[2]
    taps = None
    for n in (Q + 5, Q + 6):
        raw, x = signal(n, i16)
        if taps is None:
            first = duc_ref.duc_f64(row_edge_taps(T, L, ct), x, L, duc_ref.phase_word(0.2), ct)
            taps = (row_edge_taps(T, L, ct).astype(np.float64) * (0.9 / np.max(np.abs(first)))).astype(np.float32)
        ref = duc_ref.duc_f64(taps, x, L, duc_ref.phase_word(0.2), ct)
        with fir.IfFirDuc(taps, L, max_samples=n, complex_taps=ct) as f:
            f.set_nco(0.2)
            if i16:
                f.set_input_format(fir.INPUT_I16)
            for o16 in (False, True):
                f.set_output_format(fir.OUTPUT_I16 if o16 else fir.OUTPUT_F32)
                runs = []
                for off, in_off in ((0, 0), (1, 0), (2, 1), (3, 3)):
                    f.reset()
                    runs.append(run_device(torch_cuda, f, raw, [Q // 2 + 1, n - Q // 2 - 1], out_off=off, in_off=in_off))
                check(runs[0], ref, o16, "duc-align T=%d L=%d n=%d" % (T, L, n))
                for r in runs[1:]:
                    assert np.array_equal(r, runs[0])


@pytest.mark.gpu
@pytest.mark.parametrize("T,L,ct,i16", [(255, 4, False, False), (1023, 8, True, True), (63, 64, False, True)])
def test_retune_is_as_if_set_since_the_reset(gpu_ok, fir, torch_cuda, T, L, ct, i16):
    """feed a, set_nco(f2), feed b: the outputs of b are, bit for bit, those of a fresh context at f2 fed a || b; get_nco
    returns the quantised value"""
    n = duc_ref.stream_len(T, L)
    cut = n // 3 + 1
    f1, f2 = 0.2, -0.37000001
    raw, x = signal(n, i16)
    taps = row_edge_taps(T, L, ct)
    with fir.IfFirDuc(taps, L, max_samples=n, complex_taps=ct) as f, fir.IfFirDuc(taps, L, max_samples=n, complex_taps=ct) as fresh:
        for c in (f, fresh):
            if i16:
                c.set_input_format(fir.INPUT_I16)
        assert f.get_nco() == 0.0
        f.set_nco(f1)
        assert f.get_nco() == round(f1 * 2 ** 32) / 2.0 ** 32 != f1
        ya = f.process(raw[:2 * cut])
        f.set_nco(f2)
        assert f.get_nco() == round(f2 * 2 ** 32) / 2.0 ** 32
        yb = f.process(raw[2 * cut:])
        fresh.set_nco(f2)
        whole = fresh.process(raw)
        assert np.array_equal(yb, whole[ya.size:])
        assert not np.array_equal(ya, whole[:ya.size])
        check(whole, duc_ref.duc_f64(taps, x, L, duc_ref.phase_word(f2), ct), False, "duc-retune f2")
        check(ya, duc_ref.duc_f64(taps, x[:2 * cut], L, duc_ref.phase_word(f1), ct), False, "duc-retune f1")


@pytest.mark.gpu
@pytest.mark.parametrize("L", [3, 64])
@pytest.mark.parametrize("start", [(1 << 32) - 1000, (1 << 40) + 3])
def test_stream_positions_past_2_32(gpu_ok, fir, torch_cuda, L, start):
    """through the development hook the context starts at an absolute input index near 2^32 and past 2^40 with a zero history:
    the outputs are the definition evaluated with that offset (every sample's phase comes from the 64-bit index), and a cut
    across 2^32 gives the bits of the uncut run; a call whose (c + N) L would pass 2^64 is refused and changes nothing"""
    T, freq = 255, 0.123456789
    n = max(duc_ref.stream_len(T, L), 1500)   # (2^32 - 1000 + n passes 2^32)
    for ct, i16 in ((False, False), (True, True)):
        raw, x = signal(n, i16)
        taps = row_edge_taps(T, L, ct)
        ref = duc_ref.duc_f64(taps, x, L, duc_ref.phase_word(freq), ct, first=start)
        with fir.IfFirDuc(taps, L, max_samples=n, complex_taps=ct, dev=True) as f:
            f.set_nco(freq)
            if i16:
                f.set_input_format(fir.INPUT_I16)
            f.debug_config(position=start)
            one = run_device(torch_cuda, f, raw, [n])
            check(one, ref, False, "duc-position L=%d start=%d complex=%d i16=%d" % (L, start, ct, i16))
            f.debug_config(position=start)
            y = run_device(torch_cuda, f, raw, [997, 5, 1, n - 1003])   # 2^32 lies inside the second piece
            assert np.array_equal(y, one)
            # the position is not the index modulo 2^32: from 0 the same samples give other outputs
            f.reset()
            zero = run_device(torch_cuda, f, raw, [n])
            assert not np.array_equal(zero, one)
            # (c + N) L past 2^64
            limit = ((1 << 64) - 1) // L
            f.debug_config(position=limit - 10)
            assert f.out_count(10) == 10 * L and f.out_count(11) == 0
            with pytest.raises(fir.IfFirError, match="2\\^64"):
                f.process(raw[:2 * 11])
            assert f.process(raw[:2 * 10]).size == 10 * L
            f.reset()
            assert np.array_equal(run_device(torch_cuda, f, raw, [n]), zero)


@pytest.mark.gpu
@pytest.mark.parametrize("T,L", [(255, 4), (255, 3)])
def test_against_the_interpolator_chain(gpu_ok, fir, T, L):
    """what users do today: IfFirInterp with the same NCO, then the real part -- both within SPEC §3 of float64 (another
    route: not the same bits)"""
    n, freq = 5000, 0.2
    _, x = signal(n, False)
    taps = taps_for(fir, T, L, False)
    ref = duc_ref.duc_f64(taps, x, L, duc_ref.phase_word(freq))
    with fir.IfFirDuc(taps, L, max_samples=n) as f:
        f.set_nco(freq)
        y = f.process(x)
    with fir.IfFirInterp(taps, L, max_samples=n) as chain:
        chain.set_nco(freq)
        wide = chain.process(x)[0::2]
    for name, got in (("up-converter", y), ("chain", np.ascontiguousarray(wide))):
        check(got, ref, False, "duc-chain T=%d L=%d %s" % (T, L, name))


@pytest.mark.gpu
def test_degenerate_calls(gpu_ok, fir):
    T, L, n = 100, 64, 300
    _, x = signal(n, False)
    with fir.IfFirDuc(taps_for(fir, T, L, False), L, max_samples=n) as f:
        f.set_nco(0.2)
        one = f.process(x)
        assert one.size == n * L and one.dtype == np.float32
        f.reset()
        assert f.process(x[:0]).size == 0 and f.out_count(0) == 0 and f.out_count(7) == 7 * L
        parts = [f.process(x[2 * i:2 * i + 2]) for i in range(n)]
        assert np.array_equal(np.concatenate(parts), one)
        f.reset()
        f.set_output_format(fir.OUTPUT_I16)
        y16 = f.process(x)
        assert y16.dtype == np.int16 and np.array_equal(y16, duc_ref.to_i16(one))


@pytest.mark.gpu
@pytest.mark.filterwarnings("ignore:The CUDA Graph is empty")
def test_reset_and_rejected_arguments(gpu_ok, fir, torch_cuda):
    torch = torch_cuda
    n, L = 3000, 4
    _, x = signal(n, False)
    taps = taps_for(fir, 95, L, False)
    with fir.IfFirDuc(taps, L, max_samples=n) as f:
        f.set_nco(0.2)
        y0 = f.process(x)
        f.process(x[:2 * 1001])
        f.reset()
        assert f.get_nco() == round(0.2 * 2 ** 32) / 2.0 ** 32   # a reset keeps the frequency
        assert np.array_equal(f.process(x), y0)
        f.reset()
        f.process(x[:2 * 1001])
        with pytest.raises(fir.IfFirError, match="ullMaxSamples"):
            f.process(np.zeros(2 * (n + 1), dtype=np.float32))
        with pytest.raises(fir.IfFirError, match="format"):
            f.set_input_format(5)
        with pytest.raises(fir.IfFirError, match="format"):
            f.set_output_format(2)
        for bad in (0.5000001, -0.6, float("nan"), float("inf")):
            with pytest.raises(fir.IfFirError, match="0.5"):
                f.set_nco(bad)
        buf = torch.zeros(2 * n * L + 8, dtype=torch.float32, device="cuda")
        with pytest.raises(fir.IfFirError, match="aligned"):
            f.process_device(buf.data_ptr() + 4, buf.data_ptr(), 100)      # float32 pairs: 8 bytes
        with pytest.raises(fir.IfFirError, match="aligned"):
            f.process_device(buf.data_ptr(), buf.data_ptr() + 2, 100)      # float32 output: 4 bytes
        with pytest.raises(fir.IfFirError, match="NULL"):
            f.process_device(0, buf.data_ptr(), 100)
        with pytest.raises(fir.IfFirError, match="NULL"):
            f.process_device(buf.data_ptr(), 0, 100)
        assert f.process_device(0, 0, 0) == 0                              # N = 0: legal, nothing is read
        f.set_input_format(fir.INPUT_I16)
        f.set_output_format(fir.OUTPUT_I16)
        with pytest.raises(fir.IfFirError, match="aligned"):
            f.process_device(buf.data_ptr() + 2, buf.data_ptr(), 100)      # int16 pairs: 4 bytes
        with pytest.raises(fir.IfFirError, match="aligned"):
            f.process_device(buf.data_ptr(), buf.data_ptr() + 1, 100)      # int16 output: 2 bytes
        f.set_input_format(fir.INPUT_F32)
        f.set_output_format(fir.OUTPUT_F32)
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
        assert np.array_equal(f.process(x[2 * 1001:]), y0[1001 * L:])
    for T, up in ((0, 4), (4097, 4), (31, 0), (31, 65)):
        with pytest.raises(fir.IfFirError) as e:
            fir.IfFirDuc(np.ones(T, dtype=np.float32), up)
        assert str(e.value)
    with pytest.raises(fir.IfFirError, match="finite"):
        fir.IfFirDuc(np.array([1.0, np.nan, 0.5], dtype=np.float32), 2)


@pytest.mark.gpu
def test_random_configurations_against_float64(gpu_ok, fir, torch_cuda):
    """20 seeded draws: T log-uniform in 1..4096, L uniform in 1..64, complex taps, both formats and the frequency drawn per
    case, taps loud at both ends of every phase row and scaled to a float64 peak of 0.9, the stream of duc_ref.stream_len, 2 to
    6 pieces with one of 0 samples.  Every draw meets float64 (float32 output: SPEC §3; int16: 1 LSB), and its pieces give the
    bits of the single call."""
    rng = np.random.default_rng(20261019)
    worst = {"l2": (0.0, None), "max": (0.0, None), "lsb": (0, None)}
    for draw in range(20):
        L = int(rng.integers(1, 65))
        T = min(4096, max(1, int(round(np.exp(rng.uniform(0.0, np.log(4096.0)))))))
        ct, i16, o16 = bool(rng.integers(2)), bool(rng.integers(2)), bool(rng.integers(2))
        freq = (0.0, 0.2, 1 / 4096, float(rng.uniform(-0.5, 0.5)), float(rng.uniform(-0.5, 0.5)))[int(rng.integers(5))]
        n = duc_ref.stream_len(T, L)
        cuts = np.sort(rng.choice(np.arange(1, n), int(rng.integers(2, 7)) - 2, replace=False))
        pieces = [int(v) for v in np.diff(np.concatenate([[0], cuts, [n]]))]
        pieces.insert(int(rng.integers(len(pieces) + 1)), 0)
        case = "draw %d: T=%d L=%d complex=%d i16=%d o16=%d f=%r n=%d pieces=%s" % (draw, T, L, ct, i16, o16, freq, n, pieces)
        assert 2 <= len(pieces) <= 6 and sum(pieces) == n, case
        raw, x = signal(n, i16)
        word = duc_ref.phase_word(freq)
        taps = row_edge_taps(T, L, ct, seed=draw)
        taps = (taps.astype(np.float64) * (0.9 / np.max(np.abs(duc_ref.duc_f64(taps, x, L, word, ct))))).astype(np.float32)
        ref = duc_ref.duc_f64(taps, x, L, word, ct)
        with fir.IfFirDuc(taps, L, max_samples=n, complex_taps=ct) as f:
            f.set_nco(freq)
            if i16:
                f.set_input_format(fir.INPUT_I16)
            if o16:
                f.set_output_format(fir.OUTPUT_I16)
            one = run_device(torch_cuda, f, raw, [n])
            f.reset()
            y = run_device(torch_cuda, f, raw, pieces)
        got = check(one, ref, o16, case)
        for name, v in (("lsb", got),) if o16 else (("l2", got[0]), ("max", got[1])):
            if v > worst[name][0]:
                worst[name] = (v, case)
        assert np.array_equal(y, one), case
    for name in ("l2", "max", "lsb"):
        print("duc-random worst %s=%.3g at %s" % (name, worst[name][0], worst[name][1]))
