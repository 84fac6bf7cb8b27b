"""The corner turn (if_fir_turn_t, docs/SPEC.md §20) on the GPU.  The stage has no arithmetic but the format conversion, so
every check is on bits: byte equality of whole device buffers -- the guard band in front, the data, the rows' tails and the
guard band behind, all filled with a canary before the call -- against an image built from tests/turn_ref.py, or torch.equal on
integer views.  Every test goes through process_device unless it says otherwise."""
import functools

import numpy as np
import pytest

import turn_ref
from turn_ref import TO_FRAMES, TO_STREAMS

GUARD = 64              # elements in front of and behind every buffer (a multiple of 16 bytes in either format)
CANARY = 0xA5           # every byte outside what a call may write


@pytest.fixture(scope="module")
def torch_cuda(gpu_ok):
    import torch
    torch.cuda.set_device(0)
    return torch


def esz(i16):
    return 4 if i16 else 8


def edt(i16):
    return np.int16 if i16 else np.float32


@functools.lru_cache(maxsize=None)
def elements(shape, i16, seed):
    """seeded input elements, computed once and left unchanged"""
    x = turn_ref.make_elements(shape, i16, seed)
    x.setflags(write=False)
    return x


class Buffer:
    """a device buffer of n elements of 8 or 4 bytes between two guard bands, its first element `off` elements past a 16-byte
    boundary; host images of it are uint8 arrays of the whole allocation"""

    def __init__(self, torch, n, i16, off=0):
        self.torch, self.n, self.e, self.off = torch, n, esz(i16), off
        self.lo = (GUARD + off) * self.e
        self.t = torch.full(((2 * GUARD + off + n) * self.e,), CANARY, dtype=torch.uint8, device="cuda")
        assert self.t.data_ptr() % 16 == 0
        self.ptr = self.t.data_ptr() + self.lo

    def image(self):
        """the host image of an untouched buffer"""
        return np.full(self.t.numel(), CANARY, dtype=np.uint8)

    def put(self, img):
        self.t.copy_(self.torch.from_numpy(img))

    def get(self):
        return self.t.cpu().numpy()

    def span(self, img, first, count):
        """the bytes of elements [first, first + count) inside a host image"""
        return img[self.lo + first * self.e: self.lo + (first + count) * self.e]


def rows_image(buf, rows, P):
    """rows (C, F, 2) laid out at pitch P in an image of buf: tails and guards keep the canary"""
    img = buf.image()
    C, F = rows.shape[:2]
    for c in range(C):
        buf.span(img, c * P, F)[:] = np.ascontiguousarray(rows[c]).view(np.uint8).reshape(-1)
    return img


def flat_image(buf, x):
    img = buf.image()
    buf.span(img, 0, x.size // 2)[:] = np.ascontiguousarray(x).view(np.uint8).reshape(-1)
    return img


def make(fir, direction, B, sel, i16=False, o16=False, max_frames=4096, dev=False):
    return fir.IfFirTurn(direction, B, sel=sel, input_format=fir.INPUT_I16 if i16 else fir.INPUT_F32,
                         output_format=fir.OUTPUT_I16 if o16 else fir.OUTPUT_F32, max_frames=max_frames, dev=dev)


def run_streams(torch, t, frames, P, o16, off=0, cuts=None):
    """TO_STREAMS of frames (F, B, 2) at pitch P in the calls `cuts` (frame counts; default one call); returns (the output
    buffer's bytes, the image turn_ref wants)"""
    F, B = frames.shape[:2]
    C, i16 = t.channels, frames.dtype == np.int16
    src, dst = Buffer(torch, F * B, i16, off), Buffer(torch, C * P, o16, off)
    src.put(flat_image(src, frames))
    torch.cuda.synchronize()            # the buffers are filled on torch's stream, the context works on its own
    a = 0
    for n in cuts or [F]:
        t.process_device(src.ptr + a * B * src.e, dst.ptr + a * dst.e, n, P)
        a += n
    assert a == F
    t.synchronize()
    return dst.get(), rows_image(dst, turn_ref.to_streams(frames, t.sel, o16), P)


def run_frames(torch, t, rows, P, o16, off=0, cuts=None):
    """TO_FRAMES of rows (C, F, 2) lying at pitch P"""
    C, F = rows.shape[:2]
    B, i16 = t.bins, rows.dtype == np.int16
    src, dst = Buffer(torch, C * P, i16, off), Buffer(torch, F * B, o16, off)
    src.put(rows_image(src, rows, P))
    torch.cuda.synchronize()
    a = 0
    for n in cuts or [F]:
        t.process_device(src.ptr + a * src.e, dst.ptr + a * B * dst.e, n, P)
        a += n
    assert a == F
    t.synchronize()
    return dst.get(), flat_image(dst, turn_ref.to_frames(rows, t.sel, B, o16))


def run(torch, t, direction, F, P, i16, o16, seed=0, off=0, cuts=None):
    if direction == TO_STREAMS:
        return run_streams(torch, t, elements((F, t.bins), i16, seed), P, o16, off, cuts)
    return run_frames(torch, t, elements((t.channels, F), i16, seed), P, o16, off, cuts)


def same(got, want):
    d = np.flatnonzero(got != want)
    if d.size:
        print("turn: %d of %d bytes differ, the first at byte %d (got %02x, wanted %02x)" % (d.size, got.size, d[0], got[d[0]], want[d[0]]))
    return got.shape == want.shape and d.size == 0


def thinned_matrix():
    """every B of the edge set with every C it admits (and C = B); F, the selection and the pitch's excess over F turn through
    their sets as the list goes, so that every value meets several shapes"""
    cases, k = [], 0
    for B in turn_ref.BINS:
        for C in sorted({c for c in turn_ref.CHANNELS if c <= B} | {B}):
            F = turn_ref.FRAMES[(k * 4 + 1) % len(turn_ref.FRAMES)]
            if F * B > 129 * 8192:      # keep a case within a few seconds: the largest frames meet the frame counts up to 129
                F = (129, 65, 127, 64, 63)[k % 5]
            cases.append((B, C, F, turn_ref.SELECTIONS[k % 4], (0, 1, 37)[k % 3]))
            k += 1
    return cases


MATRIX = thinned_matrix()


def test_matrix_covers_the_edge_sets():
    assert {c[0] for c in MATRIX} == set(turn_ref.BINS) and {c[1] for c in MATRIX} >= set(turn_ref.CHANNELS)
    assert {c[2] for c in MATRIX} == set(turn_ref.FRAMES) and {c[3] for c in MATRIX} == set(turn_ref.SELECTIONS)
    assert {c[4] for c in MATRIX} == {0, 1, 37} and any(c[0] == c[1] == 8192 for c in MATRIX)


@pytest.mark.gpu
@pytest.mark.parametrize("direction", [TO_STREAMS, TO_FRAMES])
@pytest.mark.parametrize("B,C,F,kind,extra", MATRIX)
def test_matrix_bit_for_bit(gpu_ok, fir, torch_cuda, B, C, F, kind, extra, direction):
    """the four format pairs on one context (the setters take effect from the next call): data, row tails and guards"""
    sel = turn_ref.selection(kind, B, C)
    with make(fir, direction, B, sel, max_frames=max(F, 1)) as t:
        for i16, o16 in turn_ref.FORMATS:
            t.set_input_format(fir.INPUT_I16 if i16 else fir.INPUT_F32)
            t.set_output_format(fir.OUTPUT_I16 if o16 else fir.OUTPUT_F32)
            got, want = run(torch_cuda, t, direction, F, F + extra, i16, o16, seed=B + C)
            assert same(got, want), (i16, o16)


@pytest.mark.gpu
@pytest.mark.parametrize("direction", [TO_STREAMS, TO_FRAMES])
def test_the_span_form_equals_the_list_form(gpu_ok, fir, torch_cuda, direction):
    """pulSel NULL with ulFirst = 5 against the same bins listed"""
    B, C, F = 200, 70, 65
    with fir.IfFirTurn(direction, B, channels=C, first=5, max_frames=F) as t:
        assert t.sel == list(range(5, 75))
        got, want = run(torch_cuda, t, direction, F, F + 1, False, False)
        assert same(got, want)


@pytest.mark.gpu
@pytest.mark.parametrize("i16,o16", turn_ref.FORMATS)
@pytest.mark.parametrize("direction", [TO_STREAMS, TO_FRAMES])
@pytest.mark.parametrize("B,C,F", [(65, 3, 129), (918, 65, 127), (64, 64, 65)])
def test_pointers_one_element_off_the_16_byte_grid(gpu_ok, fir, torch_cuda, B, C, F, direction, i16, o16):
    """input and output pointers one element past a 16-byte boundary and an odd pitch: every row starts off the grid"""
    P = F + 2 if F % 2 else F + 1
    assert P % 2 == 1
    with make(fir, direction, B, turn_ref.selection("scattered", B, C), i16, o16, max_frames=F) as t:
        got, want = run(torch_cuda, t, direction, F, P, i16, o16, off=1)
        assert same(got, want)


@pytest.mark.gpu
@pytest.mark.parametrize("direction", [TO_STREAMS, TO_FRAMES])
def test_special_values(gpu_ok, fir, torch_cuda, direction):
    """NaNs with payloads, infinities, -0, denormals, the saturation edges and ties in every bin and at every frame: float32 to
    float32 returns the input bits, float32 to int16 follows the rule (NaN 0, infinities saturate, ties to even)"""
    B, C = 70, 9
    sel = turn_ref.selection("straddle", B, C)
    sp = turn_ref.special_f32()
    F = sp.size + 3
    shape = (F, B) if direction == TO_STREAMS else (C, F)
    x = np.array(elements(shape, False, 5))
    # every special value as a real part and, shifted by one, as an imaginary part along the frame axis of every column
    col = np.stack([np.resize(sp, F), np.resize(np.roll(sp, 1), F)], axis=-1)
    if direction == TO_STREAMS:
        x[:, :, :] = col[:, None, :]
    else:
        x[:, :, :] = col[None, :, :]
    assert np.isnan(x).any() and np.isinf(x).any() and np.signbit(x[x == 0]).any()
    for o16 in (False, True):
        with make(fir, direction, B, sel, False, o16, max_frames=F) as t:
            if direction == TO_STREAMS:
                got, want = run_streams(torch_cuda, t, x, F + 1, o16)
            else:
                got, want = run_frames(torch_cuda, t, x, F + 1, o16)
            assert same(got, want), o16
    # what the reference says here, spelled out for the int16 side
    q = np.float32(2.0 ** -15)
    assert list(turn_ref.to_i16(np.array([np.nan, np.inf, -np.inf, 32767.5 * q, -32767.5 * q, 0.5 * q, 1.5 * q, -2.5 * q], dtype=np.float32))) == \
        [0, 32767, -32768, 32767, -32768, 0, 2, -2]


@pytest.mark.gpu
@pytest.mark.parametrize("direction", [TO_STREAMS, TO_FRAMES])
@pytest.mark.parametrize("B,C,F", [(918, 200, 129), (65, 2, 1000), (4097, 64, 127)])
def test_grid_limits(gpu_ok, fir, torch_cuda, B, C, F, direction):
    """1 and 3 workgroups walk the tiles in the stride loop: the same bytes as the launcher's own grid"""
    sel = turn_ref.selection("straddle", B, C)
    with make(fir, direction, B, sel, False, True, max_frames=F, dev=True) as t:
        free, want = run(torch_cuda, t, direction, F, F + 37, False, True)
        assert same(free, want)
        for limit in (1, 3):
            t.debug_config(grid_limit=limit)
            got, _ = run(torch_cuda, t, direction, F, F + 37, False, True)
            assert same(got, free), limit


@pytest.mark.gpu
@pytest.mark.parametrize("direction", [TO_STREAMS, TO_FRAMES])
@pytest.mark.parametrize("B,C,F", [(65, 3, 131), (918, 65, 197)])
def test_stream_cuts_and_a_format_change(gpu_ok, fir, torch_cuda, B, C, F, direction):
    """one call == two == three calls with the pointers advanced by hand, calls of 0 and of 1 frame among them; then the
    output format changed between two calls: each piece has its format's bytes"""
    sel = turn_ref.selection("scattered", B, C)
    P = F + 2
    with make(fir, direction, B, sel, True, False, max_frames=F) as t:
        one, want = run(torch_cuda, t, direction, F, P, True, False)
        assert same(one, want)
        for cuts in ([63, F - 63], [0, 1, F - 1], [F - 1, 1, 0], [65, 0, F - 65], [1, 64, F - 65]):
            got, _ = run(torch_cuda, t, direction, F, P, True, False, cuts=cuts)
            assert same(got, one), cuts
    # float32 in; the first 70 frames go out as float32, the rest as int16, into two buffers: each equals its own one-format run
    torch = torch_cuda
    shape = (F, B) if direction == TO_STREAMS else (C, F)
    x = elements(shape, False, 9)
    head = x[:70] if direction == TO_STREAMS else x[:, :70]
    tail = x[70:] if direction == TO_STREAMS else x[:, 70:]
    with make(fir, direction, B, sel, False, False, max_frames=F) as t:
        runner = run_streams if direction == TO_STREAMS else run_frames
        got, want = runner(torch, t, head, P, False)
        assert same(got, want)
        t.set_output_format(fir.OUTPUT_I16)
        got, want = runner(torch, t, tail, P, True)
        assert same(got, want)
        t.set_input_format(fir.INPUT_I16)
        xi = elements(shape, True, 9)
        got, want = runner(torch, t, xi[70:] if direction == TO_STREAMS else xi[:, 70:], P, True)
        assert same(got, want)


@pytest.mark.gpu
@pytest.mark.parametrize("direction", [TO_STREAMS, TO_FRAMES])
@pytest.mark.parametrize("B,C,F,i16,o16", [(65, 3, 129, False, False), (918, 200, 65, True, False), (64, 64, 127, False, True)])
def test_host_entry_point_equals_the_device_one(gpu_ok, fir, torch_cuda, B, C, F, i16, o16, direction):
    """if_fir_turn_process with a pitch on the host rows: the same elements as process_device, the host tails untouched"""
    sel = turn_ref.selection("reversed", B, C)
    P = F + 5
    with make(fir, direction, B, sel, i16, o16, max_frames=F) as t:
        got, want = run(torch_cuda, t, direction, F, P, i16, o16, seed=3)
        assert same(got, want)
        if direction == TO_STREAMS:
            frames = elements((F, B), i16, 3)
            out = t.process(frames, pitch=P)
            assert out.shape == (C, P, 2) and turn_ref.same_bits(out[:, :F], turn_ref.to_streams(frames, sel, o16))
            assert not out[:, F:].any()                       # the binding's zeros: the call left the tails alone
        else:
            rows = elements((C, F), i16, 3)
            padded = np.full((C, P, 2), 77, dtype=rows.dtype)
            padded[:, :F] = rows
            out = t.process(padded, frames=F)
            assert turn_ref.same_bits(out, turn_ref.to_frames(rows, sel, B, o16))
        assert t.process(np.zeros((0, 2), dtype=edt(i16))).size == 0          # F = 0 on the host path


@pytest.mark.gpu
def test_refusals_word_for_word(gpu_ok, fir, torch_cuda):
    torch = torch_cuda
    B, C, F = 65, 3, 64
    sel = [5, 64, 7]
    who = "if_fir_turn_process_device: "
    src, dst = Buffer(torch, (F + 1) * B, False), Buffer(torch, C * (F + 1), False)
    torch.cuda.synchronize()
    with make(fir, TO_STREAMS, B, sel, max_frames=F) as t:
        before = dst.get()
        with pytest.raises(fir.IfFirError) as e:
            t.process_device(src.ptr, dst.ptr, 8, 7)
        assert str(e.value) == who + "a row pitch of 7 elements is below the call's 8 frames"
        with pytest.raises(fir.IfFirError) as e:
            t.process_device(src.ptr, dst.ptr, 8, 2 ** 40 + 1)
        assert str(e.value) == who + "a row pitch of 1099511627777 elements is above 2^40"
        with pytest.raises(fir.IfFirError) as e:
            t.process_device(src.ptr, dst.ptr, F + 1, F + 1)
        assert str(e.value) == who + "65 frames exceed ullMaxFrames 64 of init"
        for bad_in, bad_out in ((4, 0), (0, 4)):
            with pytest.raises(fir.IfFirError) as e:
                t.process_device(src.ptr + bad_in, dst.ptr + bad_out, 8, 8)
            assert str(e.value) == who + "device pointers must be aligned to one element: 8-byte (input) and 8-byte (output)"
        t.set_input_format(fir.INPUT_I16)
        with pytest.raises(fir.IfFirError) as e:
            t.process_device(src.ptr + 2, dst.ptr, 8, 8)
        assert str(e.value) == who + "device pointers must be aligned to one element: 4-byte (input) and 8-byte (output)"
        t.set_input_format(fir.INPUT_F32)
        for pin, pout in ((0, dst.ptr), (src.ptr, 0)):
            with pytest.raises(fir.IfFirError) as e:
                t.process_device(pin, pout, 8, 8)
            assert str(e.value) == who + "NULL device pointer"
        t.process_device(0, 0, 0, 0)                          # F = 0 is legal, with no pointers at all, and writes nothing
        with pytest.raises(fir.IfFirError, match="if_fir_turn_set_output_format: unknown format 2"):
            t.set_output_format(2)
        with pytest.raises(fir.IfFirError, match="if_fir_turn_set_input_format: unknown format 2"):
            t.set_input_format(2)
        side = torch.cuda.Stream()
        t.set_stream(side.cuda_stream)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            graph.capture_begin()
            try:
                with pytest.raises(fir.IfFirError) as e:
                    t.process_device(src.ptr, dst.ptr, 8, 8)
            finally:
                graph.capture_end()
        assert str(e.value) == who + "the context's stream is being captured into a hipGraph; calls carry host-side streaming state and cannot be replayed"
        t.set_stream(0)
        t.synchronize()
        assert np.array_equal(dst.get(), before)              # nothing was written
        # the context is usable after all of them
        got, want = run(torch, t, TO_STREAMS, F, F, False, False)
        assert same(got, want)
    head = "if_fir_turn_init: "
    for kw, message in ((dict(sel=[5, 9, 5]), "bin 5 is listed twice (places 0 and 2)"),
                        (dict(sel=[5, 65, 7]), "bin 65 at place 1 of the list is outside the frame's 65"),
                        (dict(sel=[5, 9, 7], first=2), "ulFirst must be 0 beside a list of bins (got 2)"),
                        (dict(channels=66), "channels must be 1..65, the frame's bins (got 66)")):
        for direction in (TO_STREAMS, TO_FRAMES):
            with pytest.raises(fir.IfFirError) as e:
                fir.IfFirTurn(direction, B, **kw)
            assert str(e.value) == head + message


@pytest.mark.gpu
@pytest.mark.parametrize("i16", [False, True])
@pytest.mark.parametrize("B,C,F,kind", [(918, 65, 129, "straddle"), (65, 65, 64, "reversed"), (4097, 3, 65, "scattered")])
def test_round_trip(gpu_ok, fir, torch_cuda, B, C, F, kind, i16):
    """TO_FRAMES after TO_STREAMS on the device, at an odd pitch with a tail: the input frames with the unlisted bins zeroed"""
    torch = torch_cuda
    sel = turn_ref.selection(kind, B, C)
    frames = elements((F, B), i16, 11)
    P = F + 2 if F % 2 else F + 1
    src, mid, dst = Buffer(torch, F * B, i16), Buffer(torch, C * P, i16), Buffer(torch, F * B, i16)
    src.put(flat_image(src, frames))
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    with make(fir, TO_STREAMS, B, sel, i16, i16, max_frames=F) as down, make(fir, TO_FRAMES, B, sel, i16, i16, max_frames=F) as up:
        down.set_stream(stream.cuda_stream)
        up.set_stream(stream.cuda_stream)
        down.process_device(src.ptr, mid.ptr, F, P)
        up.process_device(mid.ptr, dst.ptr, F, P)             # no host copy and no synchronisation in between
        stream.synchronize()
    want = np.zeros_like(frames)
    want[:, sel] = frames[:, sel]
    assert same(dst.get(), flat_image(dst, want))
    assert same(mid.get(), rows_image(mid, turn_ref.to_streams(frames, sel, i16), P))


# ---- offsets past 2^32 ------------------------------------------------------------------------------------------------------------
def _words(torch, n, seed):
    """n float32 elements as int64 words (whatever the bits are: the comparison is on integers)"""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    return torch.randint(-2 ** 62, 2 ** 62, (n,), dtype=torch.int64, device="cuda", generator=g)


@pytest.mark.gpu
@pytest.mark.parametrize("direction", [TO_STREAMS, TO_FRAMES])
def test_row_offsets_past_2_32(gpu_ok, fir, torch_cuda, direction):
    """C = 3 rows at a pitch of 2^28 + 5 float32 elements: row 2 starts 4.3e9 bytes in.  The row side is allocated
    uninitialised; only the pieces a call reads or writes and a guard band beside each are looked at"""
    torch = torch_cuda
    B, C, F, P = 65, 3, 100, 2 ** 28 + 5
    sel = turn_ref.selection("scattered", B, C)
    assert 8 * (C - 1) * P > 2 ** 32
    rows = torch.empty((C - 1) * P + F + GUARD, dtype=torch.int64, device="cuda")
    canary = -0x5A5A5A5A5A5A5A5B
    for c in range(C):
        rows[c * P + F: c * P + F + GUARD] = canary
        if c:
            rows[c * P - GUARD: c * P] = canary
    with make(fir, direction, B, sel, max_frames=F) as t:
        if direction == TO_STREAMS:
            frames = _words(torch, F * B, 1)
            torch.cuda.synchronize()
            t.process_device(frames.data_ptr(), rows.data_ptr(), F, P)
            t.synchronize()
            fr = frames.view(F, B)
            for c in range(C):
                assert torch.equal(rows[c * P: c * P + F], fr[:, sel[c]]), c
        else:
            src = [_words(torch, F, 10 + c) for c in range(C)]
            for c in range(C):
                rows[c * P: c * P + F] = src[c]
            out = torch.full((F * B + GUARD,), canary, dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            t.process_device(rows.data_ptr(), out.data_ptr(), F, P)
            t.synchronize()
            want = torch.zeros((F, B), dtype=torch.int64, device="cuda")
            for c in range(C):
                want[:, sel[c]] = src[c]
            assert torch.equal(out[:F * B].view(F, B), want) and bool((out[F * B:] == canary).all())
    for c in range(C):
        assert bool((rows[c * P + F: c * P + F + GUARD] == canary).all()), c
        if c:
            assert bool((rows[c * P - GUARD: c * P] == canary).all()), c


@pytest.mark.gpu
@pytest.mark.parametrize("direction", [TO_STREAMS, TO_FRAMES])
def test_frame_offsets_past_2_32(gpu_ok, fir, torch_cuda, direction):
    """B = 8192 and 2^16 + 3 float32 frames: 4.3e9 bytes on the frame side, two scattered bins; compared on the device"""
    torch = torch_cuda
    B, C, F = 8192, 2, 2 ** 16 + 3
    sel = [8190, 77]
    assert 8 * F * B > 2 ** 32
    P = F + 1
    canary = -0x5A5A5A5A5A5A5A5B
    with make(fir, direction, B, sel, max_frames=F) as t:
        if direction == TO_STREAMS:
            frames = torch.empty(F * B, dtype=torch.int64, device="cuda")     # uninitialised but for the bins the call reads
            fr = frames.view(F, B)
            for c in range(C):
                fr[:, sel[c]] = _words(torch, F, 20 + c)
            rows = torch.full((C * P + GUARD,), canary, dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            t.process_device(frames.data_ptr(), rows.data_ptr(), F, P)
            t.synchronize()
            for c in range(C):
                assert torch.equal(rows[c * P: c * P + F], fr[:, sel[c]]), c
                assert bool((rows[c * P + F: (c + 1) * P] == canary).all())
            assert bool((rows[C * P:] == canary).all())
        else:
            rows = _words(torch, C * P, 30)
            out = torch.empty(F * B + GUARD, dtype=torch.int64, device="cuda")
            out[F * B:] = canary
            torch.cuda.synchronize()
            t.process_device(rows.data_ptr(), out.data_ptr(), F, P)
            t.synchronize()
            fr = out[:F * B].view(F, B)
            for c in range(C):
                assert torch.equal(fr[:, sel[c]], rows[c * P: c * P + F]), c
            # every other element is zero: the sum of the absolute values of all equals that of the two listed columns
            nz = torch.count_nonzero(fr)
            assert int(nz) == int(torch.count_nonzero(fr[:, sel[0]])) + int(torch.count_nonzero(fr[:, sel[1]]))
            assert bool((out[F * B:] == canary).all())


# ---- chains -----------------------------------------------------------------------------------------------------------------------
def _prototype(M):
    return (np.hanning(4 * M) * np.sinc((np.arange(4 * M) - 2 * M + 0.5) / M)).astype(np.float32)


@pytest.mark.gpu
def test_bank_turn_resampler_chain(gpu_ok, fir, torch_cuda):
    """IfFirPfb(M = 256) -> turn -> IfFirArb on a row, all on one stream with no host copy: the bits of the same resampler
    configuration run on frames[:, sel[c]].contiguous()"""
    from matrix_util import row_edge_taps
    torch = torch_cuda
    M, frames_n = 256, 300
    n = M * frames_n
    sel = [201, 17]
    rng = np.random.default_rng(256)
    x = (0.2 * rng.standard_normal(2 * n)).astype(np.float32)
    b, T, R = 4, 27, 2 ** 32 + 999
    taps = row_edge_taps(T, 1 << b, False)
    P = frames_n + 1                                            # odd: row 1 starts off the 16-byte grid
    stream = torch.cuda.Stream()
    din = torch.from_numpy(x).cuda()
    dbank = torch.zeros(frames_n * M, dtype=torch.int64, device="cuda")
    drows = torch.zeros(2 * P, dtype=torch.int64, device="cuda")
    with fir.IfFirPfb(_prototype(M), M, max_samples=n) as bank, make(fir, TO_STREAMS, M, sel, max_frames=frames_n) as t, \
            fir.IfFirArb(taps, b, R, max_samples=frames_n) as arb:
        m = arb.out_count(frames_n)
        assert m > frames_n // 2
        outs = [torch.zeros(m, dtype=torch.int64, device="cuda") for _ in range(4)]
        torch.cuda.synchronize()
        for c in (bank, t, arb):
            c.set_stream(stream.cuda_stream)
        assert bank.process_device(din.data_ptr(), dbank.data_ptr(), n) == frames_n
        t.process_device(dbank.data_ptr(), drows.data_ptr(), frames_n, P)
        for c in range(2):
            arb.reset()
            assert arb.process_device(drows.data_ptr() + 8 * c * P, outs[c].data_ptr(), frames_n) == m
        stream.synchronize()
        assert bool(torch.count_nonzero(dbank.view(frames_n, M)[:, sel[0]]) > frames_n // 2)
        for c in range(2):
            col = dbank.view(frames_n, M)[:, sel[c]].contiguous()
            torch.cuda.synchronize()
            arb.reset()
            assert arb.process_device(col.data_ptr(), outs[2 + c].data_ptr(), frames_n) == m
            stream.synchronize()
            assert torch.equal(outs[c], outs[2 + c]), c
        assert not torch.equal(outs[0], outs[1])


@pytest.mark.gpu
def test_turn_synthesis_chain(gpu_ok, fir, torch_cuda):
    """two rows -> turn (TO_FRAMES) -> IfFirSynth on one stream: the bits of IfFirSynth fed the same frames built in torch"""
    torch = torch_cuda
    M, F = 256, 120
    sel = [130, 9]
    P = F + 3
    rng = np.random.default_rng(257)
    rows = torch.from_numpy((0.2 * rng.standard_normal(2 * 2 * P)).astype(np.float32)).cuda()
    built = torch.zeros((F, M, 2), dtype=torch.float32, device="cuda")
    r = rows.view(2, P, 2)
    for c in range(2):
        built[:, sel[c]] = r[c, :F]
    dframes = torch.full((F * M * 2,), 7.0, dtype=torch.float32, device="cuda")
    stream = torch.cuda.Stream()
    h = _prototype(M)
    with make(fir, TO_FRAMES, M, sel, max_frames=F) as t, fir.IfFirSynth(h, M, max_frames=F) as synth:
        m = synth.sample_count(F)
        y = [torch.zeros(2 * m, dtype=torch.float32, device="cuda") for _ in range(2)]
        torch.cuda.synchronize()
        t.set_stream(stream.cuda_stream)
        synth.set_stream(stream.cuda_stream)
        t.process_device(rows.data_ptr(), dframes.data_ptr(), F, P)
        assert synth.process_device(dframes.data_ptr(), y[0].data_ptr(), F) == m
        stream.synchronize()
        assert torch.equal(dframes.view(torch.int32), built.view(-1).view(torch.int32))
        synth.reset()
        assert synth.process_device(built.data_ptr(), y[1].data_ptr(), F) == m
        stream.synchronize()
    assert torch.equal(y[0].view(torch.int32), y[1].view(torch.int32)) and bool(torch.count_nonzero(y[0]) > m)
