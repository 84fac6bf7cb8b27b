"""The frame power stage (if_fir_fpow_t, docs/SPEC.md §19) on the GPU: the bits of the float32 order model of tests/fpow_ref.py
in the powers and §8's mapping in the codes over the shape matrix; stream cuts, format changes, grid limits, off-grid pointers
and positions past 2^32 bit for bit in both outputs; failed calls and the host entry point; the chains real-input bank ->
stage -> detector and bank -> stage against the estimator, on device pointers with no host copy between the stages.  Device
output buffers carry a sentinel guard behind their last value, and the guard is checked.  Every test goes through
process_device unless it says otherwise.

Chain tolerance (SPEC §19): per frame, max_k |P - P_ref| <= CHAIN_EPS * max_k P_ref.  A plain complex64 bank into the float32
order model misses the float64 estimator by at most 1.2179e-7 of the frame's peak at the two shapes (tests/test_fpow_host.py
measures it); CHAIN_EPS is 4 times that, 4.8716e-7, the factor §8 gives its own figure, and is below the cap of 1e-5."""
import functools

import numpy as np
import pytest

import fpow_ref
import psd_ref

GUARD = 64              # elements behind the last frame
SENTINEL = 12345.0
SENTINEL_CODE = 0x5A5A
NORM = fpow_ref.NORM


@pytest.fixture(scope="module")
def torch_cuda(gpu_ok):
    import torch
    torch.cuda.set_device(0)
    return torch


def stream_frames(K):
    """three output frames and a ragged tail; the longest average: two"""
    return 2 * K + 5 if K == 65535 else 3 * K + min(K - 1, 5)


@functools.lru_cache(maxsize=None)
def signal(F, B, first, G, Bo, i16):
    raw = fpow_ref.make_signal(F, B, first, G, Bo, i16)
    raw.setflags(write=False)
    return raw


@functools.lru_cache(maxsize=None)
def model(F, B, first, G, Bo, K, i16, pos=0):
    """the float32 order model of the whole stream, computed once and left unchanged"""
    m = fpow_ref.model_f32(fpow_ref.values_f32(signal(F, B, first, G, Bo, i16), i16, B), first, G, Bo, K, NORM, pos)
    m.setflags(write=False)
    return m


def make(fir, B, first, G, Bo, K, i16, F, dev=False):
    return fir.IfFirFpow(B, K, norm=NORM, first=first, group=G, out_bins=Bo, ref_power=fpow_ref.ref_power_of(i16),
                         input_format=fir.INPUT_I16 if i16 else fir.INPUT_F32, max_frames=F, dev=dev)


def run_device(torch, f, raw, pieces, first=0, formats=None, want_power=True, off=(0, 0, 0)):
    """feed `raw` (frames of f.bins elements) from ONE device buffer in consecutive pieces of frames to a context at absolute
    frame index `first`; frame_count is checked before every call and the guards behind the last frame after the last one.
    formats: one input format per piece, `raw` then maps each format to the stream in it.  off: elements by which the input,
    code and power pointers are moved off the allocation's alignment.  Returns ((frames, Bo) codes, (frames, Bo) powers,
    frames per call)."""
    B, Bo, K = f.bins, f.out_bins, f.frames
    if formats is None:
        i16 = raw.dtype == np.int16
        raw, formats = {i16: raw}, [i16] * len(pieces)
    F = next(iter(raw.values())).size // (2 * B)
    din = {}
    for k, v in raw.items():
        assert v.size == 2 * F * B
        din[k] = torch.zeros(v.size + 2 * off[0], dtype=torch.int16 if k else torch.float32, device="cuda")
        din[k][2 * off[0]:] = torch.from_numpy(np.array(v)).cuda()
    total = fpow_ref.frame_count(first, F, K)
    codes = torch.full((total * Bo + GUARD + off[1],), SENTINEL_CODE, dtype=torch.int16, device="cuda")
    power = torch.full((total * Bo + GUARD + off[2],), SENTINEL, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()   # the buffers are filled on torch's stream, the context works on its own
    pos = done = 0
    counts = []
    current = None
    for s, fmt in zip(pieces, formats):
        if fmt != current:
            f.set_input_format(1 if fmt else 0)
            current = fmt
        want = f.frame_count(s)
        assert want == fpow_ref.frame_count(first + pos, s, K), (pos, s, want)
        got = f.process_device(din[fmt].data_ptr() + (4 if fmt else 8) * (off[0] + pos * B), s,
                               codes.data_ptr() + 2 * (off[1] + done * Bo),
                               power.data_ptr() + 4 * (off[2] + done * Bo) if want_power else 0)
        assert got == want
        counts.append(got)
        pos += s
        done += got
    f.synchronize()
    assert pos == F and done == total
    hc = codes.cpu().numpy().view(np.uint16)
    hp = power.cpu().numpy()
    assert np.all(hc[:off[1]] == SENTINEL_CODE) and np.all(hc[off[1] + total * Bo:] == SENTINEL_CODE), "a guard around the codes was written"
    assert np.all(hp[:off[2]] == SENTINEL) and np.all(hp[off[2] + total * Bo:] == SENTINEL), "a guard around the powers was written"
    if not want_power:
        assert np.all(hp == SENTINEL)
    return hc[off[1]:off[1] + total * Bo].reshape(total, Bo).copy(), hp[off[2]:off[2] + total * Bo].reshape(total, Bo).copy(), counts


def same_bits(a, b):
    if a.shape != b.shape:
        print("fpow shapes differ: %r, %r" % (a.shape, b.shape))
        return False
    wa, wb = np.ascontiguousarray(a).view(np.uint32).reshape(-1), np.ascontiguousarray(b).view(np.uint32).reshape(-1)
    d = np.flatnonzero(wa != wb)
    if d.size:
        fa, fb = wa.view(np.float32), wb.view(np.float32)
        print("fpow bits differ in %d of %d words, first at %d (%r, %r), largest difference %g" % (
            d.size, wa.size, d[0], fa[d[0]], fb[d[0]], np.max(np.abs(fa[d].astype(np.float64) - fb[d]))))
    return d.size == 0


def check_codes(codes, power, ref_power):
    """every code within one of §8's mapping applied in float64 to the device's own float power"""
    want = fpow_ref.codes(power, ref_power).astype(np.int64)
    assert np.max(np.abs(codes.astype(np.int64) - want)) <= 1


@pytest.mark.gpu
@pytest.mark.parametrize("i16", [False, True])
@pytest.mark.parametrize("B,first,G,Bo,K", fpow_ref.MATRIX)
def test_bits_of_the_order_model(gpu_ok, fir, torch_cuda, B, first, G, Bo, K, i16):
    """pfPower is the float32 order model bit for bit, the codes are §8's mapping of it within one; the loud bin clamps at
    65535, the zero bin reads power 0 and code 0"""
    F = stream_frames(K)
    raw = signal(F, B, first, G, Bo, i16)
    with make(fir, B, first, G, Bo, K, i16, F) as f:
        codes, power, counts = run_device(torch_cuda, f, raw, [F])
    want = model(F, B, first, G, Bo, K, i16)
    assert counts == [2 if K == 65535 else 3] and power.shape == want.shape
    assert same_bits(power, want)
    check_codes(codes, power, fpow_ref.ref_power_of(i16))
    loud, zero, clamp = fpow_ref.special_bins(Bo)
    if loud is not None:
        assert np.all(codes[:, loud] == 65535)
    if zero is not None:
        assert np.all(power[:, zero] == 0) and np.all(codes[:, zero] == 0)
    if clamp is not None:
        assert np.any(codes[:, clamp] == 65535)
    if Bo >= 5:
        noise = np.delete(codes, [loud, zero, clamp], axis=1)
        assert np.any((noise > 0) & (noise < 65535))


# the shapes of the cut tests: G = 1 with an odd B (the 16-byte and the element-aligned loads alternate by row) and a whole chunk
# per frame; G = 3 with two chunks and one frame
CUT_SHAPES = ((65, 1, 1, 64, 8), (200, 5, 3, 65, 17))


def cut_frames(K):
    return 6 * K + 3


def cut_lists(K, F):
    """pieces of 0, 1, 7, 8, 9, K - 1, K, K + 1 frames in two orders, and a random cut list"""
    named = [0, 1, 7, 8, 9, K - 1, K, K + 1]
    assert sum(named) < F
    rng = np.random.default_rng(K)
    cuts = np.sort(rng.integers(0, F + 1, 9))
    rand = [int(v) for v in np.diff(np.concatenate([[0], cuts, [F]]))]
    return [named + [F - sum(named)], [F - sum(named)] + named[::-1], rand]


@pytest.mark.gpu
@pytest.mark.parametrize("i16", [False, True])
@pytest.mark.parametrize("B,first,G,Bo,K", CUT_SHAPES)
def test_cuts_bit_for_bit(gpu_ok, fir, torch_cuda, B, first, G, Bo, K, i16):
    """process(a || b) == process(a); process(b) in both outputs wherever the frames are cut, calls of 0 and 1 frames included"""
    F = cut_frames(K)
    raw = signal(F, B, first, G, Bo, i16)
    with make(fir, B, first, G, Bo, K, i16, F) as f:
        codes, power, _ = run_device(torch_cuda, f, raw, [F])
        assert same_bits(power, model(F, B, first, G, Bo, K, i16))
        for pieces in cut_lists(K, F):
            f.reset()
            c, p, counts = run_device(torch_cuda, f, raw, pieces)
            assert sum(counts) == F // K and (0 not in pieces or counts[pieces.index(0)] == 0)
            assert same_bits(p, power) and np.array_equal(c, codes), pieces


@pytest.mark.gpu
@pytest.mark.parametrize("B,first,G,Bo,K", CUT_SHAPES)
def test_format_change_inside_a_chunk(gpu_ok, fir, torch_cuda, B, first, G, Bo, K):
    """the same values as int16 and as float32: a change of format at a cut inside a chunk keeps the stream and the bits"""
    F = cut_frames(K)
    xi = signal(F, B, first, G, Bo, True)
    both = {True: xi, False: xi.astype(np.float32) * np.float32(2.0 ** -15)}
    with make(fir, B, first, G, Bo, K, False, F) as f:
        codes, power, _ = run_device(torch_cuda, f, both[False], [F])
        assert same_bits(power, model(F, B, first, G, Bo, K, True))
        f.reset()
        pieces = [3, 2, K, 6, F - K - 11]
        c, p, _ = run_device(torch_cuda, f, both, pieces, formats=[False, True, False, True, False])
        assert same_bits(p, power) and np.array_equal(c, codes)


@pytest.mark.gpu
@pytest.mark.parametrize("i16", [False, True])
@pytest.mark.parametrize("limit", [1, 3])
def test_grid_limits(gpu_ok, fir, torch_cuda, limit, i16):
    """both kernels on 1 and on 3 workgroups: the stride loops turn, the bits stay"""
    B, first, G, Bo, K = 918, 0, 1, 918, 20
    F = stream_frames(K)
    raw = signal(F, B, first, G, Bo, i16)
    with make(fir, B, first, G, Bo, K, i16, F, dev=True) as f:
        f.debug_config(grid_limit=limit)
        codes, power, _ = run_device(torch_cuda, f, raw, [K + 3, F - K - 3])
    assert same_bits(power, model(F, B, first, G, Bo, K, i16))
    check_codes(codes, power, fpow_ref.ref_power_of(i16))


@pytest.mark.gpu
@pytest.mark.parametrize("i16", [False, True])
@pytest.mark.parametrize("B,first,G,Bo,K", [(64, 0, 1, 64, 8), (130, 2, 2, 64, 9), (4097, 1, 64, 64, 3)])
def test_pointers_one_element_off_the_16_byte_grid(gpu_ok, fir, torch_cuda, B, first, G, Bo, K, i16):
    """input, code and power pointers each one element past a 16-byte boundary: the element-aligned path, the same bits"""
    F = stream_frames(K)
    raw = signal(F, B, first, G, Bo, i16)
    with make(fir, B, first, G, Bo, K, i16, F) as f:
        codes, power, _ = run_device(torch_cuda, f, raw, [F])
        f.reset()
        c, p, _ = run_device(torch_cuda, f, raw, [F], off=(1, 1, 1))
    assert same_bits(power, model(F, B, first, G, Bo, K, i16))
    assert same_bits(p, power) and np.array_equal(c, codes)


@pytest.mark.gpu
@pytest.mark.parametrize("i16", [False, True])
@pytest.mark.parametrize("position", [2 ** 32 - 5, 2 ** 40 + 3])
def test_positions_past_2_32(gpu_ok, fir, torch_cuda, position, i16):
    """the context seeked there with nothing carried against the model started there, in one call and in three"""
    B, first, G, Bo, K = 130, 2, 2, 64, 9
    F = 4 * K + 2
    raw = signal(F, B, first, G, Bo, i16)
    want = model(F, B, first, G, Bo, K, i16, position)
    assert want.shape[0] == fpow_ref.frame_count(position, F, K) >= 4
    with make(fir, B, first, G, Bo, K, i16, F, dev=True) as f:
        for pieces in ([F], [4, 9, F - 13]):
            f.debug_config(position=position)
            codes, power, _ = run_device(torch_cuda, f, raw, pieces, first=position)
            assert same_bits(power, want)
            check_codes(codes, power, fpow_ref.ref_power_of(i16))


@pytest.mark.gpu
def test_a_failed_call_changes_nothing(gpu_ok, fir, torch_cuda):
    """c + F past 2^64 after a seek is refused with its message; position and carried sums are as before"""
    torch = torch_cuda
    B, first, G, Bo, K = 65, 1, 1, 64, 3
    start = 2 ** 64 - 12
    F = 11                                     # the last frame a stream has is 2^64 - 2: c + F = 2^64 - 1
    raw = signal(F, B, first, G, Bo, False)
    want = model(F, B, first, G, Bo, K, False, start)
    din = torch.from_numpy(np.array(raw)).cuda()
    dcodes = torch.zeros(8 * Bo, dtype=torch.int16, device="cuda")
    dpower = torch.full((8 * Bo,), SENTINEL, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    with make(fir, B, first, G, Bo, K, False, 64, dev=True) as f:
        f.debug_config(position=start)
        assert f.process_device(din.data_ptr(), 4, dcodes.data_ptr(), dpower.data_ptr()) == fpow_ref.frame_count(start, 4, K) == 1
        f.synchronize()
        before = dpower.cpu().numpy().copy()
        for bad in (9, 64):
            assert f.frame_count(bad) == 0
            with pytest.raises(fir.IfFirError, match="if_fir_fpow_process_device: frame count too large: the stream position would pass 2\\^64"):
                f.process_device(din.data_ptr(), bad, dcodes.data_ptr() + 2 * Bo, dpower.data_ptr() + 4 * Bo)
        with pytest.raises(fir.IfFirError, match="if_fir_fpow_process_device: 65 frames exceed ullMaxFrames 64 of init"):
            f.process_device(din.data_ptr(), 65, dcodes.data_ptr() + 2 * Bo, dpower.data_ptr() + 4 * Bo)
        with pytest.raises(fir.IfFirError, match="device pointers must be aligned to one element: 8-byte \\(input\\), 2-byte \\(codes\\), 4-byte \\(power\\)"):
            f.process_device(din.data_ptr() + 4, 1, dcodes.data_ptr() + 2 * Bo, dpower.data_ptr() + 4 * Bo)
        with pytest.raises(fir.IfFirError, match="if_fir_fpow_process_device: NULL device pointer"):
            f.process_device(din.data_ptr(), 7, 0, 0)
        f.synchronize()
        assert np.array_equal(dpower.cpu().numpy(), before)
        assert f.frame_count(F - 4) == fpow_ref.frame_count(start + 4, F - 4, K)
        got = f.process_device(din.data_ptr() + 8 * 4 * B, F - 4, dcodes.data_ptr() + 2 * Bo, dpower.data_ptr() + 4 * Bo)
        f.synchronize()
    assert got + 1 == want.shape[0]
    assert same_bits(dpower.cpu().numpy()[:want.size].reshape(want.shape), want)


@pytest.mark.gpu
@pytest.mark.parametrize("i16", [False, True])
@pytest.mark.parametrize("B,first,G,Bo,K", [(65, 1, 1, 64, 8), (200, 5, 3, 65, 17)])
def test_host_entry_point_and_null_power(gpu_ok, fir, torch_cuda, B, first, G, Bo, K, i16):
    """process (host pointers) in three calls equals process_device; without pfPower the codes are the same"""
    F = cut_frames(K)
    raw = signal(F, B, first, G, Bo, i16)
    cuts = [0, 5, K + 6, F]
    with make(fir, B, first, G, Bo, K, i16, F) as f:
        dcodes, dpower, _ = run_device(torch_cuda, f, raw, [F])
        f.reset()
        parts = [f.process(raw[2 * B * a:2 * B * b]) for a, b in zip(cuts[:-1], cuts[1:])]
        codes, power = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
        assert same_bits(power, dpower) and np.array_equal(codes, dcodes)
        f.reset()
        parts = [f.process(raw[2 * B * a:2 * B * b], want_power=False) for a, b in zip(cuts[:-1], cuts[1:])]
        assert all(p[1] is None for p in parts) and np.array_equal(np.concatenate([p[0] for p in parts]), dcodes)
        f.reset()
        c, _, _ = run_device(torch_cuda, f, raw, [5, F - 5], want_power=False)
        assert np.array_equal(c, dcodes)
        # an empty call on the host path, and one above init's size
        assert f.process(raw[:0])[0].shape == (0, Bo)
        with pytest.raises(fir.IfFirError, match="if_fir_fpow_process: %d frames exceed ullMaxFrames %d of init" % (F + 1, F)):
            f.process(np.zeros(2 * B * (F + 1), dtype=raw.dtype))


# ---- real-input bank -> stage -> detector ---------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_real_bank_feeds_the_stage_feeds_the_detector(gpu_ok, pkg, fir, torch_cuda):
    """IfFirRpfb(M = 256) -> IfFirFpow -> wb_detect_frames_device on one stream, no host copy and no synchronisation between
    the stages; the device detector's records equal the host detector's on the downloaded codes, and the codes are §8's mapping
    of the powers of the bank's own frames"""
    from oracle import wb_oracle
    torch = torch_cuda
    wb = pkg.wb_detect
    M, K, frames, cap = 256, 4, 6, 8
    bins = M // 2 + 1
    n = frames * K * M
    rng = np.random.default_rng(256)
    t = np.arange(n, dtype=np.float64)
    r = 0.05 * rng.standard_normal(n)
    for k in range(40, 53):                                   # a band of carriers 9 dB over the floor
        r += 0.012 * np.cos(2 * np.pi * (k + 0.37) / M * t + rng.uniform(0, 2 * np.pi))
    r = r.astype(np.float32)
    h = (np.hanning(4 * M) * np.sinc((np.arange(4 * M) - 2 * M + 0.5) / M)).astype(np.float32)
    norm = float(np.sum(h.astype(np.float64) ** 2))
    ref_power = 0.05 ** 2 / 10 ** 0.3                          # the floor reads about +3 dB
    stream = torch.cuda.Stream()
    din = torch.from_numpy(r).cuda()
    dbank = torch.full((2 * frames * K * bins + GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
    dcodes = torch.full((frames * bins + GUARD,), SENTINEL_CODE, dtype=torch.int16, device="cuda")
    dpower = torch.full((frames * bins + GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
    dframes = torch.zeros(frames * wb.FRAME_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    dsignals = torch.zeros(frames * cap * wb.SIGNAL_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    with fir.IfFirRpfb(h, M, max_samples=n) as bank, fir.IfFirFpow(bins, K, norm=norm, ref_power=ref_power, max_frames=frames * K) as f:
        bank.set_stream(stream.cuda_stream)
        f.set_stream(stream.cuda_stream)
        assert bank.process_device(din.data_ptr(), dbank.data_ptr(), n) == frames * K
        assert f.process_device(dbank.data_ptr(), frames * K, dcodes.data_ptr(), dpower.data_ptr()) == frames
        wb.detect_frames_device(dcodes.data_ptr(), frames, bins, dframes.data_ptr(), dsignals.data_ptr(), cap, 0, stream.cuda_stream)
        stream.synchronize()
    hb = dbank.cpu().numpy()
    hc = dcodes.cpu().numpy().view(np.uint16)
    hp = dpower.cpu().numpy()
    assert np.all(hb[2 * frames * K * bins:] == SENTINEL) and np.all(hc[frames * bins:] == SENTINEL_CODE) and np.all(hp[frames * bins:] == SENTINEL)
    codes, power = hc[:frames * bins].reshape(frames, bins), hp[:frames * bins].reshape(frames, bins)
    want = fpow_ref.model_f32(hb[:2 * frames * K * bins].reshape(frames * K, bins, 2), 0, 1, bins, K, np.float32(norm))
    assert same_bits(power, want)
    check_codes(codes, power, float(np.float32(ref_power)))
    assert np.any((codes > 0) & (codes < 65535)) and np.median(codes[:, 40:53]) > np.median(codes[:, 60:]) + 10000
    got_frames = dframes.cpu().numpy().view(wb.FRAME_DTYPE)
    got_signals = dsignals.cpu().numpy().view(wb.SIGNAL_DTYPE).reshape(frames, cap)
    for k in range(frames):
        st, oframe, osig = wb_oracle.detect(codes[k], max_signals=cap)
        assert st == 1
        assert got_frames[k].tobytes() == oframe.tobytes(), k
        stored = min(int(oframe["signal_count"]), cap)
        assert got_signals[k][:stored].tobytes() == osig[:stored].tobytes(), k


# ---- bank -> stage against the estimator ------------------------------------------------------------------------------------------
def frame_errors(power, ref):
    assert power.shape == ref.shape and not np.any(np.isnan(power))
    return np.max(np.abs(power.astype(np.float64) - ref), axis=1) / np.max(ref, axis=1)


@pytest.mark.gpu
@pytest.mark.parametrize("N,H,K", fpow_ref.CHAIN_SHAPES)
def test_bank_and_stage_equal_the_estimator(gpu_ok, fir, torch_cuda, N, H, K):
    """IfFirPfb(N, taps = the reversed window, hop H) -> IfFirFpow(K) against IfFirPsd(N, H, K, window) on the same stream,
    aligned as SPEC §19 says: both within their tolerance of psd_ref.power_f64, their codes within 2 of each other"""
    torch = torch_cuda
    x = fpow_ref.chain_stream(N, H, K)
    n = x.size // 2
    w = psd_ref.hann(N)
    d, q = fpow_ref.chain_align(N, H)
    ref = psd_ref.power_f64(x, N, H, K, w)                    # bins -N/2 .. N/2 - 1
    frames = ref.shape[0]
    assert frames == (3 * K + 2) // K >= 3
    order = psd_ref.bin_indices(N, -N // 2, N)                # the estimator's column i is the bank's bin order[i]
    delayed = np.concatenate([np.zeros(2 * d, dtype=np.float32), x])
    nd = n + d
    bank_frames = -(-nd // H)
    assert bank_frames - q >= frames * K
    din = torch.from_numpy(delayed).cuda()
    dbank = torch.full((2 * bank_frames * N + GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
    dcodes = torch.full((frames * N + GUARD,), SENTINEL_CODE, dtype=torch.int16, device="cuda")
    dpower = torch.full((frames * N + GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    with fir.IfFirPfb(w[::-1].copy(), N, hop=H, max_samples=nd) as bank, \
            fir.IfFirFpow(N, K, norm=float(np.sum(w.astype(np.float64) ** 2)), ref_power=fpow_ref.CHAIN_REF_POWER,
                          max_frames=bank_frames) as f, \
            fir.IfFirPsd(N, H, K, -N // 2, N, ref_power=fpow_ref.CHAIN_REF_POWER, window=w, max_samples=n) as est:
        bank.set_stream(stream.cuda_stream)
        f.set_stream(stream.cuda_stream)
        assert bank.process_device(din.data_ptr(), dbank.data_ptr(), nd) == bank_frames
        # no host copy and no synchronisation in between; the stage starts at the bank's frame q
        assert f.process_device(dbank.data_ptr() + 8 * q * N, bank_frames - q, dcodes.data_ptr(), dpower.data_ptr()) == frames
        stream.synchronize()
        ecodes, epower = est.process(x)
    hc, hp = dcodes.cpu().numpy().view(np.uint16), dpower.cpu().numpy()
    assert np.all(hc[frames * N:] == SENTINEL_CODE) and np.all(hp[frames * N:] == SENTINEL)
    codes, power = hc[:frames * N].reshape(frames, N)[:, order], hp[:frames * N].reshape(frames, N)[:, order]
    assert epower.shape == ref.shape
    err, eerr = frame_errors(power, ref), frame_errors(epower, ref)
    worst = int(np.max(np.abs(codes.astype(np.int64) - ecodes.astype(np.int64))))
    print("fpow chain N=%d H=%d K=%d: bank -> stage %.3g of the peak (CHAIN_EPS %.3g), estimator %.3g (EPS %.3g), codes differ by at most %d"
          % (N, H, K, err.max(), fpow_ref.CHAIN_EPS, eerr.max(), psd_ref.EPS, worst))
    assert np.all(err <= fpow_ref.CHAIN_EPS), err
    assert np.all(eerr <= psd_ref.EPS), eerr
    check_codes(codes, power, fpow_ref.CHAIN_REF_POWER)
    assert np.any((codes > 0) & (codes < 65535))
    assert worst <= 2
