"""The streaming power-spectrum estimator (if_fir_psd_t, docs/SPEC.md §8) on the GPU against the float64 reference of
tests/psd_ref.py; bin selection, code mapping, stream cuts bit for bit, error paths, and estimator -> wb_detect on one stream.
Device output buffers carry a sentinel guard behind their last frame, and the guard is checked.  No call goes above 2^19 samples.

Tolerance (SPEC §8): per frame, max_k |P - P_ref| <= EPS * max_k P_ref over the frame's N bins.  A plain complex64
implementation (scipy.fft on complex64, float32 sums in the §8 order) misses the float64 reference by at most 3.2912e-7 of the
frame's peak over this file's matrix (tests/test_psd_host.py measures it); EPS is 4 times that, 1.31648e-6, which covers a
different butterfly order and table twiddles, and is below the cap of 1e-5."""
import functools

import numpy as np
import pytest

import psd_ref

EPS = psd_ref.EPS
GUARD = 64              # elements behind the last frame
SENTINEL = 12345.0
SENTINEL_CODE = 0x5A5A


@pytest.fixture(scope="module")
def torch_cuda(gpu_ok):
    import torch
    torch.cuda.set_device(0)
    return torch


@functools.lru_cache(maxsize=None)
def base_signal(n):
    import __graft_entry__ as g
    x = g.load_oracle().synth_iq(n, channel=3)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def signal(n, N, i16):
    """(what the context is fed, the same samples as float32)"""
    raw, x = psd_ref.matrix_signal(base_signal(n), N, i16)
    raw.setflags(write=False)
    x.setflags(write=False)
    return raw, x


def window_of(name, N):
    return None if name == "hann" else psd_ref.asymmetric_window(N)


@functools.lru_cache(maxsize=None)
def reference(n, N, H, K, i16, window):
    ref = psd_ref.power_f64(signal(n, N, i16)[1], N, H, K, window_of(window, N))
    ref.setflags(write=False)
    return ref


def run_device(torch, f, raw, pieces, i16=False, formats=None, want_power=True):
    """feed `raw` from ONE device buffer in consecutive pieces; frame_count is checked against the reference count before every
    call and the guards behind the last frame after the last one.  formats: per piece (float32 array, int16 array) choice.
    Returns ((frames, bins) codes, (frames, bins) power, frames per call)."""
    N, H, K, bins = f.size, f.hop, f.segments, f.bins
    if formats is None:
        n = raw.size // 2
        din = {i16: torch.from_numpy(np.array(raw)).cuda()}
        formats = [i16] * len(pieces)
    else:
        n = raw[False].size // 2
        din = {k: torch.from_numpy(np.array(v)).cuda() for k, v in raw.items()}
    total = psd_ref.frame_count(0, n, N, H, K)
    codes = torch.full((total * bins + GUARD,), SENTINEL_CODE, dtype=torch.int16, device="cuda")
    power = torch.full((total * bins + GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
    pos = done = 0
    counts = []
    current = None
    for s, fmt in zip(pieces, formats):
        assert s <= 1 << 19
        if fmt != current:
            f.set_input_format(1 if fmt else 0)
            current = fmt
        want = f.frame_count(s)
        assert want == psd_ref.frame_count(pos, s, N, H, K), (pos, s, want)
        got = f.process_device(din[fmt].data_ptr() + (4 if fmt else 8) * pos, s, codes.data_ptr() + 2 * done * bins,
                               power.data_ptr() + 4 * done * bins if want_power else 0)
        assert got == want
        counts.append(got)
        pos += s
        done += got
    f.synchronize()
    assert pos == n and done == total
    hc = codes.cpu().numpy().view(np.uint16)
    hp = power.cpu().numpy()
    assert np.all(hc[total * bins:] == SENTINEL_CODE), "the guard behind the last frame's codes was written"
    assert np.all(hp[total * bins:] == SENTINEL), "the guard behind the last frame's power was written"
    if not want_power:
        assert np.all(hp == SENTINEL)
    return hc[:total * bins].reshape(total, bins), hp[:total * bins].reshape(total, bins), counts


def check_codes(codes, power, ref_power):
    """every code within one of the mapping applied in float64 to the device's own float power"""
    want = psd_ref.codes(power, ref_power).astype(np.int64)
    assert np.max(np.abs(codes.astype(np.int64) - want)) <= 1


def frame_errors(power, ref):
    assert power.shape == ref.shape and not np.any(np.isnan(power))
    return np.max(np.abs(power.astype(np.float64) - ref), axis=1) / np.max(ref, axis=1)


def cases():
    return [(N, H, K, i16, w) for (N, H) in psd_ref.MATRIX for K in psd_ref.SEGMENTS for i16 in (False, True)
            for w in ("hann", "asymmetric")]


@pytest.mark.gpu
@pytest.mark.parametrize("N,H,K,i16,window", cases())
def test_matrix_against_float64(gpu_ok, fir, torch_cuda, N, H, K, i16, window):
    n = psd_ref.matrix_samples(N, H, K)
    raw, _ = signal(n, N, i16)
    ref = reference(n, N, H, K, i16, window)
    assert ref.shape[0] >= 2
    ref_power = 0.01
    with fir.IfFirPsd(N, H, K, -N // 2, N, ref_power=ref_power, window=window_of(window, N),
                      input_format=fir.INPUT_I16 if i16 else fir.INPUT_F32, max_samples=n) as f:
        cut = n // 3
        c1, p1 = f.process(raw[:2 * cut])
        c2, p2 = f.process(raw[2 * cut:])
        codes, power = np.concatenate([c1, c2]), np.concatenate([p1, p2])
        f.reset()
        dcodes, dpower, _ = run_device(torch_cuda, f, raw, [n], i16)
    err = frame_errors(power, ref)
    print("N=%d H=%d K=%d i16=%d %s: worst frame error %.3g of the peak (EPS %.3g)" % (N, H, K, i16, window, err.max(), EPS))
    assert np.all(err <= EPS), err
    check_codes(codes, power, ref_power)
    assert np.array_equal(dpower, power) and np.array_equal(dcodes, codes)


@pytest.mark.gpu
@pytest.mark.parametrize("N,first,bins", [(1024, -459, 918), (1024, 77, 1), (1024, -3, 7), (256, -128, 10), (256, 118, 10),
                                          (2048, -1024, 2048), (512, -256, 300), (4096, 1000, 1048)])
def test_bin_selection(gpu_ok, fir, torch_cuda, N, first, bins):
    """918 centred bins of 1024, a single bin, a span crossing DC, spans touching -N/2 and N/2, all bins: the selected bins carry
    exactly the bits of the same bins of an all-bins context (which test_matrix holds to the float64 reference), and meet the
    reference themselves"""
    H, K = N // 2, 3
    n = psd_ref.matrix_samples(N, H, K)
    raw, x = signal(n, N, False)
    ref_all = reference(n, N, H, K, False, "hann")
    with fir.IfFirPsd(N, H, K, -N // 2, N, ref_power=0.01, max_samples=n) as f:
        call, pall, _ = run_device(torch_cuda, f, raw, [n])
    with fir.IfFirPsd(N, H, K, first, bins, ref_power=0.01, max_samples=n) as f:
        csel, psel, _ = run_device(torch_cuda, f, raw, [n])
    lo = first + N // 2
    assert np.array_equal(psel, pall[:, lo:lo + bins]) and np.array_equal(csel, call[:, lo:lo + bins])
    ref = psd_ref.power_f64(x, N, H, K, None, first, bins)
    assert np.all(np.max(np.abs(psel - ref), axis=1) <= EPS * np.max(ref_all, axis=1))
    assert np.all(frame_errors(pall, ref_all) <= EPS)


@pytest.mark.gpu
def test_codes_at_the_clamps(gpu_ok, fir, torch_cuda):
    N, H, K = 512, 192, 3
    n = psd_ref.matrix_samples(N, H, K)
    with fir.IfFirPsd(N, H, K, -N // 2, N, ref_power=1.0, max_samples=n) as f:
        codes, power, _ = run_device(torch_cuda, f, np.zeros(2 * n, dtype=np.float32), [n])
        assert codes.shape[0] >= 2 and np.all(codes == 0) and np.all(power == 0.0) and not np.any(np.isnan(power))
    # a full-scale tone on bin 40 with a small reference power: the top of the scale on its bin
    t = np.arange(n)
    tone = np.exp(2j * np.pi * 40 / N * t)
    xi = np.empty(2 * n, dtype=np.int16)
    xi[0::2] = np.clip(np.round(tone.real * 32767), -32768, 32767)
    xi[1::2] = np.clip(np.round(tone.imag * 32767), -32768, 32767)
    with fir.IfFirPsd(N, H, K, -N // 2, N, ref_power=1e-3, input_format=fir.INPUT_I16, max_samples=n) as f:
        codes, power, _ = run_device(torch_cuda, f, xi, [n], i16=True)
        assert np.all(codes[:, N // 2 + 40] == 65535) and np.all(np.argmax(power, axis=1) == N // 2 + 40)
        check_codes(codes, power, 1e-3)
        assert codes.min() < 65535


def cut_lists(N, H, K, n):
    """pieces that sum to n: cuts inside a segment, inside a chunk, on a chunk edge and on a frame edge; a call shorter than
    one segment; a 0-sample call; a run of 1-sample calls across a segment's, a chunk's or a frame's last sample"""
    chunk_edge = 7 * H + N           # the first chunk's last sample + 1
    frame_edge = (K - 1) * H + N     # the first frame's last sample + 1
    marks = sorted({N // 3, N // 3 + 5, N + H // 2 + 1, chunk_edge - 1, chunk_edge, chunk_edge + H + 3, frame_edge, frame_edge + 1,
                    frame_edge + 8 * H + N // 2, 2 * frame_edge})
    marks = [m for m in marks if 0 < m < n]
    a = [b - a for a, b in zip([0] + marks, marks + [n])]
    a.insert(3, 0)
    ones_from = frame_edge - 40
    run = min(300, n - ones_from - 1)
    b = [ones_from] + [1] * run + [0] + [n - ones_from - run]
    c = [chunk_edge - 3, 0] + [1] * 6 + [n - chunk_edge - 3]
    for pieces in (a, b, c):
        assert sum(pieces) == n and min(pieces) >= 0
    return a, b, c


@pytest.mark.gpu
@pytest.mark.parametrize("N,H,K", [(1024, 385, 9), (256, 1, 20)])
def test_stream_cuts_bit_for_bit(gpu_ok, fir, torch_cuda, N, H, K):
    n = (3 * K + 2) * H + N + 11
    xi, x = signal(n, N, True)       # int16 samples and the same values as float32: a change of format keeps the bits
    both = {False: x, True: xi}
    with fir.IfFirPsd(N, H, K, -N // 2, N, ref_power=0.01, max_samples=n, dev=True) as f:
        codes, power, counts = run_device(torch_cuda, f, x, [n])
        assert counts == [3] and np.all(frame_errors(power, psd_ref.power_f64(x, N, H, K)) <= EPS)
        for pieces in cut_lists(N, H, K, n):
            f.reset()
            c, p, counts = run_device(torch_cuda, f, x, pieces)
            assert sum(counts) == 3 and counts[pieces.index(0)] == 0
            assert np.array_equal(p, power) and np.array_equal(c, codes), pieces
        # float32, then int16 from a cut inside a chunk on
        pieces = [5 * H + N // 2, 0, 6 * H + 1, n - 11 * H - N // 2 - 1]
        f.reset()
        c, p, _ = run_device(torch_cuda, f, both, pieces, formats=[False, False, True, True])
        assert np.array_equal(p, power) and np.array_equal(c, codes)
        # the host entry point, the power left out
        f.reset()
        f.set_input_format(fir.INPUT_F32)
        parts, pos = [], 0
        for s in pieces:
            plan = f.debug_plan(s)
            assert plan[2] == f.frame_count(s) and plan[3] < 7 * H + N
            got, none = f.process(x[2 * pos:2 * (pos + s)], want_power=False)
            assert none is None and got.shape == (plan[2], N)
            parts.append(got)
            pos += s
        assert np.array_equal(np.concatenate(parts), codes)
        # reset in the middle of a frame returns to the first frame's bits
        f.process(x[:2 * (N + 3 * H + 7)])
        f.reset()
        c, p = f.process(x[:2 * ((K - 1) * H + N)])
        assert np.array_equal(c, codes[:1]) and np.array_equal(p, power[:1])


@pytest.mark.gpu
@pytest.mark.parametrize("N,H,K", [(1024, 385, 9), (256, 1, 20), (4096, 4095, 3)])
def test_plan_hook_is_the_reference_plan(gpu_ok, fir, N, H, K):
    rng = np.random.default_rng(N + K)
    with fir.IfFirPsd(N, H, K, 0, 1, max_samples=12 * H + N, dev=True) as f:
        pos = carried = 0
        zeros = np.zeros(2 * (12 * H + N), dtype=np.float32)
        for s in [0, 1, N - 1, 1, 7 * H] + [int(v) for v in rng.integers(0, 12 * H + N, 12)]:
            want = psd_ref.plan(pos, carried, s, N, H, K)
            assert f.debug_plan(s) == want, (pos, carried, s)
            f.process(zeros[:2 * s])
            pos, carried = pos + s, want[3]


@pytest.mark.gpu
@pytest.mark.filterwarnings("ignore:The CUDA Graph is empty")
def test_rejected_arguments_leave_the_stream(gpu_ok, fir, torch_cuda):
    torch = torch_cuda
    N, H, K = 256, 100, 3
    n = 4000
    _, x = signal(n, N, False)
    for kw in (dict(size=300), dict(size=128), dict(size=8192), dict(hop=0), dict(hop=N + 1), dict(segments=0), dict(segments=65536),
               dict(first_bin=-N // 2 - 1), dict(first_bin=N // 2 - 9, bins=10), dict(bins=0), dict(bins=N + 1, first_bin=-N // 2),
               dict(ref_power=0.0), dict(input_format=7), dict(max_samples=0)):
        args = dict(size=N, hop=H, segments=K, first_bin=-5, bins=10, ref_power=1.0)
        args.update(kw)
        with pytest.raises(fir.IfFirError) as e:
            fir.IfFirPsd(**args)
        assert "if_fir_psd_init" in str(e.value), kw
    with fir.IfFirPsd(N, H, K, -5, 10, ref_power=0.01, max_samples=n) as f:
        codes, power = f.process(x)
        f.reset()
        cut = 1001
        first = f.process(x[:2 * cut])
        with pytest.raises(fir.IfFirError, match="ullMaxSamples"):
            f.process(np.zeros(2 * (n + 1), dtype=np.float32))
        with pytest.raises(fir.IfFirError, match="format"):
            f.set_input_format(5)
        buf = torch.zeros(2 * n + 8, dtype=torch.float32, device="cuda")
        out = torch.zeros(64 * 10, dtype=torch.int16, device="cuda")
        with pytest.raises(fir.IfFirError, match="ullMaxSamples"):
            f.process_device(buf.data_ptr(), n + 1, out.data_ptr())
        with pytest.raises(fir.IfFirError, match="NULL"):
            f.process_device(0, 100, out.data_ptr())
        assert f.frame_count(n - cut) > 0
        with pytest.raises(fir.IfFirError, match="NULL"):
            f.process_device(buf.data_ptr(), n - cut, 0)
        with pytest.raises(fir.IfFirError, match="aligned"):
            f.process_device(buf.data_ptr() + 4, 100, out.data_ptr())
        with pytest.raises(fir.IfFirError, match="aligned"):
            f.process_device(buf.data_ptr(), 100, out.data_ptr() + 1)
        side = torch.cuda.Stream()
        f.set_stream(side.cuda_stream)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            graph.capture_begin()
            try:
                with pytest.raises(fir.IfFirError, match="captured"):
                    f.process_device(buf.data_ptr(), 100, out.data_ptr())
            finally:
                graph.capture_end()
        f.set_stream(0)
        # every refused call left the stream where it was
        rest = f.process(x[2 * cut:])
        assert np.array_equal(np.concatenate([first[0], rest[0]]), codes) and np.array_equal(np.concatenate([first[1], rest[1]]), power)


# ---- estimator -> detector ------------------------------------------------------------------------------------------------
E2E = dict(N=1024, H=512, K=64, first=-459, bins=918, frames=6)
E2E_FLOOR = 1e-4                              # noise power per complex sample
E2E_REF = E2E_FLOOR / 10 ** (-0.03)           # the floor sits at -0.3 dB: 2 dB below code 16500 (1.698 dB)
# (low edge MHz, high edge MHz, dB above the floor): a 1.5 MHz beacon centred below 10492 MHz, a 0.55 MHz signal (symbol-rate
# class 500) 3 dB under it and a 0.95 MHz signal (class 1000) 1 dB over it (over-powered)
E2E_SIGNALS = ((10490.9, 10492.4, 10.0), (10494.0, 10494.55, 7.0), (10496.0, 10496.95, 11.0))


def e2e_input():
    """seeded band-limited noise: each signal is white noise cut to its band in the frequency domain of the whole stream"""
    n = (E2E["frames"] * E2E["K"] - 1) * E2E["H"] + E2E["N"]
    rng = np.random.default_rng(2024)
    step = 9.0 / E2E["bins"]                 # MHz per bin: the detector's 10490.5 .. 10499.5 MHz over the frame
    white = lambda: (rng.standard_normal(n) + 1j * rng.standard_normal(n)) / np.sqrt(2)
    x = white() * np.sqrt(E2E_FLOOR)
    f = np.fft.fftfreq(n) * E2E["N"]         # in bins of the transform
    for lo, hi, db in E2E_SIGNALS:
        b0, b1 = (lo - 10490.5) / step + E2E["first"], (hi - 10490.5) / step + E2E["first"]
        X = np.fft.fft(white())
        X[(f < b0) | (f > b1)] = 0
        x = x + np.fft.ifft(X) * np.sqrt(E2E_FLOOR * (10 ** (db / 10) - 1))
    iq = np.empty(2 * n, dtype=np.float32)
    iq[0::2], iq[1::2] = x.real, x.imag
    assert np.max(np.abs(iq)) < 1.0          # below full scale
    return iq


EQUAL_FIELDS = ("symbolrate", "out_of_band", "over_powered")


def same_detection(a, b):
    (fa, sa), (fb, sb) = a, b
    return (fa["signal_count"] == fb["signal_count"] and fa["beacon_valid"] == fb["beacon_valid"] and len(sa) == len(sb)
            and all(x[k] == y[k] for x, y in zip(sa, sb) for k in EQUAL_FIELDS)
            and all(fa["beacon"][k] == fb["beacon"][k] for k in EQUAL_FIELDS))


@pytest.mark.gpu
def test_estimator_feeds_the_detector_on_one_stream(gpu_ok, pkg, fir, torch_cuda):
    from oracle import wb_oracle
    torch = torch_cuda
    N, H, K, first, bins, frames = (E2E[k] for k in ("N", "H", "K", "first", "bins", "frames"))
    iq = e2e_input()
    n = iq.size // 2
    ref_codes = psd_ref.codes(psd_ref.power_f64(iq, N, H, K, None, first, bins), E2E_REF)
    assert ref_codes.shape == (frames, bins)
    allow = 1 + (10 / np.log(10)) * EPS * 100 / psd_ref.SLOPE    # codes: the code error EPS allows 20 dB below the peak
    want = []
    rng = np.random.default_rng(7)
    for k in range(frames):
        st, frame, sig = wb_oracle.detect(ref_codes[k])
        assert st == 1 and frame["beacon_valid"] == 1 and frame["signal_count"] == 2
        assert frame["beacon"]["used_bandwidth"] >= 1.0 and frame["beacon"]["used_center_freq"] < 10492.0
        assert [s["symbolrate"] for s in sig] == [500.0, 1000.0] and [s["over_powered"] for s in sig] == [0, 1]
        floor_code = (frame["noise_power"] - psd_ref.ZERO_DB) / psd_ref.SLOPE
        assert 1.5 <= (16500 - floor_code) * psd_ref.SLOPE <= 2.5
        want.append((frame, sig))
        # the input is fair: reference codes moved by up to `allow` codes give the same detection
        for _ in range(8):
            moved = np.clip(ref_codes[k].astype(np.int64) + rng.integers(-int(allow), int(allow) + 1, bins), 0, 65535)
            st, f2, s2 = wb_oracle.detect(moved)
            assert st == 1 and same_detection((frame, sig), (f2, s2))

    wb = pkg.wb_detect
    cap = 8
    stream = torch.cuda.Stream()
    din = torch.from_numpy(iq).cuda()
    dcodes = torch.full((frames * bins + GUARD,), SENTINEL_CODE, dtype=torch.int16, device="cuda")
    dframes = torch.zeros(frames * wb.FRAME_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    dsignals = torch.zeros(frames * cap * wb.SIGNAL_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    with fir.IfFirPsd(N, H, K, first, bins, ref_power=E2E_REF, max_samples=n) as f:
        f.set_stream(stream.cuda_stream)
        assert f.process_device(din.data_ptr(), n, dcodes.data_ptr()) == frames
        # no host copy and no synchronisation in between: the detector reads the estimator's frames on the same stream
        wb.detect_frames_device(dcodes.data_ptr(), frames, bins, dframes.data_ptr(), dsignals.data_ptr(), cap, 0, stream.cuda_stream)
        stream.synchronize()
    got_codes = dcodes.cpu().numpy().view(np.uint16)
    assert np.all(got_codes[frames * bins:] == SENTINEL_CODE)
    got_frames = dframes.cpu().numpy().view(wb.FRAME_DTYPE)
    got_signals = dsignals.cpu().numpy().view(wb.SIGNAL_DTYPE).reshape(frames, cap)
    step = 9.0 / bins
    db = allow * psd_ref.SLOPE
    print("codes differ from the reference's by at most %d (allowed at 20 dB below the peak: %.2f)"
          % (np.max(np.abs(got_codes[:frames * bins].astype(np.int64) - ref_codes.reshape(-1))), allow))
    for k in range(frames):
        frame, sig = want[k]
        gf, gs = got_frames[k], got_signals[k][:int(got_frames[k]["signal_count"])]
        assert same_detection((frame, sig), (gf, gs)), k
        assert abs(gf["noise_power"] - frame["noise_power"]) <= db
        for a, b in [(frame["beacon"], gf["beacon"])] + list(zip(sig, gs)):
            for name in ("full_start_freq", "full_end_freq", "full_center_freq", "used_start_freq", "used_end_freq", "used_center_freq"):
                assert abs(a[name] - b[name]) <= step * (1 + 1e-9), (k, name)
            for name in ("full_power", "used_power"):
                assert abs(a[name] - b[name]) <= db, (k, name, a[name], b[name])
