"""The streaming power-spectrum estimator (if_fir_psd_t, docs/SPEC.md §8) where tests/test_psd_gpu.py does not go: averages of
thousands of segments (the frame kernel adds up to 8192 chunk sums and calls start at chunk indices in the thousands), calls of
thousands of chunks (the chunk kernel's grid-stride loop turns, on any chip and under a grid limit), calls of thousands of frames,
stream positions past 2^32, 2^40 and up to 2^64, and device pointers off the allocation's grid.

Two kinds of check.  Bit for bit: with the all-ones window sum w^2 = N exactly, so a context of 8 segments per frame has the
scale 2^-(3 + log2 N) and its power output times 8 N IS the chunk sum; a long frame must then be psd_ref.chunk_order_power of those
chunk sums, the float32 accumulation §8 pins.  Against float64: max_k |P - P_ref| <= eps_of(K) max_k P_ref per frame, where
eps_of(K) = EPS up to three chunks per frame and EPS + ceil(K / 8) 2^-24 beyond (SPEC §8; tests/test_psd_host.py holds the plain
complex64 implementation to the same rule).  No call goes above 2^19 samples."""
import numpy as np
import pytest

import psd_ref
from test_psd_gpu import (EPS, GUARD, SENTINEL, SENTINEL_CODE, check_codes, cut_lists, frame_errors, reference, run_device, signal,
                          window_of)

TINY = np.finfo(np.float32).tiny


@pytest.fixture(scope="module")
def torch_cuda(gpu_ok):
    import torch
    torch.cuda.set_device(0)
    return torch


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b)


def feed(torch, f, raw, pieces, i16=False, seg0=0, shift=0, before=None):
    """run_device for a context whose stream starts at segment seg0 of a frame (a seek), with `shift` elements in FRONT of the
    input (one sample each), the codes and the power inside their allocations, and sentinel guards in front of both outputs as well
    as behind; before(pos, s) runs ahead of every call.  Returns (codes, power, frames per call)."""
    N, H, K, bins = f.size, f.hop, f.segments, f.bins
    n = raw.size // 2
    done_at = lambda p: (seg0 + psd_ref.segments_complete(p, N, H)) // K - seg0 // K
    total = done_at(n)
    pad = np.zeros(2 * shift, dtype=raw.dtype)
    din = torch.from_numpy(np.concatenate([pad, np.array(raw)])).cuda()
    codes = torch.full((shift + total * bins + GUARD,), SENTINEL_CODE, dtype=torch.int16, device="cuda")
    power = torch.full((shift + total * bins + GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
    size = 4 if i16 else 8
    assert shift == 0 or (din.data_ptr() + size * shift) % 16 and (codes.data_ptr() + 2 * shift) % 4 and (power.data_ptr() + 4 * shift) % 8
    pos = done = 0
    counts = []
    for s in pieces:
        assert s <= 1 << 19
        if before:
            before(pos, s)
        want = f.frame_count(s)
        assert want == done_at(pos + s) - done_at(pos), (pos, s, want)
        got = f.process_device(din.data_ptr() + size * (shift + pos), s, codes.data_ptr() + 2 * (shift + done * bins),
                               power.data_ptr() + 4 * (shift + done * bins))
        assert got == want
        counts.append(got)
        pos += s
        done += got
    f.synchronize()
    assert pos == n and done == total
    hc = codes.cpu().numpy().view(np.uint16)
    hp = power.cpu().numpy()
    end = shift + total * bins
    assert np.all(hc[end:] == SENTINEL_CODE) and np.all(hc[:shift] == SENTINEL_CODE), "a guard around the codes was written"
    assert np.all(hp[end:] == SENTINEL) and np.all(hp[:shift] == SENTINEL), "a guard around the power was written"
    return hc[shift:end].reshape(total, bins), hp[shift:end].reshape(total, bins), counts


# ---- 1. a long frame is the float32 sum, in chunk order, of its chunk sums -----------------------------------------------------
ONES = [(256, 1, 65528, False, None), (256, 1, 65535, False, None), (256, 1, 65535, True, None), (1024, 3, 8200, True, (-459, 918)),
        (512, 2, 1003, False, None), (4096, 1, 4104, True, None)]


@pytest.mark.gpu
@pytest.mark.parametrize("N,H,K,i16,span", ONES)
def test_long_frame_is_the_chunk_order_sum(gpu_ok, fir, torch_cuda, N, H, K, i16, span):
    """context A (N, H, K) against the model of psd_ref.chunk_order_power over the chunk sums that contexts of 8 and of 1
    segments per frame give exactly; A fed whole and in three calls, which start at chunk indices in the hundreds or thousands"""
    first, bins = span or (-N // 2, N)
    n = (K - 1) * H + N + 10 * H             # one frame and 10 segments
    raw, _ = signal(n, N, i16)
    ones = np.ones(N, dtype=np.float32)
    fmt = fir.INPUT_I16 if i16 else fir.INPUT_F32
    ref_power = 0.01
    make = lambda k: fir.IfFirPsd(N, H, k, first, bins, ref_power=ref_power, window=ones, input_format=fmt, max_samples=n)
    full, short = K // 8, K % 8
    with make(8) as b:
        _, pb, _ = run_device(torch_cuda, b, raw, [n], i16)
    pb = pb[:full]
    assert pb.shape == (full, bins) and pb.min() >= TINY, "a chunk sum is zero or subnormal: the scaling back is not exact"
    chunks = [pb * np.float32(8 * N)]
    if short:
        # the short last chunk: its segments one by one from a context of 1 segment per frame (scale 2^-log2 N, exact), added in
        # segment order; the context of `short` segments per frame on the same samples is that sum, scaled once
        tail = raw[2 * (K - short) * H:]
        with make(1) as s1:
            _, p1, _ = run_device(torch_cuda, s1, tail, [tail.size // 2], i16)
        p1 = p1[:short]
        assert p1.shape == (short, bins) and p1.min() >= TINY
        last = psd_ref.segment_order_sum(p1 * np.float32(N))
        with make(short) as c:
            _, pc, _ = run_device(torch_cuda, c, tail, [tail.size // 2], i16)
        assert same_bits(pc[0], last * np.float32(1.0 / (float(short) * N)))
        chunks.append(last[None])
    want = psd_ref.chunk_order_power(np.concatenate(chunks), K, N)
    with make(K) as a:
        codes, power, counts = run_device(torch_cuda, a, raw, [n], i16)
        assert counts == [1] and power.shape == (1, bins)
        wrong = np.flatnonzero(power[0].view(np.uint32) != want.view(np.uint32))
        assert wrong.size == 0, "%d of %d bins are not the chunk-order sum, the first at %d: %r for %r" % (
            wrong.size, bins, wrong[0], power[0][wrong[0]], want[wrong[0]])
        check_codes(codes, power, ref_power)
        a.reset()
        cuts = [n // 3, 2 * n // 3 - n // 3, n - 2 * n // 3]
        c3, p3, counts = run_device(torch_cuda, a, raw, cuts, i16)
        assert counts == [0, 0, 1]
        assert same_bits(p3, power) and same_bits(c3, codes)


# ---- 2. long averages against float64 --------------------------------------------------------------------------------------------
def long_cases():
    return [(N, H, K, i16, w) for (N, H, K) in psd_ref.LONG for i16 in (False, True) for w in ("hann", "asymmetric")]


@pytest.mark.gpu
@pytest.mark.parametrize("N,H,K,i16,window", long_cases())
def test_long_averages_against_float64(gpu_ok, fir, torch_cuda, N, H, K, i16, window):
    """one call at the default launch (8000 chunks and more at the first shape: the chunk kernel's stride loop turns on any chip); the
    measured errors are in profiles/r23_psd_long_accuracy.txt"""
    n = psd_ref.long_samples(N, H, K)
    raw, _ = signal(n, N, i16)
    ref = reference(n, N, H, K, i16, window)
    assert ref.shape[0] == 1
    ref_power = 0.01
    with fir.IfFirPsd(N, H, K, -N // 2, N, ref_power=ref_power, window=window_of(window, N),
                      input_format=fir.INPUT_I16 if i16 else fir.INPUT_F32, max_samples=n) as f:
        codes, power, counts = run_device(torch_cuda, f, raw, [n], i16)
    err = frame_errors(power, ref)
    eps = psd_ref.eps_of(K)
    print("LONG N=%d H=%d K=%d i16=%d %s: frame error %.4g of the peak (eps_of(K) %.4g, old EPS %.4g%s)"
          % (N, H, K, i16, window, err.max(), eps, EPS, ": above the old EPS" if err.max() > EPS else ""))
    assert counts == [1] and np.all(err <= eps), err
    check_codes(codes, power, ref_power)


# ---- 3. grid limits ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("i16", [False, True])
@pytest.mark.parametrize("N,H", [(256, 1), (512, 192), (1024, 385), (2048, 2048), (4096, 4095)])
def test_grid_limits_keep_the_bits(gpu_ok, fir, torch_cuda, N, H, i16):
    """one and two workgroups walk the call's 6 chunks: a workgroup's second and later chunks, in each of the chunk kernel's 10
    instantiations, give the bits of the default launch, which is held to the float64 reference"""
    K = 20
    n = psd_ref.matrix_samples(N, H, K)
    raw, _ = signal(n, N, i16)
    ref = reference(n, N, H, K, i16, "hann")
    with fir.IfFirPsd(N, H, K, -N // 2, N, ref_power=0.01, input_format=fir.INPUT_I16 if i16 else fir.INPUT_F32, max_samples=n,
                      dev=True) as f:
        assert f.debug_plan(n)[1] >= 6
        codes, power, counts = run_device(torch_cuda, f, raw, [n], i16)
        assert counts == [ref.shape[0]] and ref.shape[0] >= 2 and np.all(frame_errors(power, ref) <= EPS)
        for limit in (1, 2):
            f.reset()
            f.debug_config(grid_limit=limit)
            c, p, _ = run_device(torch_cuda, f, raw, [n], i16)
            assert same_bits(p, power) and same_bits(c, codes), limit
        f.reset()
        f.debug_config(grid_limit=0)
        c, p, _ = run_device(torch_cuda, f, raw, [n], i16)
        assert same_bits(p, power) and same_bits(c, codes)


# ---- 4. many frames in one call ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("N,H,K,first,bins,frames,i16", [(1024, 1, 1, -459, 918, 3000, False), (256, 1, 3, -128, 256, 2000, True),
                                                         (512, 64, 2, -256, 300, 500, False)])
def test_many_frames_in_one_call(gpu_ok, fir, torch_cuda, N, H, K, first, bins, frames, i16):
    """the frame kernel's (frame, bin) split with thousands of frames and a bin count that divides nothing"""
    n = (frames * K - 1) * H + N + H // 2
    raw, x = signal(n, N, i16)
    ref = psd_ref.power_f64(x, N, H, K, None, first, bins)
    peak = np.max(psd_ref.power_f64(x, N, H, K), axis=1)
    assert ref.shape == (frames, bins)
    with fir.IfFirPsd(N, H, K, first, bins, ref_power=0.01, input_format=fir.INPUT_I16 if i16 else fir.INPUT_F32, max_samples=n) as f:
        codes, power, counts = run_device(torch_cuda, f, raw, [n], i16)
        assert counts == [frames]
        err = np.max(np.abs(power - ref), axis=1) / peak
        print("N=%d H=%d K=%d %d frames: worst frame error %.3g of the peak (EPS %.3g)" % (N, H, K, frames, err.max(), EPS))
        assert not np.any(np.isnan(power)) and np.all(err <= psd_ref.eps_of(K)) and psd_ref.eps_of(K) == EPS
        check_codes(codes, power, 0.01)
        f.reset()
        pieces = [n // 7 + 3, 0, n // 3 + 1, N // 2 - 1]
        pieces.append(n - sum(pieces))
        c, p, counts = run_device(torch_cuda, f, raw, pieces, i16)
        assert sum(counts) == frames and counts[1] == 0 and max(counts) > frames // 4
        assert same_bits(p, power) and same_bits(c, codes)


# ---- 5. seek -------------------------------------------------------------------------------------------------------------------------
def frame_boundary_past(limit, N, H, K):
    """m K H just past `limit`, neither a power of two nor a multiple of N"""
    m = limit // (K * H) + 1
    while (m * K * H) % N == 0 or (m * K * H) & (m * K * H - 1) == 0:
        m += 1
    assert limit < m * K * H < limit + 4 * K * H
    return m * K * H


@pytest.mark.gpu
@pytest.mark.parametrize("N,H,K", [(256, 100, 3), (1024, 385, 9)])
def test_seek_to_a_frame_boundary(gpu_ok, fir, torch_cuda, N, H, K):
    n = (3 * K + 2) * H + N + 11
    raw, _ = signal(n, N, False)
    lists = ([n],) + cut_lists(N, H, K, n)
    with fir.IfFirPsd(N, H, K, -N // 2, N, ref_power=0.01, max_samples=n, dev=True) as f:
        fresh = []
        for pieces in lists:
            f.reset()
            fresh.append(feed(torch_cuda, f, raw, pieces))
        assert fresh[0][2] == [psd_ref.frame_count(0, n, N, H, K)] and fresh[0][2][0] >= 3
        for limit in (1 << 32, 1 << 40):
            start = frame_boundary_past(limit, N, H, K)
            for pieces, (codes, power, counts) in zip(lists, fresh):
                f.debug_config(position=start)
                state = {"carried": 0}

                def plan_is_the_reference(pos, s):
                    want = psd_ref.plan(start + pos, state["carried"], s, N, H, K)
                    assert f.debug_plan(s) == want, (start, pos, s)
                    state["carried"] = want[3]
                c, p, got = feed(torch_cuda, f, raw, pieces, before=plan_is_the_reference)
                assert got == counts and same_bits(p, power) and same_bits(c, codes), (start, pieces)


@pytest.mark.gpu
def test_seek_inside_a_frame(gpu_ok, fir, torch_cuda):
    """the stream starts at chunk 5 of a frame of 13 chunks: that frame is the sum of segments 40 .. 99 alone (over K sum w^2), from
    an accumulator of +0, wherever the position is"""
    N, H, K, seg0 = 256, 1, 100, 40
    n = psd_ref.matrix_samples(N, H, K)
    raw, x = signal(n, N, False)
    ref = reference(n, N, H, K, False, "hann").copy()
    ref[0] = psd_ref.power_f64_segments(x, N, H, K, seg0, K)
    tail = raw[2 * seg0 * H:]
    with fir.IfFirPsd(N, H, K, -N // 2, N, ref_power=0.01, max_samples=n, dev=True) as f:
        # a stream first, so that both accumulator buffers hold something the seek has to clear
        f.process(raw[:2 * (N + 30 * H)])
        f.process(raw[:2 * 9 * H])
        f.debug_config(position=seg0 * H)
        assert f.debug_plan(0) == psd_ref.plan(seg0 * H, 0, 0, N, H, K)
        codes, power, counts = feed(torch_cuda, f, tail, [tail.size // 2], seg0=seg0)
        assert counts == [2]
        err = frame_errors(power, ref)
        print("seek to segment %d of %d: frame errors %s (eps_of(K) %.4g)" % (seg0, K, err, psd_ref.eps_of(K)))
        assert np.all(err <= psd_ref.eps_of(K))
        # (the whole first frame is not what is wanted: the partial sum misses it by far more than the tolerance)
        assert np.max(np.abs(power[0] - reference(n, N, H, K, False, "hann")[0])) > 100 * psd_ref.eps_of(K) * np.max(ref[0])
        check_codes(codes, power, 0.01)
        far = seg0 * H + K * H * (1 << 33)
        f.debug_config(position=far)
        pieces = [5 * H + N // 2, 0, 9 * H + 1]
        pieces.append(tail.size // 2 - sum(pieces))
        state = {"carried": 0}

        def plan_is_the_reference(pos, s):
            want = psd_ref.plan(far + pos, state["carried"], s, N, H, K)
            assert f.debug_plan(s) == want, (pos, s)
            state["carried"] = want[3]
        c, p, counts = feed(torch_cuda, f, tail, pieces, seg0=seg0, before=plan_is_the_reference)
        assert sum(counts) == 2 and same_bits(p, power) and same_bits(c, codes)


@pytest.mark.gpu
def test_refused_seeks_and_the_end_of_the_position(gpu_ok, fir, torch_cuda):
    n = 4000
    raw, _ = signal(n, 256, False)
    for (N, H, K), bad in (((256, 100, 3), (50, 100, 200, 301, (1 << 40) + 1)), ((256, 1, 100), (4, 44, 99, 107, 100 * (1 << 33) + 12))):
        with fir.IfFirPsd(N, H, K, -N // 2, N, ref_power=0.01, max_samples=n, dev=True) as f:
            codes, power = f.process(raw)
            f.reset()
            cut = 1001
            head = f.process(raw[:2 * cut])
            plan = f.debug_plan(n - cut)
            for position in bad:
                with pytest.raises(fir.IfFirError, match="if_fir_debug_psd_config: position %d " % position):
                    f.debug_config(position=position)
                assert f.debug_plan(n - cut) == plan
            rest = f.process(raw[2 * cut:])
            assert same_bits(np.concatenate([head[1], rest[1]]), power) and same_bits(np.concatenate([head[0], rest[0]]), codes)
    # a call that would carry the position past 2^64 is refused; the stream goes on and ends as an undisturbed one
    N, H, K = 256, 100, 3
    start = ((1 << 64) - 1000) // (K * H) * (K * H)
    left = (1 << 64) - start
    assert 1000 <= left < 1000 + K * H
    with fir.IfFirPsd(N, H, K, -N // 2, N, ref_power=0.01, max_samples=n, dev=True) as f, \
            fir.IfFirPsd(N, H, K, -N // 2, N, ref_power=0.01, max_samples=n, dev=True) as calm:
        for c in (f, calm):
            c.debug_config(position=start)
        a = f.process(raw[:2 * 600])
        with pytest.raises(fir.IfFirError, match="if_fir_psd_process: sample count too large"):
            f.process(raw[:2 * (left - 600)])
        buf = torch_cuda.zeros(2 * n, dtype=torch_cuda.float32, device="cuda")
        out = torch_cuda.zeros(64 * N, dtype=torch_cuda.int16, device="cuda")
        with pytest.raises(fir.IfFirError, match="if_fir_psd_process_device: sample count too large"):
            f.process_device(buf.data_ptr(), left - 600, out.data_ptr())
        assert f.frame_count(left - 600) == 0
        b = f.process(raw[2 * 600:2 * (left - 1)])   # (to 2^64 - 1: a position of 2^64 itself has no representation)
        want = calm.process(raw[:2 * (left - 1)])
        assert want[0].shape[0] == psd_ref.frame_count(0, left - 1, N, H, K) >= 2
        assert same_bits(np.concatenate([a[1], b[1]]), want[1]) and same_bits(np.concatenate([a[0], b[0]]), want[0])
        calm.reset()
        again = calm.process(raw[:2 * (left - 1)])
        assert same_bits(again[1], want[1]) and same_bits(again[0], want[0])


# ---- 6. pointers off the allocation's grid ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("i16", [False, True])
@pytest.mark.parametrize("N,H,K", [(512, 192, 9), (256, 1, 20)])
def test_pointers_one_element_off(gpu_ok, fir, torch_cuda, N, H, K, i16):
    """the input one sample (8 or 4 bytes), the codes 2 bytes and the power 4 bytes into their allocations, all at once: element
    alignment is all the entry point asks for"""
    n = psd_ref.matrix_samples(N, H, K)
    raw, _ = signal(n, N, i16)
    with fir.IfFirPsd(N, H, K, -N // 2, N, ref_power=0.01, input_format=fir.INPUT_I16 if i16 else fir.INPUT_F32, max_samples=n) as f:
        codes, power, counts = run_device(torch_cuda, f, raw, [n], i16)
        ref = reference(n, N, H, K, i16, "hann")
        assert counts == [ref.shape[0]] and ref.shape[0] >= 2 and np.all(frame_errors(power, ref) <= EPS)
        for pieces in ([n], [n // 3, n - n // 3]):
            f.reset()
            c, p, _ = feed(torch_cuda, f, raw, pieces, i16, shift=1)
            assert same_bits(p, power) and same_bits(c, codes)
