"""The rational resampler (if_fir_resamp_t, docs/SPEC.md §7) on the GPU against the float64 reference of tests/resamp_ref.py,
SPEC §3 tolerance; stream cuts, tile and grid edges bit for bit.  Device output buffers carry a sentinel guard behind their
last sample, and the guard is checked."""
import functools

import numpy as np
import pytest

import resamp_ref

TOL = 1e-6
GUARD = 64          # float32 words behind the last output
SENTINEL = 12345.0
# (L, M, T): ratios above and below 1, a common factor, plain decimator / interpolator / filter, long phase rows, the longest
# filter, T < L (phases without a tap), a call that emits fewer outputs than one period, a single tap
MATRIX = ((3, 2, 95), (2, 3, 63), (5, 7, 255), (4, 6, 33), (1, 4, 255), (4, 1, 255), (1, 1, 31), (64, 63, 1537), (63, 64, 1537),
          (64, 1, 4096), (4, 3, 4096), (1, 3, 1023), (7, 5, 3), (3, 64, 100), (5, 2, 1))


@pytest.fixture(scope="module")
def torch_cuda(gpu_ok):
    import torch
    torch.cuda.set_device(0)
    return torch


def taps_for(fir, T, L, M, complex_taps):
    """image-rejection low-pass of gain L, cut-off 0.45 / max(L, M) (complex: the shifted design).  if_bpf_design makes odd
    lengths >= 3: an even T is the design of T - 1 taps plus a last tap of an eighth of the centre tap, negated (the last tap
    index is then met by a value that matters, not by a window's zero), T = 1 is the single tap L."""
    w = max(L, M)
    odd = T if T % 2 else T - 1
    if odd < 3:
        h = np.array([L, 0.5 * L] if complex_taps else [L], dtype=np.float32)
    elif complex_taps:
        h = (fir.bpf_design_complex(odd, 0.1 / w, 0.8 / w) * np.float32(L)).astype(np.float32)
    else:
        h = (fir.bpf_design(odd, 0.0, 0.45 / w) * np.float32(L)).astype(np.float32)
    if odd >= 3 and odd != T:
        width = 2 if complex_taps else 1
        mid = h[(odd // 2) * width:(odd // 2) * width + width]
        h = np.concatenate([h, -mid / np.float32(8)]).astype(np.float32)
    assert h.size == T * (2 if complex_taps else 1)
    return h


@functools.lru_cache(maxsize=None)
def signal(n, i16):
    """(what the context is fed, the same samples as float32)"""
    import __graft_entry__ as g
    x = g.load_oracle().synth_iq(n, channel=3)
    if i16:
        xi = np.clip(np.round(x * 14000.0), -32768, 32767).astype(np.int16)
        return xi, xi.astype(np.float32) * np.float32(2.0 ** -15)
    return x, x


@functools.lru_cache(maxsize=None)
def reference(fir, L, M, T, ct, i16, n):
    ref = resamp_ref.resample_f64(taps_for(fir, T, L, M, ct), signal(n, i16)[1], L, M, ct)
    ref.setflags(write=False)
    return ref


def cases():
    """every ratio with {real, complex} taps x {float32, int16}: each row meets all four kernel instantiations"""
    return [(L, M, T, ct, i16) for (L, M, T) in MATRIX for ct in (False, True) for i16 in (False, True)]


def run_device(torch, f, raw, pieces, i16):
    """feed `raw` from ONE device buffer in consecutive pieces (sample-aligned offsets); returns (outputs, counts)"""
    n = raw.size // 2
    din = torch.from_numpy(np.ascontiguousarray(raw)).cuda()
    total = resamp_ref.out_count(0, n, f.interpolation, f.decimation)
    buf = torch.full((2 * total + GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
    in_bytes = 4 if i16 else 8
    pos = done = 0
    counts = []
    for s in pieces:
        want = f.out_count(s)
        got = f.process_device(din.data_ptr() + in_bytes * pos, buf.data_ptr() + 8 * done, s)
        assert got == want == resamp_ref.out_count(pos, s, f.interpolation, f.decimation), (pos, s, got, want)
        counts.append(got)
        pos += s
        done += got
    f.synchronize()
    assert pos == n and done == total
    h = buf.cpu().numpy()
    assert np.all(h[2 * total:] == SENTINEL), "the guard behind the last output was written"
    return h[:2 * total], counts


@pytest.mark.gpu
@pytest.mark.parametrize("L,M,T,ct,i16", cases())
def test_matrix_against_float64(gpu_ok, fir, oracle, torch_cuda, L, M, T, ct, i16):
    n = 60_000
    raw, _ = signal(n, i16)
    ref = reference(fir, L, M, T, ct, i16, n)
    with fir.IfFirResamp(taps_for(fir, T, L, M, ct), L, M, max_samples=n, complex_taps=ct) as f:
        if i16:
            f.set_input_format(fir.INPUT_I16)
        cut = n // 3
        y = np.concatenate([f.process(raw[:2 * cut]), f.process(raw[2 * cut:])])
        f.reset()
        yd, _ = run_device(torch_cuda, f, raw, [cut, n - cut], i16)
    assert y.size == ref.size == 2 * resamp_ref.out_count(0, n, L, M)
    l2, mx = oracle.err_metrics(y, ref)
    print("L=%d M=%d T=%d complex=%d i16=%d: l2=%.3g max=%.3g" % (L, M, T, ct, i16, l2, mx))
    assert l2 <= TOL and mx <= TOL, (l2, mx)
    assert np.array_equal(yd, y)


@pytest.mark.gpu
@pytest.mark.parametrize("L,M", [(3, 2), (2, 3), (5, 7), (63, 64)])
def test_split_invariance_bit_for_bit(gpu_ok, fir, torch_cuda, L, M):
    n, T = 20_011, 255
    x, _ = signal(n, False)
    taps = taps_for(fir, T, L, M, False)
    sizes = [1, 2, 0, M - 1, L, 4097]
    sizes.append(n - sum(sizes))
    with fir.IfFirResamp(taps, L, M, max_samples=n) as f:
        assert f.out_count(n) == resamp_ref.out_count(0, n, L, M)
        one = f.process(x)
        f.reset()
        parts, pos = [], 0
        for s in sizes:
            want = f.out_count(s)
            parts.append(f.process(x[2 * pos:2 * (pos + s)]))
            assert parts[-1].size == 2 * want
            pos += s
        assert np.array_equal(np.concatenate(parts), one)
        f.reset()
        y, counts = run_device(torch_cuda, f, x, sizes, False)
        assert sum(counts) == -(-n * L // M) and counts[2] == 0
        assert np.array_equal(y, one)


@pytest.mark.gpu
@pytest.mark.parametrize("L,M,T", [(3, 2, 95), (5, 7, 255), (1, 3, 1023)])
def test_tile_and_grid_edges(gpu_ok, fir, torch_cuda, L, M, T):
    """output counts one less than, equal to and one more than 1 tile and 5 tiles (from a reset, L > M reaches only the counts
    ceil(n L / M): the next one up then stands in); the grid capped to 1 and to 3 workgroups gives the bits of the uncapped run"""
    taps = taps_for(fir, T, L, M, False)
    with fir.IfFirResamp(taps, L, M, max_samples=1 << 16, dev=True) as f:
        tile = f.tile_outputs()
        assert tile > 0 and tile % L == 0
        n_for = lambda outs: (outs - 1) * M // L + 1          # the fewest inputs that emit `outs` outputs
        n_max = n_for(5 * tile + 1)
        seen = set()
        x, _ = signal(n_max, False)
        ref_all = resamp_ref.resample_f64(taps, x, L, M)
        for want in (tile - 1, tile, tile + 1, 5 * tile - 1, 5 * tile, 5 * tile + 1):
            n = n_for(want)
            outs = resamp_ref.out_count(0, n, L, M)
            assert want <= outs < want + -(-L // M)
            seen.add(outs - want)
            runs = []
            for limit in (0, 1, 3):
                f.debug_config(grid_limit=limit)
                f.reset()
                y, _ = run_device(torch_cuda, f, x[:2 * n], [n], False)
                runs.append(y)
            assert np.array_equal(runs[0], runs[1]) and np.array_equal(runs[0], runs[2]), outs
            ref = ref_all[:2 * outs]
            assert np.max(np.abs(runs[0] - ref)) <= TOL * np.max(np.abs(ref)), outs
        assert 0 in seen


@pytest.mark.gpu
def test_degenerate_calls(gpu_ok, fir):
    L, M, T, n = 3, 64, 100, 700
    x, _ = signal(n, False)
    with fir.IfFirResamp(taps_for(fir, T, L, M, False), L, M, max_samples=n) as f:
        one = f.process(x)
        assert one.size == 2 * -(-n * L // M)
        f.reset()
        assert f.process(x[:0]).size == 0 and f.out_count(0) == 0
        parts = [f.process(x[2 * i:2 * i + 2]) for i in range(n)]
        assert sum(1 for p in parts if p.size == 0) == n - one.size // 2   # most calls emit nothing
        assert np.array_equal(np.concatenate(parts), one)


@pytest.mark.gpu
@pytest.mark.filterwarnings("ignore:The CUDA Graph is empty")
def test_reset_and_rejected_arguments(gpu_ok, fir, torch_cuda):
    torch = torch_cuda
    n = 10_000
    x, _ = signal(n, False)
    taps = taps_for(fir, 95, 3, 4, False)
    with fir.IfFirResamp(taps, 3, 4, max_samples=n) as f:
        y0 = f.process(x)
        f.process(x[:2 * 1001])
        f.reset()
        assert np.array_equal(f.process(x), y0)
        f.reset()
        f.process(x[:2 * 1001])
        with pytest.raises(fir.IfFirError, match="ullMaxSamples"):
            f.process(np.zeros(2 * (n + 1), dtype=np.float32))
        with pytest.raises(fir.IfFirError, match="format"):
            f.set_input_format(5)
        buf = torch.zeros(2 * n + 8, dtype=torch.float32, device="cuda")
        with pytest.raises(fir.IfFirError, match="aligned"):
            f.process_device(buf.data_ptr() + 4, buf.data_ptr(), 100)
        with pytest.raises(fir.IfFirError, match="aligned"):
            f.process_device(buf.data_ptr(), buf.data_ptr() + 4, 100)
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
        assert np.array_equal(f.process(x[2 * 1001:]), y0[2 * f_count(1001, 3, 4):])
    for T, L, M in ((0, 3, 2), (4097, 3, 2), (31, 0, 2), (31, 65, 2), (31, 3, 0), (31, 3, 65)):
        with pytest.raises(fir.IfFirError) as e:
            fir.IfFirResamp(np.ones(T, dtype=np.float32), L, M)
        assert str(e.value)


def f_count(n, L, M):
    return resamp_ref.out_count(0, n, L, M)


@pytest.mark.gpu
@pytest.mark.parametrize("L,M,T", [(3, 4, 95), (5, 2, 127)])
def test_against_interpolate_then_decimate(gpu_ok, fir, oracle, L, M, T):
    """what users do today: IfFirInterp(h, L), then IfFir([1.0], decimation=M) -- both within SPEC §3 of float64"""
    n = 40_000
    x, _ = signal(n, False)
    taps = taps_for(fir, T, L, M, False)
    ref = resamp_ref.resample_f64(taps, x, L, M)
    with fir.IfFirResamp(taps, L, M, max_samples=n) as f:
        y = f.process(x)
    with fir.IfFirInterp(taps, L, max_samples=n) as up, \
            fir.IfFir(np.ones(1, dtype=np.float32), decimation=M, max_samples=n * L) as down:
        chain = down.process(up.process(x))
    assert y.size == chain.size == ref.size
    for name, got in (("resampler", y), ("chain", chain)):
        l2, mx = oracle.err_metrics(got, ref)
        assert l2 <= TOL and mx <= TOL, (name, l2, mx)
