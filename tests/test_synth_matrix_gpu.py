"""The polyphase synthesis bank's two routes at every ring depth, size and run edge (docs/SPEC.md §14), with
the tools of tests/test_synth_gpu.py (one guarded device buffer, sample_count at every step, the float64 fold form).

tests/synth_ref.DEPTH_CASES: per size the J either side of every step of the ring's depth NB = ceil((J-1)/B) + 1, of the plan's
switch between the routes and of the ring's limit, J = 1 (no history, no carry, a ring of one batch) and J = 32, each as a shape
with J terms in every phase and as one whose hop divides nothing and whose J-th term only phase 0 has.  The workspace route
against float64 within SPEC §3 over the whole output, the LDS ring and the host path against its bits.  Then, on one shape per
batch size with J on a step, and on M = 2048 and 4096 at the most their ring holds: the ring taken in one, two and three runs,
streams cut into ragged calls through it, a bin span and frame positions past 2^32.  tests/test_synth_host.py shows on the CPU
that a fault in the ring's index algebra moves these cases."""
import numpy as np
import pytest

import synth_ref
from matrix_util import row_edge_taps
from test_synth_gpu import check, frames_signal, ragged_pieces, reference, run_device, same_bits, stream_frames

PAIRS = tuple((M, J) for M in synth_ref.SIZES for J in synth_ref.DEPTH_J[M])


@pytest.fixture(scope="module")
def torch_cuda(gpu_ok):
    import torch
    torch.cuda.set_device(0)
    return torch


@pytest.mark.gpu
@pytest.mark.parametrize("M,J", PAIRS)
def test_depth_matrix(gpu_ok, fir, oracle, torch_cuda, M, J):
    """both shapes of (M, J), float32 and int16, in two calls: the workspace route within tolerance of float64 over the whole
    output; the ring route, where two workgroups of it fit a CU, the same bits; the route of a fresh context is the ring exactly
    where four fit; the host path on that route the same bits"""
    Synth = fir.IfFirSynth
    for M_, T, L in synth_ref.depth_shapes(M, J):
        assert M_ == M and synth_ref.terms(T, L) == J and (M, T, L) in synth_ref.DEPTH_CASES
        F = stream_frames(M, T, L)
        cut = F // 3 + 1
        ring_fits = synth_ref.lds_route_fits(M, T, L)
        with fir.IfFirSynth(row_edge_taps(T, L, False), M, L, max_frames=F, dev=True) as f:
            plan = f.debug_config()
            assert plan == (Synth.ROUTE_LDS if synth_ref.lds_route_fits(M, T, L, 4) else Synth.ROUTE_WORKSPACE)
            for i16 in (False, True):
                raw, _ = frames_signal(oracle, F, M, i16)
                f.set_input_format(fir.INPUT_I16 if i16 else fir.INPUT_F32)
                assert f.debug_config(route=Synth.ROUTE_WORKSPACE) == Synth.ROUTE_WORKSPACE
                f.reset()
                y, _ = run_device(torch_cuda, f, raw, [cut, F - cut])
                # (a reference of this list is used once: the function without its cache)
                ref = reference.__wrapped__(M, T, L, i16, F)
                assert y.shape == ref.shape == (F * L,)
                check(oracle, y, ref, "depth M=%d J=%d T=%d L=%d i16=%d" % (M, J, T, L, i16))
                if ring_fits:
                    assert f.debug_config(route=Synth.ROUTE_LDS) == Synth.ROUTE_LDS
                    f.reset()
                    ring, _ = run_device(torch_cuda, f, raw, [cut, F - cut])
                    assert same_bits(ring, y), ("ring", T, L, i16)
                else:
                    with pytest.raises(fir.IfFirError, match="route 2"):
                        f.debug_config(route=Synth.ROUTE_LDS)
                assert f.debug_config() == plan
                f.reset()
                host = np.concatenate([f.process(raw[:2 * cut * M]), f.process(raw[2 * cut * M:])]).view(np.complex64)
                assert same_bits(host, y), ("host", T, L, i16)


def run_frames(M, T, L):
    """frames of a call whose batch count is the first from 3 J + 2 on that neither 2 nor 3 divides, with one frame in the last
    batch: two and three runs are unequal, and the last batch is ragged where a batch has several frames"""
    B, batches = synth_ref.batch(M), 3 * synth_ref.terms(T, L) + 2
    while batches % 2 == 0 or batches % 3 == 0:
        batches += 1
    return (batches - 1) * B + 1


@pytest.mark.gpu
@pytest.mark.parametrize("M,T,L", synth_ref.RING_STEP_CASES)
def test_runs_through_the_ring(gpu_ok, fir, oracle, torch_cuda, M, T, L):
    """the ring route with the launcher's own grid (a batch a run) and with 1, 2 and 3 workgroups (the call in one, two and
    three runs, each with its warm-up), float32 and int16: the bits of the workspace route's default launch, which is held to
    float64"""
    F, B = run_frames(M, T, L), synth_ref.batch(M)
    batches = -(-F // B)
    assert batches % 2 and batches % 3 and batches > 3 * synth_ref.terms(T, L) and (B == 1 or F % B) and F * L > 3 * 256
    with fir.IfFirSynth(row_edge_taps(T, L, False), M, L, max_frames=F, dev=True) as f:
        for i16 in (False, True):
            raw, _ = frames_signal(oracle, F, M, i16)
            f.set_input_format(fir.INPUT_I16 if i16 else fir.INPUT_F32)
            assert f.debug_config(route=fir.IfFirSynth.ROUTE_WORKSPACE) == fir.IfFirSynth.ROUTE_WORKSPACE
            f.reset()
            want, _ = run_device(torch_cuda, f, raw, [F])
            check(oracle, want, reference(M, T, L, i16, F), "runs M=%d T=%d L=%d i16=%d" % (M, T, L, i16))
            for limit in (0, 1, 2, 3):
                assert f.debug_config(grid_limit=limit, route=fir.IfFirSynth.ROUTE_LDS) == fir.IfFirSynth.ROUTE_LDS
                f.reset()
                y, _ = run_device(torch_cuda, f, raw, [F])
                assert same_bits(y, want), (i16, limit)


@pytest.mark.gpu
@pytest.mark.parametrize("M,T,L", synth_ref.RING_STEP_CASES)
def test_cuts_through_the_ring(gpu_ok, fir, oracle, torch_cuda, M, T, L):
    """the ring route fed ragged pieces -- calls of 0 and 1 frame first (with J = 1 there is no history to carry them), pieces
    shorter and longer than the history, calls of B - 1, B and B + 1 frames -- with the input format changed between them,
    against one call: the same bits"""
    J, B = synth_ref.terms(T, L), synth_ref.batch(M)
    F = stream_frames(M, T, L) + 2 * J + 20 + 3 * B
    xi, _ = frames_signal(oracle, F, M, True)
    xf = xi.astype(np.float32) * np.float32(2.0 ** -15)
    pieces = ragged_pieces(F - 3 * B, J, np.random.default_rng([M, T, L]))
    pieces = pieces[:11] + [B - 1, B, B + 1] + pieces[11:]
    assert sum(pieces) == F and pieces[:3] == [0, 1, 1]
    formats = [(fir.INPUT_F32, fir.INPUT_I16)[(k // 2) % 2] for k in range(len(pieces))]
    with fir.IfFirSynth(row_edge_taps(T, L, False), M, L, max_frames=F, dev=True) as f:
        assert f.debug_config(route=fir.IfFirSynth.ROUTE_LDS) == fir.IfFirSynth.ROUTE_LDS
        one, _ = run_device(torch_cuda, f, xf, [F])
        check(oracle, one, reference(M, T, L, True, F), "ring cuts M=%d T=%d L=%d" % (M, T, L))
        f.reset()
        y, counts = run_device(torch_cuda, f, {fir.INPUT_F32: xf, fir.INPUT_I16: xi}, pieces, formats=formats)
        assert counts[0] == 0 and 0 in counts[1:] and L in counts and max(counts) > L and {B * L, (B + 1) * L} <= set(counts)
        assert same_bits(y, one)
        f.reset()
        f.set_input_format(fir.INPUT_I16)
        y, _ = run_device(torch_cuda, f, xi, [F])
        assert same_bits(y, one)


@pytest.mark.gpu
def test_a_bin_span_through_the_ring_at_2048(gpu_ok, fir, oracle, torch_cuda):
    """(2048, J = 3), the most the ring holds at that size: a span around DC and one across M - 1 -> 0 against the full-width
    call whose other channels hold +0, both through the ring: the same bits; the first against float64"""
    M, T, L = synth_ref.depth_shapes(2048, 3)[0]
    F = stream_frames(M, T, L)
    taps = row_edge_taps(T, L, False)
    for first_bin, bins in ((-3, 7), (M - 1, 2)):
        raw, _ = frames_signal(oracle, F, bins, False)
        full = np.zeros((F, M, 2), dtype=np.float32)
        full[:, synth_ref.channels(M, first_bin, bins)] = raw.reshape(F, bins, 2)
        with fir.IfFirSynth(taps, M, L, first_bin=first_bin, bins=bins, max_frames=F, dev=True) as f:
            assert f.debug_config(route=fir.IfFirSynth.ROUTE_LDS) == fir.IfFirSynth.ROUTE_LDS
            y, _ = run_device(torch_cuda, f, raw, [F // 2, F - F // 2])
        with fir.IfFirSynth(taps, M, L, max_frames=F, dev=True) as f:
            assert f.debug_config(route=fir.IfFirSynth.ROUTE_LDS) == fir.IfFirSynth.ROUTE_LDS
            want, _ = run_device(torch_cuda, f, full.reshape(-1), [F])
        assert same_bits(y, want), (first_bin, bins)
        if bins == 7:
            check(oracle, y, reference(M, T, L, False, F, 0, first_bin, bins), "ring span M=%d first=%d bins=%d" % (M, first_bin, bins))


@pytest.mark.gpu
@pytest.mark.parametrize("start", [(1 << 32) - 5, (1 << 40) + 12345])
def test_frame_positions_past_2_32_without_a_history(gpu_ok, fir, oracle, torch_cuda, start):
    """(2048, T = L = 2047): J = 1, and the hop is no divisor of M, so the first output of frame `start` is no multiple of M.
    Both routes (the ring is the plan's own here), float32 and int16: the reference evaluated at that position, a cut (across
    frame 2^32 for the first start) the same bits, position 0 other values"""
    M, T, L = synth_ref.depth_shapes(2048, 1)[1]
    assert (T, L) == (2047, 2047) and (start * L) % M and synth_ref.lds_route_fits(M, T, L, 4)
    F = stream_frames(M, T, L) + 6
    assert F > 6     # the cut's pieces: 3, 2, 1 and the rest
    for i16 in (False, True):
        raw, _ = frames_signal(oracle, F, M, i16)
        ref = reference(M, T, L, i16, F, start)
        with fir.IfFirSynth(row_edge_taps(T, L, False), M, L, max_frames=F, dev=True) as f:
            if i16:
                f.set_input_format(fir.INPUT_I16)
            assert f.debug_config() == fir.IfFirSynth.ROUTE_LDS
            for route in (fir.IfFirSynth.ROUTE_LDS, fir.IfFirSynth.ROUTE_WORKSPACE):
                assert f.debug_config(route=route, position=start) == route
                assert f.sample_count(F) == F * L
                one, _ = run_device(torch_cuda, f, raw, [F])
                check(oracle, one, ref, "position J=1 route=%d start=%d i16=%d" % (route, start, i16))
                f.debug_config(route=route, position=start)
                y, _ = run_device(torch_cuda, f, raw, [3, 2, 1, F - 6])
                assert same_bits(y, one)
                f.reset()
                zero, _ = run_device(torch_cuda, f, raw, [F])
                assert not np.array_equal(zero, one)
