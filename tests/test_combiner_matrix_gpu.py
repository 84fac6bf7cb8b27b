"""The channel combiner's overlap-save kernel (fir_combiner_kernel<ROWS, I16>, docs/SPEC.md §9) unit by unit against the float64
definition (tests/combiner_ref.py) at SPEC §3's tolerance: every compiled (rows, int16) unit at every L the route takes and at
every tap count either side of an overlap class; the move by G bins at the edges of the split of a phase word, at every L, from
stream position 0 and from one where the blocks' first points are no multiples of 64; call sizes round a block; the number of
workgroups that walk the block loop; the centres changed again and again.  The case lists are combiner_ref's, which
tests/test_combiner_host.py walks on the CPU (the complex64 model under half the bound, the end taps, the faults they notice).
Where two runs must be equal, they are compared bit by bit."""
import numpy as np
import pytest

import combiner_ref as cr
import matrix_util

TAG = "combiner-units"


@pytest.fixture(scope="module")
def torch_cuda(gpu_ok):
    import torch
    torch.cuda.set_device(0)
    return torch


def make(fir, taps, L, centres, ct, n, i16=False, grid_limit=2):
    """a development-library context on the overlap-save route; grid_limit = 2: one workgroup walks several blocks"""
    f = fir.IfFirCombiner(taps, L, centres, max_samples=n, complex_taps=ct, dev=True)
    try:
        assert f.get_backend() == fir.BACKEND_HIP_FFT
        f.debug_config(grid_limit=grid_limit)
        if i16:
            f.set_input_format(fir.INPUT_I16)
    except Exception:
        f.close()
        raise
    return f


def cut(arrs, a, b):
    return [x[2 * a:2 * b] for x in arrs]


def what(L, C, T, ct, i16):
    return "rows=%d i16=%d L=%d C=%d T=%d ct=%d" % (cr.overlap_rows(T), i16, L, C, T, ct)


# ---------------------------------------------------------------- A: every unit, every L, either side of every class

def test_the_boundary_cases_reach_every_unit():
    units, ls, taps, ct_rows = cr.boundary_coverage()
    assert len(cr.boundary_cases()) == 85
    assert units == {(r, a) for r in (4, 8, 16, 32, 48) for a in (False, True)}   # the ten fir_combiner_kernel<ROWS, I16>
    assert ls == {4, 8, 16, 32, 64}
    assert taps == set(cr.BOUNDARY_TAPS)
    assert ct_rows == {4, 8, 16, 32, 48}
    assert [cr.overlap_rows(T) for T in (1, 257, 258, 513, 514, 1025, 1026, 2049, 2050, 3073)] == [4, 4, 8, 8, 16, 16, 32, 32, 48, 48]


@pytest.mark.gpu
@pytest.mark.parametrize("L,C,T,ct,i16", cr.boundary_cases())
def test_boundary_matrix_against_float64(gpu_ok, fir, oracle, L, C, T, ct, i16):
    taps, raw, _, centres, words, ref = cr.case_reference(L, C, T, ct, i16)
    n = raw[0].size // 2
    with make(fir, taps, L, centres, ct, n, i16) as f:
        assert [cr.phase_word(v) for v in f.get_centres()] == words
        y = f.process(raw)
    assert y.size == 2 * n * L
    matrix_util.check(oracle, y, ref, "A " + what(L, C, T, ct, i16), tag=TAG)


# ---------------------------------------------------------------- B: bin moves

@pytest.mark.gpu
@pytest.mark.parametrize("L,C,T,ct,i16", [pytest.param(*c, id=cr.case_id(c)) for c in cr.move_cases()])
def test_bin_moves_against_float64(gpu_ok, fir, oracle, L, C, T, ct, i16):
    """combiner_ref.MOVE_WORDS, given as signed(P) / 2^32: k = (bin - G) & 4095 into the table and, modulo 4096 / L, into the small
    transform, and the block scalar tw[(G n0) & 4095], with G = 0, 1, 2047, 2048, 4095 and residuals 0, +-1, -2^19, 2^19 - 1; all
    the words as the channels of one context (walked by two workgroups from position 0, by the default launch after the seek),
    and each word alone"""
    taps, raw, _, centres, words, ref = cr.case_reference(L, C, T, ct, i16)
    n = raw[0].size // 2
    with make(fir, taps, L, centres, ct, n, i16, grid_limit=0 if C.seek else 2) as f:
        assert [cr.phase_word(v) for v in f.get_centres()] == words == list(C)
        if C.seek:
            f.debug_seek(C.seek)
        y = f.process(raw)
    assert y.size == 2 * n * L
    matrix_util.check(oracle, y, ref, "B rows=%d L=%d T=%d %s from %d" % (cr.overlap_rows(T), L, T, "all words" if len(C) > 1 else
                                                                          "word %#x" % C[0], C.seek), tag=TAG)


# ---------------------------------------------------------------- C: block edges

# (rows, L, complex taps, int16): the longest filter of each rows class, every L once, float32 and int16 in turn
EDGE_SHAPES = [(4, 64, False, False), (8, 32, True, True), (16, 4, True, False), (32, 8, False, True), (48, 16, True, False)]
EDGE_CENTRES = (37.0 / 4096, 0.2003)   # one on the grid with G != 0, one off it


def edge_sizes(a_in):
    return (1, 2, a_in - 1, a_in, a_in + 1, 2 * a_in, 2 * a_in + 1, 3 * a_in - 1)


@pytest.mark.gpu
@pytest.mark.parametrize("rows,L,ct,i16", EDGE_SHAPES)
def test_single_calls_round_a_block(gpu_ok, fir, oracle, torch_cuda, rows, L, ct, i16):
    """one call of n samples after a reset, n round the samples a block advances by (a_in = (4096 - 64 rows) / L); for
    n = a_in + 1 and 3 a_in - 1 also through device pointers into a buffer with a guard of 12345.0 before the first output and
    behind the last"""
    torch = torch_cuda
    T = cr.ROWS_TAPS[rows]
    assert cr.overlap_rows(T) == rows and T - 1 == 64 * rows
    a_in = (4096 - 64 * rows) // L
    pad = 4096
    taps = matrix_util.edge_taps(T, L, ct)
    raw, xs = cr.signals(oracle, 3 * a_in, 2, i16)
    words = [cr.phase_word(v) for v in EDGE_CENTRES]
    with make(fir, taps, L, EDGE_CENTRES, ct, 3 * a_in, i16) as f:
        for n in edge_sizes(a_in):
            ref = cr.reference(taps, cut(xs, 0, n), L, words, ct)
            f.reset()
            y = f.process(cut(raw, 0, n))
            assert y.size == 2 * n * L
            matrix_util.check(oracle, y, ref, "C rows=%d i16=%d L=%d n=%d" % (rows, i16, L, n), tag=TAG)
            if n in (a_in + 1, 3 * a_in - 1):
                f.reset()
                dins = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in cut(raw, 0, n)]
                buf = torch.full((2 * (n * L + 2 * pad),), 12345.0, dtype=torch.float32, device="cuda")
                assert f.process_device([d.data_ptr() for d in dins], buf.data_ptr() + 8 * pad, n) == n * L
                f.synchronize()
                h = buf.cpu().numpy()
                assert np.all(h[:2 * pad] == 12345.0) and np.all(h[-2 * pad:] == 12345.0), (rows, n)
                assert np.array_equal(h[2 * pad:-2 * pad], y), (rows, n)


# ---------------------------------------------------------------- D: launch width

@pytest.mark.gpu
@pytest.mark.parametrize("T,L,i16", [(513, 32, False), (2049, 8, True)])
def test_launch_width_leaves_the_bits_alone(gpu_ok, fir, oracle, T, L, i16):
    """rows 8 and 32, seven blocks and a ragged one: the default launch and 1, 2 and 3 workgroups walking the block loop give
    the same bits -- a block's arithmetic does not depend on which workgroup runs it --, and the default launch is the float64
    reference within the tolerance"""
    C, ct = 3, True
    rows = cr.overlap_rows(T)
    n = -(-(7 * (4096 - 64 * rows) + 517) // L)
    taps = matrix_util.edge_taps(T, L, ct)
    raw, xs = cr.signals(oracle, n, C, i16)
    centres = cr.centres_for(L, C)
    outs = {}
    with make(fir, taps, L, centres, ct, n, i16, grid_limit=0) as f:
        for limit in (0, 1, 2, 3):
            f.reset()
            f.debug_config(grid_limit=limit)
            outs[limit] = f.process(raw)
    for limit in (1, 2, 3):
        assert np.array_equal(outs[limit].view(np.uint32), outs[0].view(np.uint32)), (T, L, limit)
    matrix_util.check(oracle, outs[0], cr.reference(taps, xs, L, [cr.phase_word(v) for v in centres], ct),
                      "D rows=%d i16=%d L=%d C=%d T=%d default launch" % (rows, i16, L, C, T), tag=TAG)


# ---------------------------------------------------------------- F: the centres changed again and again

@pytest.mark.gpu
def test_centres_changed_before_every_call(gpu_ok, fir, oracle):
    """one stream in six calls, new centres before calls 2 to 6: the two device images of the residual tables change hands on
    every change that brings residual tables and stay on one that brings none, and the table count goes 2 -> 5 -> 1 -> 3 -> 3 ->
    (5 ->) 5.  Every call against the float64 reference of the centres then in force, from n = 0 on"""
    L, C, T, ct = 16, 4, 513, True
    taps = matrix_util.edge_taps(T, L, ct)
    n = cr.stream_samples(T, L)
    raw, xs = cr.signals(oracle, n, C, False)
    a_in = (4096 - 64 * cr.overlap_rows(T)) // L
    w = cr.phase_word(0.2003)
    shared = [w, (w + (5 << 20)) % (1 << 32), cr.phase_word(-0.3107), 100 << 20]
    plan = [
        [[0, 37 << 20, w, w]],                                                   # call 1: two on the grid, two on one residual
        [[cr.phase_word(v) for v in cr.centres_for(L, C)]],                      # all off the grid and distinct: five tables
        [[1 << 20, 4095 << 20, 2047 << 20, 1 << 31]],                            # all on the grid: table 0 alone, no new image
        [shared],                                                                # two channels share a residual
        [shared],                                                                # the same centres again
        [[cr.phase_word(v) for v in cr.centres_for(L, C)[::-1] * 0.83 + 0.01],   # two changes in a row: the first is never used
         [(100 << 20) + (1 << 19), (100 << 20) + (1 << 19) - 1, 1, (1 << 32) - 1]],
    ]
    tables = [len({cr.split_word(P)[1] for P in sets[-1]} | {0}) for sets in plan]
    assert tables == [2, 5, 1, 3, 3, 5], tables
    sizes = [a_in + 3, 97, a_in - 1, 1, 60]
    sizes.append(n - sum(sizes))
    assert sizes[-1] > 0
    pos = 0
    with make(fir, taps, L, [cr.word_centre(P) for P in plan[0][0]], ct, n) as f:
        for k, (sets, s) in enumerate(zip(plan, sizes)):
            for words in (sets if k else []):   # (call 1 runs on the centres of the init)
                f.set_centres([cr.word_centre(P) for P in words])
            words = sets[-1]
            assert [cr.phase_word(v) for v in f.get_centres()] == words
            y = f.process(cut(raw, pos, pos + s))
            assert y.size == 2 * s * L
            matrix_util.check(oracle, y, cr.reference(taps, xs, L, words, ct)[2 * pos * L:2 * (pos + s) * L],
                              "F call %d (%d samples, %d tables)" % (k + 1, s, tables[k]), tag=TAG)
            pos += s
    assert pos == n
