"""The channel combiner's host side (no GPU): its C ABI in the header and the libraries, the float64 reference against the
third-party form, the identity the overlap-save route rests on, the host-built multiply tables, a complex64 model of the route
against SPEC §3's bound, the tap-boundary sensitivity of the test matrices, the faults of the route that the boundary and
bin-move cases notice, and the compiled kernels' resources."""
import os
import re
import subprocess

import numpy as np
import pytest

import combiner_ref as cr
import matrix_util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "qo-100-tools_amd", "csrc")
COMBINER_ABI = {"if_fir_combiner_init", "if_fir_combiner_init_complex", "if_fir_combiner_destroy", "if_fir_combiner_reset",
                "if_fir_combiner_set_backend", "if_fir_combiner_get_backend", "if_fir_combiner_set_input_format",
                "if_fir_combiner_set_centres", "if_fir_combiner_get_centres", "if_fir_combiner_set_stream",
                "if_fir_combiner_synchronize", "if_fir_combiner_last_error", "if_fir_combiner_out_count", "if_fir_combiner_process",
                "if_fir_combiner_process_device"}
COMBINER_DEV = {"if_fir_debug_combiner_config", "if_fir_debug_combiner_seek", "if_fir_debug_combiner_tables"}
TOL = 1e-6   # docs/SPEC.md §3
ALL_CASES = cr.cases("fft") + cr.cases("generic")
# the cases of tests/test_combiner_matrix_gpu.py: the boundary matrix (less what the matrix above has already) and the bin moves
BOUNDARY_NEW = [c for c in cr.boundary_cases() if c not in ALL_CASES]
MOVES = [pytest.param(*c, id=cr.case_id(c)) for c in cr.move_cases()]


def _defined(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True).stdout
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


def rel(y, ref):
    """(l2 error over l2 norm, max error over peak) of interleaved arrays, SPEC §3"""
    y, ref = cr.as_c(y), cr.as_c(ref)
    return np.linalg.norm(y - ref) / np.linalg.norm(ref), np.max(np.abs(y - ref)) / np.max(np.abs(ref))


def test_header_declares_and_libraries_export_the_combiner(fir):
    assert hasattr(fir, "IfFirCombiner")
    header = open(os.path.join(ROOT, "include", "if_fir.h")).read()
    declared = set(re.findall(r"\b(if_fir_combiner_[a-z_]+)\s*\(", header))
    assert declared == COMBINER_ABI, declared ^ COMBINER_ABI
    assert "typedef struct if_fir_combiner if_fir_combiner_t;" in header
    assert COMBINER_ABI <= set(fir.EXPORTS) and COMBINER_DEV <= set(fir.DEV_EXPORTS)
    dbg = open(os.path.join(ROOT, "include", "if_fir_debug.h")).read()
    assert COMBINER_DEV <= set(re.findall(r"^\w+ \*?(if_fir_[a-z_]+)\s*\(", dbg, re.M))
    fir.lib()
    product, dev = _defined(fir.LIB_PATH), _defined(fir.DEV_LIB_PATH)
    assert COMBINER_ABI <= product and COMBINER_ABI <= dev
    assert not (COMBINER_DEV & product) and COMBINER_DEV <= dev


@pytest.mark.parametrize("C,L,T,ct", [(8, 16, 255, False), (3, 4, 1023, True), (2, 8, 31, True), (2, 64, 31, False), (5, 3, 100, False)])
def test_reference_is_the_upfirdn_form(fir, oracle, C, L, T, ct):
    assert hasattr(fir, "IfFirCombiner")
    taps = matrix_util.edge_taps(T, L, ct)
    _, xs = cr.signals(oracle, 300, C, False)
    words = [cr.phase_word(f) for f in cr.centres_for(L, C)]
    a, b = cr.reference(taps, xs, L, words, ct), cr.reference_upfirdn(taps, xs, L, words, ct)
    assert np.max(np.abs(a - b)) <= 1e-12 * np.max(np.abs(b))


@pytest.mark.parametrize("P", [cr.phase_word(0.2003), cr.phase_word(-0.3107), (100 << 20) + (1 << 19), (100 << 20) - (1 << 19),
                               (4095 << 20) + 12345, 1 << 31, 777, (1 << 32) - 777])
def test_identity_of_the_overlap_save_route(fir, P):
    """exp(j theta_P n) sum_k h[k] u[n-k] = exp(j 2 pi G n / 4096) sum_k (h[k] exp(j theta_r k)) (u[n-k] exp(j theta_r (n-k)))
    with P = G 2^20 + r, in float64, for off-grid words; r = +-2^19 (both splits of a half-way word) and f = +-0.5 (P = 2^31)"""
    assert hasattr(fir, "IfFirCombiner")
    rng = np.random.default_rng(P % 1000)
    T, n = 300, 5000
    h = rng.standard_normal(T) + 1j * rng.standard_normal(T)
    u = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    lhs = cr.rotation(P, 0, n) * np.convolve(u, h)[:n]
    G, r = cr.split_word(P)
    assert 0 <= G < 4096 and abs(r) <= 1 << 19 and ((G << 20) + r) % (1 << 32) == P
    splits = [(G, r)] + ([((G - 1) % 4096, 1 << 19)] if r == -(1 << 19) else [])
    for G, r in splits:
        k = np.arange(n, dtype=np.float64)
        th = 2 * np.pi * r / 4294967296.0
        rhs = np.exp(2j * np.pi * ((G * np.arange(n)) % 4096) / 4096) * np.convolve(u * np.exp(1j * th * k), h * np.exp(1j * th * k[:T]))[:n]
        assert np.max(np.abs(lhs - rhs)) <= 1e-12 * np.max(np.abs(lhs)), (G, r)
    assert cr.phase_word(0.5) == cr.phase_word(-0.5) == 1 << 31 and cr.split_word(1 << 31) == (2048, 0)


@pytest.mark.parametrize("complex_taps", [False, True])
@pytest.mark.parametrize("centre", [0.0, 37.0 / 4096, 0.2003, -0.3107, 100.5 / 4096, 0.5, -0.5])
def test_host_multiply_tables(fir, complex_taps, centre):
    rng = np.random.default_rng(7)
    T = 1023
    t = rng.standard_normal(2 * T if complex_taps else T).astype(np.float32)
    h = cr.taps_c(t, complex_taps)
    G, r, got = fir.debug_combiner_tables(t, centre, complex_taps)
    assert (G, r) == cr.split_word(cr.phase_word(centre))
    want = cr.table_f64(h, r)
    assert np.max(np.abs(got - want)) <= 1e-6 * np.max(np.abs(want))
    if r == 0:
        assert np.array_equal(got, fir.debug_interp_tables(t, complex_taps))   # on the grid: the interpolator's H
    with pytest.raises(fir.IfFirError):
        fir.debug_combiner_tables(np.ones(3074, dtype=np.float32), centre)
    with pytest.raises(fir.IfFirError):
        fir.debug_combiner_tables(t, 0.6, complex_taps)


def _first_out(L, C):
    return C.seek * L if isinstance(C, cr.Words) else 0


@pytest.mark.parametrize("L,C,T,ct,i16", cr.cases("fft") + BOUNDARY_NEW + MOVES)
def test_complex64_model_stays_under_half_the_bound(fir, L, C, T, ct, i16):
    """a plain single-precision implementation of the route (tests/combiner_ref.py, model_c64) misses the float64 reference by
    less than half of SPEC §3's bound on every overlap-save case of the GPU matrix, of the boundary matrix and of the bin moves"""
    assert hasattr(fir, "IfFirCombiner")
    taps, _, xs, _, words, ref = cr.case_reference(L, C, T, ct, i16)
    l2, mx = rel(cr.model_c64(taps, xs, L, words, ct, first_out=_first_out(L, C)), ref)
    print("combiner-model L=%d C=%s T=%d ct=%d i16=%d l2=%.3g max=%.3g" % (L, C, T, ct, i16, l2, mx))
    assert l2 <= 0.5 * TOL and mx <= 0.5 * TOL, (l2, mx)


@pytest.mark.parametrize("L,n0", [(4, 0), (8, 5 * 3840 - 256), (16, (1 << 32) - 1000), (32, 123456789), (64, (1 << 32) + 4096 * 7 + 64)])
def test_model_of_the_kernel_block_is_the_definition(fir, L, n0):
    """tools/fft_model.py's combiner_block -- the kernel's index algebra: the rotation at the load, the small transform read modulo
    4096/L, the move by G bins into the owning thread's registers, the first inverse pass from the registers -- against the
    definition on one block: positions >= T - 1 are sum_c exp(j theta_P (n0 + p)) (h * u_c)[p]; centres on and off the grid"""
    assert hasattr(fir, "IfFirCombiner")
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import fft_model
    rng = np.random.default_rng(L)
    T = 255
    h = rng.standard_normal(T) + 1j * rng.standard_normal(T)
    words = [cr.phase_word(f) for f in (0.2003, -0.3107, 37.0 / 4096, 100.5 / 4096, 0.5, 0.0)]
    xins = [rng.standard_normal(4096 // L) + 1j * rng.standard_normal(4096 // L) for _ in words]
    want = 0
    for x, P in zip(xins, words):
        u = np.zeros(4096, dtype=np.complex128)
        u[::L] = x
        want = want + cr.rotation(P, n0, 4096) * np.convolve(u, h)[:4096]
    got = fft_model.combiner_block(xins, h, L, words, n0)
    assert np.max(np.abs(got[T - 1:] - want[T - 1:])) <= 1e-11 * np.max(np.abs(want))


def _edge_moves(L, C, T, ct, i16, taps=None):
    """for every channel and for h[0] and h[T-1]: how far the float64 reference moves (l2, relative) when that tap is removed
    from that channel's filter alone: the norm of the channel's own signal through the one-tap filter (the rotation has modulus 1)"""
    base_taps, _, xs, _, words, ref = cr.case_reference(L, C, T, ct, i16)
    h = cr.taps_c(base_taps if taps is None else taps, ct)
    if taps is not None:
        ref = cr.reference(taps, xs, L, words, ct)
    norm = np.linalg.norm(cr.as_c(ref))
    moves = []
    for x in xs:
        for k in sorted({0, T - 1}):
            one = np.zeros(T, dtype=np.complex128)
            one[k] = h[k]
            moves.append(np.linalg.norm(cr.interpolate_f64(one, cr.as_c(x), L)) / norm)
    return moves


@pytest.mark.parametrize("L,C,T,ct,i16", ALL_CASES + BOUNDARY_NEW + MOVES)
def test_edge_taps_of_every_channel_move_the_reference(fir, L, C, T, ct, i16):
    """matrix_util.edge_taps: h[0] or h[T-1] missing from ONE channel's filter moves the reference by about 1 / sqrt(T C), more
    than 1e-4 = 100 x the tolerance, for every channel of every matrix shape: a boundary off by one in any channel fails the
    GPU comparison"""
    assert hasattr(fir, "IfFirCombiner")
    moves = _edge_moves(L, C, T, ct, i16)
    channels = len(C) if isinstance(C, cr.Words) else C
    assert len(moves) == (2 if T > 1 else 1) * channels and min(moves) > 1e-4, min(moves)


def _model_error(case, **fault):
    L, C, T, ct, i16 = case
    taps, _, xs, _, words, ref = cr.case_reference(L, C, T, ct, i16)
    return rel(cr.model_c64(taps, xs, L, words, ct, first_out=_first_out(L, C), **fault), ref)


def test_new_cases_notice_the_faults_they_are_for(fir):
    """model_c64's test-only switches, each one fault of the route's index algebra, push the model more than 100 x the
    tolerance (on both norms) from the float64 reference on the cases of tests/test_combiner_matrix_gpu.py aimed at it:
      - the bins moved by G + 1: every bin-move case, the words alone included;
      - a block kept from one input sample before the overlap (overlap - L): every boundary case whose filter fills its overlap
        (T - 1 = 64 rows), where h[T-1] then wraps onto the block's last sample;
      - one channel multiplied by the table of its neighbour's residual (channel 6, r = 2^19 - 1, with channel 5's r = -2^19):
        every case that carries all the words.
    A block kept from overlap - 1 is no fault and is held to the bound instead: the block's first point is a multiple of 64, so
    the one value h[T-1] reaches across the overlap is a zero between two input samples (L >= 4)."""
    assert hasattr(fir, "IfFirCombiner")
    far = 100 * TOL
    moves = cr.move_cases()
    assert len(moves) == 10 + 2 * len(cr.MOVE_WORDS)
    for case in moves:
        l2, mx = _model_error(case, move_extra=1)
        assert l2 > far and mx > far, (case, l2, mx)
        if len(case[1]) > 1:
            assert cr.split_word(case[1][6])[1] == (1 << 19) - 1 and cr.split_word(case[1][5])[1] == -(1 << 19)
            l2, mx = _model_error(case, table_of=(6, 5))
            assert l2 > far and mx > far, (case, l2, mx)
    full = [c for c in cr.boundary_cases() if c[2] - 1 == 64 * cr.overlap_rows(c[2])]
    assert len(full) == 5 * len(cr.BOUNDARY_L) and {cr.overlap_rows(c[2]) for c in full} == {4, 8, 16, 32, 48}
    for case in full:
        l2, mx = _model_error(case, keep_early=case[0])
        assert l2 > far and mx > far, (case, l2, mx)
        l2, mx = _model_error(case, keep_early=1)
        assert l2 <= 0.5 * TOL and mx <= 0.5 * TOL, (case, l2, mx)


def test_edge_tap_check_fails_on_a_windowed_design(fir):
    """the same check on a windowed low-pass (end taps zero): the reference does not notice the end taps"""
    assert hasattr(fir, "IfFirCombiner")
    L, C, T, ct, i16 = 16, 8, 255, False, False
    windowed = (fir.bpf_design(T, 0.0, 0.45 / L) * np.float32(L)).astype(np.float32)
    assert max(_edge_moves(L, C, T, ct, i16, taps=windowed)) < 1e-4
    assert min(_edge_moves(L, C, T, ct, i16)) > 1e-4


def test_combiner_kernels_use_no_scratch(fir):
    assert hasattr(fir, "IfFirCombiner")
    path = os.path.join(CSRC, "if_fir_combiner.resources.txt")
    assert os.path.exists(path), "build() first: the Makefile writes this file next to if_fir_combiner_r*.o"
    text = open(path).read()
    names = re.findall(r"Function Name: (\S+)", text)
    # 5 overlap lengths x (float32, int16) = 10 instantiations
    assert len(names) == 10 and all("fir_combiner_kernel" in n for n in names), names
    assert re.findall(r"VGPRs Spill: (\d+)", text) == ["0"] * 10
    assert re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", text) == ["0"] * 10
    assert re.findall(r"LDS Size \[bytes/block\]: (\d+)", text) == ["32768"] * 10


def test_host_table_builder_under_sanitizers(fir, tmp_path):
    """csrc/if_fir_combiner_tables.h -- the split of a phase word and the multiply table of a residual, plain C++ -- in a
    stand-alone program compiled with AddressSanitizer + UBSan and run on the CPU over words at the edges of the split, into heap
    buffers of exactly the table's size (tests/c/combiner_tables_asan.cpp)."""
    assert hasattr(fir, "IfFirCombiner")
    exe = str(tmp_path / "combiner_asan")
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-std=c++17", "-Wall", "-I" + CSRC,
                           os.path.join(ROOT, "tests", "c", "combiner_tables_asan.cpp"), "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert run.returncode == 0 and "combiner host tables: clean" in run.stdout, (run.stdout[-2000:], run.stderr[-4000:])
