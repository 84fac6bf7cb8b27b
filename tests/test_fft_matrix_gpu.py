"""The overlap-save decimator and the filter bank (docs/SPEC.md §3) unit by unit: every compiled
instantiation of fir_fft_kernel<rows, DEC4, I16, NCO, CHAN, DECN, ACC> and fir_odd_kernel<F, OVLR, I16, NCO, SUB>, every tap count
either side of an overlap class, every tail a decimation can take, call sizes round a block, pieces shorter than the history,
the block queue on a small grid; and the direct, generic and tap-split kernels on the same taps.  Reference: the float64 oracle
(oracle.fir_f64 / fir_ctaps_f64 / fir_nco_f64) on the float32 samples the library saw; SPEC §3 tolerance.

The taps are tests/matrix_util.py's edge_taps: the first and the last tap are the largest of the set (a windowed design's end
taps are zero and the next ones 1e-6 of the peak, so an overlap one sample short, a history that loses its oldest sample or a
second partition read one sample late stay inside the tolerance with them; test_dropping_an_end_tap_is_loud states the margin).

Section A restates the route of a call (csrc/if_fir_fft_route.h, launch_fft_rows, launch_fft_bank8, launch_fft_odd) in Python,
pins it to the header (tests/c/fft_route_dump.cpp) and to the build (csrc/if_fir_fft.resources.txt): the case lists of sections
B and D reach exactly the 244 + 16 kernels the library compiles.  Those tests need no GPU."""
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from matrix_util import TOL, check, edge_taps, signal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAG = "fft-matrix"
SEG = dict(seg_mode=1, seg_len=32)     # the order model of the direct and the generic kernel
SEG_TAPSPLIT = dict(seg_mode=3, seg_len=32)
NCO_FREQS = (0.37, -0.21, 1 / 4096, -0.4999, 0.123456)
_B = (False, True)


@pytest.fixture(scope="module")
def torch_cuda(gpu_ok):
    import torch
    torch.cuda.set_device(0)
    return torch


# ---------------------------------------------------------------- A: the route of a call, in Python

FFT_N, FFT_PART = 4096, 2048
NO_BANK, BANK_SLOTS, BANK_OWN = 0, 1, 2
FAMILY_NONE, FAMILY_ODD, FAMILY_TWO, FAMILY_ROWS = 0, 1, 2, 3
NOT_SERVED = dict(family=0, rows=0, tail=0, dec4=False, decn=False, nco=False, F=0, sub=0, hist=0)


def fft_two_partitions(T):
    return T > 3073


def fft_odd_tail(T, D):
    """(served, F, sub, dropped rows of the 16): decimation 3, 9, ..., 63 with at most 767 taps"""
    if 3 <= D <= 64 and D % 2 and T >= 1 and not fft_two_partitions(T) and D % 3 == 0:
        need = (T - 1 + 2 + 2) // 3
        ovlr = 2 if need <= 128 else 4 if need <= 256 else 0
        if ovlr:
            return True, 3, D // 3, ovlr
    return False, 1, 1, 0


def fft_overlap_rows(T):
    if fft_two_partitions(T):
        return 32
    return 4 if T - 1 <= 256 else 8 if T - 1 <= 512 else 16 if T - 1 <= 1024 else 32 if T - 1 <= 2048 else 48


def fft_block_advance(T, D):
    odd, F, _, ovlr = fft_odd_tail(T, D)
    if odd:
        return F * (1024 - 64 * ovlr)
    return FFT_N - FFT_PART if fft_two_partitions(T) else FFT_N - 64 * fft_overlap_rows(T)


def fft_bank_tail(D, own):
    if D in (4, 8, 16):
        return D
    if not own or D < 4 or D > 64 or D & 3:
        return 0
    return 16 if D % 16 == 0 else 8 if D % 8 == 0 else 4


def tail_factor(tail, dec4):
    return 16 if tail in (16, 17) else 8 if tail in (8, 9) else 2 if tail in (2, 3) else 4 if dec4 else 1


def tail_has_nco(tail):
    return tail not in (4, 5, 6, 17)


def fft_route(T, D, bank=NO_BANK, nco=False):
    """fft_route(T, D, bank, nco, no_fold = false) of if_fir_fft_route.h"""
    if not (1 <= D <= 64 and 1 <= T <= 4096) or (bank and fft_two_partitions(T)):
        return dict(NOT_SERVED)
    odd, F, sub, ovlr = fft_odd_tail(T, D)
    if not bank and odd:
        return dict(family=FAMILY_ODD, rows=ovlr, tail=0, dec4=False, decn=False, nco=nco, F=F, sub=sub, hist=F * 64 * ovlr)
    two = fft_two_partitions(T)
    r = dict(family=FAMILY_TWO if two else FAMILY_ROWS, rows=fft_overlap_rows(T), decn=False)
    r["hist"] = 2 * FFT_PART if two else 64 * r["rows"]
    if bank:
        own = bank == BANK_OWN
        fb = fft_bank_tail(D, own)
        if not fb or (fb == 4 and nco):
            return dict(NOT_SERVED)
        r["tail"] = (17 if own else 16) if fb == 16 else 8 if fb == 8 else 4 if not own else 5 if D == 4 else 6
        r["nco"] = nco and tail_has_nco(r["tail"])
        r["dec4"] = True
    else:
        F = 4 if D % 4 == 0 else 2 if D % 2 == 0 else 1
        r["tail"] = (0 if D == 4 else 1) if F == 4 else (2 if D == 2 else 3) if F == 2 else 0
        r["dec4"] = F > 1
        r["decn"] = F == 1 and D != 1
        r["nco"] = nco
    r["F"] = tail_factor(r["tail"], r["dec4"])
    r["sub"] = D // r["F"]
    return r


def bank8_plan(slots, all_slots_available=True):
    """fft_bank8_plan: (mask of the even slots' all-slots launch, of the odd slots', bit c: channel c left per channel)"""
    seen, m, npar, dup = 0, [0, 0], [0, 0], False
    for s in slots:
        s &= 15
        dup = dup or bool((seen >> s) & 1)
        seen |= 1 << s
        m[s & 1] |= 1 << s
        npar[s & 1] += 1
    pmask = [m[p] if (all_slots_available and not dup and npar[p] >= 4) else 0 for p in (0, 1)]
    rest = sum(1 << c for c, s in enumerate(slots) if not (pmask[s & 1] >> (s & 15)) & 1)
    return pmask[0], pmask[1], rest


def route_line(T, D, bank, nco):
    r = fft_route(T, D, bank, nco)
    odd, oF, oSub, oOvlr = fft_odd_tail(T, D)
    return ("R %d %d %d %d: family %d rows %d tail %d dec4 %d decn %d nco %d F %d sub %d hist %d | odd %d %d %d %d | rows %d advance %d "
            "bank_tail %d %d" % (T, D, bank, nco, r["family"], r["rows"], r["tail"], r["dec4"], r["decn"], r["nco"], r["F"], r["sub"], r["hist"],
                                 odd, oF, oSub, oOvlr, fft_overlap_rows(T), fft_block_advance(T, D), fft_bank_tail(D, False),
                                 fft_bank_tail(D, True)))


def single_units(T, D, i16, nco):
    """the kernels a single-channel call launches: ("odd", F, OVLR, I16, NCO, SUB) or ("fft", rows, DEC4, I16, NCO, CHAN, DECN, ACC)"""
    r = fft_route(T, D, NO_BANK, nco)
    assert r["family"] != FAMILY_NONE, (T, D)
    if r["family"] == FAMILY_ODD:                                           # launch_fft_odd
        return {("odd", r["F"], r["rows"], i16, nco, r["sub"] > 1)}
    units = {("fft", r["rows"], r["dec4"], i16, r["nco"], r["tail"], r["decn"], False)}         # launch_fft_rows / launch_fft_partition<false>
    if r["family"] == FAMILY_TWO:
        units.add(("fft", r["rows"], r["dec4"], i16, r["nco"], r["tail"], r["decn"], True))     # launch_fft_partition<true>
    return units


def bank_units(T, D, own, slots, nco, i16):
    """the kernels a filter-bank call launches (launch_fft_rows, launch_fft_bank8): one; two at decimation 8 on the slot grid when an all-slots launch leaves channels over"""
    r = fft_route(T, D, BANK_OWN if own else BANK_SLOTS, nco)
    assert r["family"] == FAMILY_ROWS, (T, D, own, nco)
    unit = lambda tail, n: ("fft", r["rows"], True, i16, n, tail, False, False)     # noqa: E731
    if r["tail"] != 8:
        return {unit(r["tail"], r["nco"])}
    if own or r["sub"] != 1:            # `general`: the per-channel form at any centre bin is the NCO = true instantiation
        return {unit(8, True)}
    even, odd, rest = bank8_plan(slots)
    units = set()
    if even or odd:                     # one all-slots launch per parity, or one over virtual blocks: the same instantiation
        units.add(unit(9, nco))
    if rest:                            # the left-over channels: slot form proper (no NCO) / general form under a context NCO
        units.add(unit(8, nco))
    return units


# ---------------------------------------------------------------- B: single channel, the case list

ROWS_TAPS = ((4, (1, 2, 3, 257)), (8, (258, 513)), (16, (514, 1025)), (32, (1026, 2049)), (48, (2050, 3073)))
TWO_PARTITION_TAPS = (3074, 4095, 4096)
ODD_EDGE_TAPS = (383, 384, 767, 768)     # (T + 3) // 3 <= 128: 2 dropped rows, <= 256: 4, else the selecting store
SINGLE_TAPS = tuple(t for _, ts in ROWS_TAPS for t in ts) + TWO_PARTITION_TAPS + ODD_EDGE_TAPS
# tail families by decimation: full rate | selecting store | decimate-by-4 | the same thinned | decimate-by-2 | thinned | odd kernel | thinned
TAILS = (("full", (1,)), ("select", (5, 7)), ("dec4", (4,)), ("dec4-sub", (12, 64)), ("dec2", (2,)), ("dec2-sub", (6, 62)), ("odd", (3,)),
         ("odd-sub", (9, 63)))
DECIMATIONS = tuple(d for _, ds in TAILS for d in ds)
FFT_FORMS = {"full": (False, 0, False), "select": (False, 0, True), "dec4": (True, 0, False), "dec4-sub": (True, 1, False),
             "dec2": (True, 2, False), "dec2-sub": (True, 3, False)}                 # (DEC4, CHAN, DECN)
WANTED_SINGLE = ({("fft", rows, dec4, a, b, tail, decn, False) for rows, _ in ROWS_TAPS for dec4, tail, decn in FFT_FORMS.values() for a in _B for b in _B}
                 | {("fft", 32, dec4, a, b, tail, decn, True) for dec4, tail, decn in FFT_FORMS.values() for a in _B for b in _B}
                 | {("odd", 3, ovlr, a, b, sub) for ovlr in (2, 4) for a in _B for b in _B for sub in _B})


def tail_family(T, D):
    """the family of TAILS the (taps, decimation) pair runs in (an odd decimation the odd kernel does not serve: the selecting store)"""
    r = fft_route(T, D)
    if r["family"] == FAMILY_ODD:
        return "odd-sub" if r["sub"] > 1 else "odd"
    return next(k for k, v in FFT_FORMS.items() if v == (r["dec4"], r["tail"], r["decn"]))


def single_cases():
    """(T, D, complex taps, int16, NCO): every boundary tap count x every decimation of TAILS, the flags cycling; then one case more,
    on the longest filter of its class, for every instantiation the product leaves out (a tail with one decimation meets a
    two-length class twice, and has four (int16, NCO) forms)."""
    out = []
    for ti, T in enumerate(SINGLE_TAPS):
        for di, D in enumerate(DECIMATIONS):
            k = 2 * (ti % 2) + di % 2 + ti // 2 + di // 4
            out.append((T, D, bool((ti + di + di // 3) & 1), bool(k & 1), bool(k & 2)))
    reached = set().union(*(single_units(T, D, i16, nco) for T, D, ct, i16, nco in out))
    longest = {4: 257, 8: 513, 16: 1025, 32: 2049, 48: 3073}
    first_d = {FFT_FORMS[name]: ds[0] for name, ds in TAILS if name in FFT_FORMS}
    for j, unit in enumerate(sorted(WANTED_SINGLE - reached)):
        if unit[0] == "odd":
            _, F, ovlr, i16, nco, sub = unit
            T, D = (383 if ovlr == 2 else 767), (9 if sub else 3)
        else:
            _, rows, dec4, i16, nco, tail, decn, acc = unit
            T, D = (4096 if acc else longest[rows]), first_d[(dec4, tail, decn)]
        if not single_units(T, D, i16, nco) <= reached:
            out.append((T, D, bool(j & 1), i16, nco))
            reached |= single_units(T, D, i16, nco)
    return out


def _single_coverage():
    cs = single_cases()
    units = set().union(*(single_units(T, D, i16, nco) for T, D, ct, i16, nco in cs))
    ct_rows = {(fft_route(T, D)["family"], fft_route(T, D)["rows"], nco) for T, D, ct, i16, nco in cs if ct}
    meets = {(T, tail_family(T, D)) for T, D, *_ in cs}
    return cs, units, ct_rows, meets


_cs, _units, _ct_rows, _meets = _single_coverage()
assert _units == WANTED_SINGLE                                                           # every (rows, tail, int16, NCO), accumulating partition, odd kernel
assert len(WANTED_SINGLE) == 5 * 24 + 24 + 16
assert {(FAMILY_ROWS, rows, b) for rows, _ in ROWS_TAPS for b in _B} <= _ct_rows          # complex taps: each rows class, NCO on and off,
assert {(FAMILY_TWO, 32, b) for b in _B} <= _ct_rows                                      # the two-partition form
assert {(FAMILY_ODD, ovlr, b) for ovlr in (2, 4) for b in _B} <= _ct_rows                 # and the odd kernel
# every boundary length meets every tail it can take: all eight up to 767 taps, the six of fir_fft_kernel beyond
assert _meets == ({(T, name) for T in SINGLE_TAPS for name in FFT_FORMS} | {(T, name) for T in SINGLE_TAPS if T <= 767 for name in ("odd", "odd-sub")})
assert all(tail_family(T, 3) == "select" for T in (768, 1025, 3073, 3074, 4096))          # 3 with >= 769 taps (768: (T + 3) // 3 = 257)
assert {fft_route(T, 3)["rows"] for T in (383, 384, 767)} == {2, 4} and fft_route(383, 3)["rows"] == 2 and fft_route(384, 3)["rows"] == 4
assert 200 <= len(_cs) <= 300, len(_cs)


# ---------------------------------------------------------------- D (cases): the filter bank

BANK_TAPS = (1, 2, 257, 258, 513, 514, 1025, 1026, 2049, 2050, 3073)
CENTRES = tuple(v / 4096.0 for v in (-2047, 777, -1, 1365, 5))      # on the 1/4096 grid: the float64 NCO oracle is exact for them
# (name, decimation, own centres, slots or number of centres, context NCO), named after how the form is reached
BANK_FORMS = (
    ("slots-4", 4, False, (3, 0, 9, 3), False),                     # slot grid at decimation 4 (a slot may repeat)
    ("own-4", 4, True, 3, False),
    ("own-12", 12, True, 5, False),
    ("slots-8-repeat", 8, False, (5, 2, 5), False),                 # a repeated slot: per-channel form, no NCO
    ("slots-8-even5", 8, False, (0, 4, 8, 2, 14), False),           # one all-slots launch
    ("slots-8-both", 8, False, (0, 2, 4, 6, 1, 3, 5, 15, 8), False),   # >= 4 even and >= 4 odd: one launch over virtual blocks
    ("slots-8-even4-odd2", 8, False, (0, 4, 3, 8, 12, 7), False),   # one all-slots launch and two left-over channels per channel
    ("slots-8-both-nco", 8, False, (0, 2, 4, 6, 1, 3, 5, 15, 8), True),   # the all-slots NCO form
    ("slots-8-even4-odd2-nco", 8, False, (0, 4, 3, 8, 12, 7), True),      # ... and its left-overs through the general form
    ("own-8", 8, True, 3, False),
    ("own-24", 24, True, 5, False),
    ("slots-16", 16, False, (15, 0, 7, 8, 1), False),
    ("slots-16-nco", 16, False, (15, 0, 7, 8, 1), True),
    ("own-16", 16, True, 5, False),
    ("own-48", 48, True, 3, False),
)
BANK_TAILS = ((4, False), (5, False), (6, False), (8, False), (8, True), (9, False), (9, True), (16, False), (16, True), (17, False))
WANTED_BANK = {("fft", rows, True, a, nco, tail, False, False) for rows, _ in ROWS_TAPS for tail, nco in BANK_TAILS for a in _B}


def bank_cases():
    """(T, form index, complex prototype, int16): every tap count x every form; int16 alternates within a rows class"""
    return [(T, fi, bool(((ti >> 1) + fi) & 1), bool((ti + fi) & 1)) for ti, T in enumerate(BANK_TAPS) for fi in range(len(BANK_FORMS))]


def bank_case_units(T, fi, i16):
    _, D, own, chans, nco = BANK_FORMS[fi]
    return bank_units(T, D, own, () if own else chans, nco, i16)


_bank_units = set().union(*(bank_case_units(T, fi, i16) for T, fi, ct, i16 in bank_cases()))
assert _bank_units == WANTED_BANK and len(WANTED_BANK) == 5 * 20                         # the 20 bank instantiations of every rows class
assert {ct for T, fi, ct, i16 in bank_cases()} == {False, True}
# how the decimation-8 forms on the slot grid split (test_filter_bank_decimation_8_routing pins the plan itself)
assert bank8_plan(BANK_FORMS[3][3]) == (0, 0, 0b111)
assert bank8_plan(BANK_FORMS[4][3]) == (0x4115, 0, 0)
assert bank8_plan(BANK_FORMS[5][3]) == (0x0155, 0x802A, 0)
assert bank8_plan(BANK_FORMS[6][3]) == (0x1111, 0, 0b100100)


# ---------------------------------------------------------------- A (tests): the restatement against the header and the build

def _bank_slot_lists():
    rng = np.random.default_rng(3)
    lists = [f[3] for f in BANK_FORMS if not f[2]] + [(7,), tuple(range(16)), (0, 2, 4), (0, 2, 4, 14, 1, 3, 5), (3, 1, 15, 13, 11, 9, 7, 5, 0, 4)]
    for _ in range(40):
        k = int(rng.integers(1, 17))
        lists.append(tuple(int(v) for v in (rng.permutation(16)[:k] if rng.random() < 0.6 else rng.integers(0, 16, size=k))))
    return lists


def test_the_python_route_is_the_headers():
    """tests/c/fft_route_dump.cpp compiles qo-100-tools_amd/csrc/if_fir_fft_route.h alone with a plain g++ and prints the route of every
    boundary tap count x decimation 1..64 x no bank / slots / own centres x NCO off / on, the odd tail, the overlap rows, the block
    advance and the bank's tail, and the decimation-8 plan of a set of slot lists: the Python statement above agrees on every line."""
    exe = os.path.join(tempfile.mkdtemp(prefix="fft_route_dump_"), "fft_route_dump")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "qo-100-tools_amd", "csrc"),
                           os.path.join(ROOT, "tests", "c", "fft_route_dump.cpp"), "-o", exe])
    lists = _bank_slot_lists()
    run = subprocess.run([exe] + [",".join(str(s) for s in sl) for sl in lists], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr
    got = run.stdout.splitlines()
    want = [route_line(T, D, bank, nco) for T in sorted(SINGLE_TAPS) for D in range(1, 65) for bank in (NO_BANK, BANK_SLOTS, BANK_OWN)
            for nco in (0, 1)]
    want += ["P %s: even %d odd %d rest %d" % ((",".join(str(s) for s in sl),) + bank8_plan(sl)) for sl in lists]
    assert len(got) == len(want) == len(SINGLE_TAPS) * 64 * 3 * 2 + len(lists)
    for g, w in zip(got, want):
        assert g == w
    assert set(BANK_TAPS) <= set(SINGLE_TAPS)


def compiled_units():
    """the template arguments in the mangled kernel names of the build's resource remarks (csrc/if_fir_fft.resources.txt)"""
    path = os.path.join(ROOT, "qo-100-tools_amd", "csrc", "if_fir_fft.resources.txt")
    assert os.path.exists(path), "build() first: the Makefile writes this file next to if_fir_fft.o"
    units, names = set(), 0
    for line in open(path):
        if not line.startswith("Function Name:"):
            continue
        m = re.search(r"fir_fft_kernelILi(\d+)ELb([01])ELb([01])ELb([01])ELi(\d+)ELb([01])ELb([01])EE", line)
        o = re.search(r"fir_odd_kernelILi(\d+)ELi(\d+)ELb([01])ELb([01])ELb([01])EE", line)
        assert bool(m) != bool(o), line
        names += 1
        if m:
            g = m.groups()
            units.add(("fft", int(g[0]), g[1] == "1", g[2] == "1", g[3] == "1", int(g[4]), g[5] == "1", g[6] == "1"))
        else:
            g = o.groups()
            units.add(("odd", int(g[0]), int(g[1]), g[2] == "1", g[3] == "1", g[4] == "1"))
    assert names == len(units)
    return units


def test_the_case_lists_reach_exactly_the_compiled_instantiations():
    """nothing compiled and untested, no case naming a kernel that does not exist: 244 fir_fft_kernel + 16 fir_odd_kernel"""
    built = compiled_units()
    assert sum(1 for u in built if u[0] == "fft") == 244 and sum(1 for u in built if u[0] == "odd") == 16
    reached = _units | _bank_units
    assert reached - built == set(), sorted(reached - built)
    assert built - reached == set(), sorted(built - reached)


def test_dropping_an_end_tap_is_loud(oracle):
    """The property the matrix rests on: with edge_taps, the float64 oracle without h[0], and without h[T-1], differs from the full
    filter by more than 1e-2 in both SPEC metrics at every boundary length, real and complex taps, on the matrix's stream: 1e4 over
    the tolerance (measured in numpy over every length from 2 to 4096: at least 0.109, at 4095 taps).  With a Blackman design in the
    place of edge_taps the difference is below 1e-6 from 255 taps on, and this test fails."""
    raw, x = signal(oracle, 6 * 3840 + 37, False)
    for T in sorted(SINGLE_TAPS):
        for ct in _B:
            taps = edge_taps(T, 1, ct)
            run = (lambda h: oracle.fir_ctaps_f64(h, x, 1)) if ct else (lambda h: oracle.fir_f64(h, x, 1))
            full = run(taps)
            for end in (0, T - 1):
                h = taps.copy().reshape(T, -1)
                h[end] = 0.0
                l2, mx = oracle.err_metrics(run(h.reshape(-1)), full)
                assert l2 > 1e-2 and mx > 1e-2, (T, ct, end, l2, mx)


# ---------------------------------------------------------------- B (tests): every single-channel instantiation, every boundary

def reference(oracle, taps, x, D, ct, freq):
    if freq:
        return oracle.fir_nco_f64(taps, x, D, oracle.nco_phase_word(freq), complex_taps=ct)
    return oracle.fir_ctaps_f64(taps, x, D) if ct else oracle.fir_f64(taps, x, D)


def make(fir, taps, D, ct, n, i16=False, freq=0.0, backend=None):
    """a development-library context; AUTO is the overlap-save backend for every filter the library accepts"""
    f = fir.IfFir(taps, D, max_samples=n, complex_taps=ct, dev=True)
    try:
        assert f.get_backend() == fir.BACKEND_HIP_FFT
        if backend is not None:
            f.set_backend(backend)
            assert f.get_backend() == backend
        if i16:
            f.set_input_format(fir.INPUT_I16)
        if freq:
            f.set_nco(freq)
    except Exception:
        f.close()
        raise
    return f


def run_pieces(f, raw, sizes):
    """process raw (interleaved) in pieces of the given sample counts, then the rest"""
    parts, pos = [], 0
    for s in sizes:
        parts.append(f.process(raw[2 * pos:2 * (pos + s)]))
        pos += s
    if 2 * pos < raw.size:
        parts.append(f.process(raw[2 * pos:]))
    return np.concatenate(parts)


def ragged_cut(n, a, D):
    """a cut near n / 3 that is a multiple neither of the block advance nor of the decimation: the second piece starts inside a
    block, on the history, and off the decimation phase"""
    cut = n // 3
    while cut % a == 0 or (D > 1 and cut % D == 0):
        cut += 1
    return cut


@pytest.mark.gpu
@pytest.mark.parametrize("T,D,ct,i16,nco", single_cases())
def test_matrix_against_float64(gpu_ok, fir, oracle, T, D, ct, i16, nco):
    a = fft_block_advance(T, D)
    n = 6 * a + 37
    raw, x = signal(oracle, n, i16)
    taps = edge_taps(T, 1, ct)
    freq = NCO_FREQS[(T + D) % len(NCO_FREQS)] if nco else 0.0
    with make(fir, taps, D, ct, n, i16, freq) as f:
        assert f.get_backend() == fir.BACKEND_HIP_FFT
        y = run_pieces(f, raw, [ragged_cut(n, a, D)])
        assert f.debug_queue_faults() == 0
    assert y.size == 2 * oracle.out_count(0, n, D)
    check(oracle, y, reference(oracle, taps, x, D, ct, freq), (tail_family(T, D), "rows", fft_route(T, D)["rows"], T, D, ct, i16, nco), TAG)


# ---------------------------------------------------------------- C: call sizes, streaming state, the block queue

# the longest filter of each class with one decimating tail beside D = 1: (T, D, complex taps, int16, NCO)
ROUND_A_BLOCK = [(257, 4, False, False, 0.0), (513, 12, True, True, 0.0), (1025, 2, False, True, 0.37), (2049, 6, True, False, -0.21),
                 (3073, 64, False, True, 1 / 4096), (4096, 4, True, False, -0.4999), (383, 3, False, True, 0.0), (767, 9, True, False, 0.123456)]


@pytest.mark.gpu
@pytest.mark.parametrize("T,D,ct,i16,freq", [(T, d, ct, i16, freq) for T, D, ct, i16, freq in ROUND_A_BLOCK for d in (1, D)])
def test_single_calls_round_a_block(gpu_ok, fir, oracle, T, D, ct, i16, freq):
    """one call of n samples after a reset, n round the samples a block advances by"""
    a = fft_block_advance(T, D)
    raw, x = signal(oracle, 2 * a + 1, i16)
    taps = edge_taps(T, 1, ct)
    with make(fir, taps, D, ct, 2 * a + 1, i16, freq) as f:
        for n in (1, 2, a - 1, a, a + 1, 2 * a, 2 * a + 1):
            f.reset()
            y = f.process(raw[:2 * n])
            assert y.size == 2 * oracle.out_count(0, n, D)
            check(oracle, y, reference(oracle, taps, x[:2 * n], D, ct, freq), ("single", T, D, n), TAG)
        assert f.debug_queue_faults() == 0


@pytest.mark.gpu
@pytest.mark.parametrize("i16", [False, True])
@pytest.mark.parametrize("T,D,hist", [(3073, 1, 3072), (4096, 4, 4096), (767, 3, 768)])
def test_pieces_shorter_than_the_history(gpu_ok, fir, oracle, T, D, hist, i16):
    """a stream of about three histories (3073 taps: the 3072-sample overlap; 4096 taps: 2048 samples of delay and the overlap; 767
    taps at decimation 3: 3 x 256) in pieces of 1, 7, 64 and 1000 samples: a piece shorter than the history shifts the old
    history instead of replacing it, and the decimation phase moves with every piece"""
    assert fft_route(T, D)["hist"] == hist
    n = 3 * hist + 11
    sizes, k = [], 0
    while sum(sizes) + (1, 7, 64, 1000)[k % 4] <= n:
        sizes.append((1, 7, 64, 1000)[k % 4])
        k += 1
    raw, x = signal(oracle, n, i16)
    ct = T == 4096
    freq = 0.37 if (T == 3073) == i16 else 0.0          # the NCO on for half of the six
    taps = edge_taps(T, 1, ct)
    with make(fir, taps, D, ct, n, i16, freq) as f:
        y = run_pieces(f, raw, sizes)
        assert f.debug_queue_faults() == 0
    check(oracle, y, reference(oracle, taps, x, D, ct, freq), ("short pieces", T, D, i16, bool(freq)), TAG)


# one case per tail family (and the two-partition form): (T, D, complex taps, int16, NCO)
SMALL_GRID = [(513, 1, False, False, 0.0), (513, 5, True, True, 0.0), (1025, 4, False, True, 0.37), (257, 12, True, False, 0.0),
              (2049, 2, False, False, -0.21), (3073, 6, False, True, 0.0), (383, 3, True, False, 0.0), (767, 9, False, True, 0.123456),
              (4096, 1, False, False, 0.0), (3074, 2, True, True, 1 / 4096)]
assert {tail_family(T, D) for T, D, *_ in SMALL_GRID} == {name for name, _ in TAILS}


@pytest.mark.gpu
@pytest.mark.parametrize("T,D,ct,i16,freq", SMALL_GRID)
def test_block_queue_on_a_small_grid(gpu_ok, fir, oracle, T, D, ct, i16, freq):
    """tuning 2001 and 2003: at most one and three workgroups, so the 40 blocks of the call go through the block queue (a normal
    launch gives every wave of the chip one block and is done).  Which wave computes a block must not matter: bit-identical to
    the default launch of the same call."""
    a = fft_block_advance(T, D)
    n = 40 * a + 37
    raw, x = signal(oracle, n, i16)
    taps = edge_taps(T, 1, ct)
    with make(fir, taps, D, ct, n, i16, freq) as f:
        y0 = f.process(raw)
        for tuning in (2001, 2003):
            f.reset()
            f.set_tuning(tuning)
            y = f.process(raw)
            assert np.array_equal(y, y0), (tuning, int(np.argmax(y != y0)))
        assert f.debug_queue_faults() == 0
    check(oracle, y0, reference(oracle, taps, x, D, ct, freq), ("small grid", T, D), TAG)


# ---------------------------------------------------------------- C': the other backends on the same taps

@pytest.mark.gpu
@pytest.mark.parametrize("T,D", [(127, 1), (127, 4), (255, 1), (255, 4)])
def test_direct_form_on_edge_taps(gpu_ok, fir, oracle, T, D):
    """the unrolled direct form, schedule variants 0..6: float64 oracle, and bit-exact against the float32 order model (a first or
    last tap of 2e-19 of the peak, as a windowed design has, cannot change a float32 sum: here it is the largest)"""
    n = 20_011
    raw, x = signal(oracle, n, False)
    taps = edge_taps(T, 1, False)
    model = oracle.fir_f32fma(taps, x, D, **SEG)
    ref = oracle.fir_f64(taps, x, D)
    with make(fir, taps, D, False, n, backend=fir.BACKEND_HIP_DIRECT) as f:
        for variant in range(7):
            f.reset()
            f.set_tuning(variant)
            y = run_pieces(f, raw, [ragged_cut(n, 256, D)])
            assert np.array_equal(y, model), (variant, np.max(np.abs(y - model)))
            check(oracle, y, ref, ("direct", T, D, variant), TAG)


@pytest.mark.gpu
@pytest.mark.parametrize("T", [1, 2, 257, 4096])
@pytest.mark.parametrize("D", [1, 3, 64])
def test_generic_kernel_on_edge_taps(gpu_ok, fir, oracle, T, D):
    """the generic kernel: float32 and int16 input, real and complex taps, NCO off and on, in two ragged pieces; real taps
    without the NCO bit-exact against the order model as well"""
    n = 20_011
    for k, (ct, i16, freq) in enumerate([(False, False, 0.0), (False, True, 0.0), (True, False, 0.0), (False, False, NCO_FREQS[(T + D) % 5]),
                                         (True, True, NCO_FREQS[(T + D + 2) % 5])]):
        raw, x = signal(oracle, n, i16)
        taps = edge_taps(T, 1, ct)
        with make(fir, taps, D, ct, n, i16, freq, backend=fir.BACKEND_HIP_GENERIC) as f:
            y = run_pieces(f, raw, [ragged_cut(n, 256, D)])
        if not ct and not freq:
            model = oracle.fir_f32fma(taps, x, D, **SEG)
            assert np.array_equal(y, model), (k, np.max(np.abs(y - model)))
        check(oracle, y, reference(oracle, taps, x, D, ct, freq), ("generic", T, D, ct, i16, bool(freq)), TAG)


@pytest.mark.gpu
@pytest.mark.parametrize("T,D", [(2, 1), (5, 3), (255, 4), (1023, 1), (4096, 64), (4096, 1)])
def test_tapsplit_kernel_on_edge_taps(gpu_ok, fir, oracle, T, D):
    """the tap-split kernel: float64 oracle, and bit-exact against its order model (segments of 32 taps over 4 lanes: mode 3)"""
    n = 20_011
    raw, x = signal(oracle, n, False)
    taps = edge_taps(T, 1, False)
    model = oracle.fir_f32fma(taps, x, D, **SEG_TAPSPLIT)
    with make(fir, taps, D, False, n, backend=fir.BACKEND_HIP_TAPSPLIT) as f:
        y = run_pieces(f, raw, [ragged_cut(n, 256, D)])
    assert np.array_equal(y, model), np.max(np.abs(y - model))
    check(oracle, y, oracle.fir_f64(taps, x, D), ("tapsplit", T, D), TAG)


# ---------------------------------------------------------------- D (tests): every filter-bank instantiation

@pytest.mark.gpu
@pytest.mark.parametrize("T,fi,ct,i16", bank_cases(), ids=["%d-%s-%s-%s" % (T, BANK_FORMS[fi][0], "ctaps" if ct else "real", "i16" if i16 else "f32")
                                                              for T, fi, ct, i16 in bank_cases()])
def test_bank_matrix_against_float64(gpu_ok, fir, oracle, torch_cuda, T, fi, ct, i16):
    """every channel of a filter-bank call in two ragged pieces against the float64 NCO oracle (slot s: phase word (s << 28) + the
    context's; own centres: the centre's); a guard band behind every output buffer stays intact.  The cut falls anywhere, for
    int16 input too: include/if_fir.h asks for nothing of a call's length, and the input pointer of a piece is aligned here."""
    torch = torch_cuda
    name, D, own, chans, with_nco = BANK_FORMS[fi]
    a = fft_block_advance(T, D)
    n = 6 * a + 37
    raw, x = signal(oracle, n, i16)
    taps = edge_taps(T, 1, ct)
    freq = NCO_FREQS[(T + fi) % len(NCO_FREQS)] if with_nco else 0.0
    centres = CENTRES[:chans] if own else None
    nch = chans if own else len(chans)
    cut = ragged_cut(n, a, D)
    xd = torch.from_numpy(raw).cuda()
    parts = [[] for _ in range(nch)]
    with make(fir, taps, D, ct, n, i16, freq) as f:
        word = oracle.nco_phase_word(f.get_nco()) if freq else 0
        for lo, hi in ((0, cut), (cut, n)):
            m_exp = oracle.out_count(lo, hi - lo, D)
            outs = [torch.full((2 * m_exp + 8,), 3.0, dtype=torch.float32, device="cuda") for _ in range(nch)]
            piece = xd[2 * lo:2 * hi].clone()
            torch.cuda.synchronize()
            ptrs = [o.data_ptr() for o in outs]
            if own:
                assert f.channelizer_process_device_freq(centres, piece.data_ptr(), ptrs, hi - lo) == m_exp
            else:
                assert f.channelizer_process_device(chans, piece.data_ptr(), ptrs, hi - lo) == m_exp
            f.synchronize()
            for c in range(nch):
                o = outs[c].cpu().numpy()
                assert np.all(o[2 * m_exp:] == 3.0), (name, T, c)
                parts[c].append(o[:2 * m_exp])
        assert f.debug_queue_faults() == 0
    errs = []
    for c in range(nch):
        pw = oracle.nco_phase_word(centres[c]) if own else ((chans[c] << 28) + word) & 0xFFFFFFFF
        ref = oracle.fir_nco_f64(taps, x, D, pw, complex_taps=ct)
        got = np.concatenate(parts[c])
        assert got.shape == ref.shape
        errs.append(oracle.err_metrics(got, ref))
    l2, mx = max(e[0] for e in errs), max(e[1] for e in errs)       # the worst channel
    print(TAG, ("bank", name, "rows", fft_overlap_rows(T), T, D, ct, i16), "l2=%.3g max=%.3g" % (l2, mx))
    assert l2 <= TOL and mx <= TOL, (name, T, errs)
