"""CPU tests: the oracle against the committed golden vectors (scipy-made) and analytic known-answer tests.
PARITY UNPINNED (no reference implementation exists: SURVEY.md §0/§8c)."""
import os

import numpy as np
import pytest

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "if_fir_golden.npz")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


@pytest.mark.parametrize("t", [127, 255, 1023])
def test_designer_matches_golden_taps(oracle, gold, t):
    h = oracle.bpf_design(t)
    assert np.array_equal(h, gold["taps_%d" % t])          # scipy.signal.firwin fixture, bit-exact in float32
    assert np.array_equal(h, oracle.bpf_design_numpy(t))   # independent numpy restatement
    assert np.array_equal(h, h[::-1])                      # type-I linear phase
    # unity gain at the band centre, >70 dB rejection at 0.40 cycles/sample (the synthetic stop-band tone)
    n = np.arange(t) - (t - 1) / 2
    assert abs(np.sum(h * np.exp(-2j * np.pi * 0.2 * n))) == pytest.approx(1.0, abs=1e-6)
    if t >= 255:
        assert abs(np.sum(h * np.exp(-2j * np.pi * 0.4 * n))) < 10 ** (-70 / 20)


def test_designer_rejects_bad_arguments(oracle):
    for bad in [dict(taps=128), dict(taps=1), dict(taps=127, f_low=0.3, f_high=0.2), dict(taps=127, f_high=0.6)]:
        with pytest.raises(ValueError):
            oracle.bpf_design(**bad)


def test_synth_matches_golden_and_numpy(oracle, gold):
    x = oracle.synth_iq(4096)
    assert np.array_equal(x, gold["x"])
    assert np.array_equal(oracle.synth_iq(1000, channel=3, first=777), oracle.synth_iq_numpy(1000, channel=3, first=777))
    # stream continuity: generating in two pieces is the same stream
    assert np.array_equal(np.concatenate([oracle.synth_iq(100), oracle.synth_iq(50, first=100)]), oracle.synth_iq(150))
    assert not np.array_equal(oracle.synth_iq(64, channel=0), oracle.synth_iq(64, channel=1))


@pytest.mark.parametrize("t", [127, 255, 1023])
@pytest.mark.parametrize("d", [1, 4])
def test_oracle_f64_matches_golden(oracle, gold, t, d):
    y = oracle.fir_f64(gold["taps_%d" % t], gold["x"], d)
    ref = gold["y_T%d_D%d" % (t, d)]
    assert y.shape == ref.shape
    assert np.max(np.abs(y - ref)) <= 4e-15  # both float64; summation order differs


def test_oracle_real_matches_golden(oracle, gold):
    y = oracle.fir_real_f64(gold["taps_127"], gold["xr"])
    assert np.max(np.abs(y - gold["yr_T127"])) <= 4e-15
    # the complex path with Q = 0 gives the same I and an all-zero Q (how the GPU path runs configs[0])
    xz = np.zeros(2 * gold["xr"].size, dtype=np.float32)
    xz[0::2] = gold["xr"]
    yc = oracle.fir_f64(gold["taps_127"], xz, 1)
    assert np.array_equal(yc[0::2], y) and not np.any(yc[1::2])


@pytest.mark.parametrize("t,d", [(127, 1), (255, 1), (255, 4), (127, 4), (31, 3), (1, 1), (2, 2)])
def test_kat_impulse_step_tone(oracle, t, d):
    rng = np.random.default_rng(t * 10 + d)
    h = (oracle.bpf_design(t) if t >= 3 and t % 2 else rng.standard_normal(t).astype(np.float32))
    n = 4 * t + 64
    # impulse -> taps
    x = np.zeros(2 * n, dtype=np.float32)
    x[0] = 1.0
    x[1] = -2.0
    y = oracle.fir_f64(h, x, 1)
    assert np.array_equal(y[0:2 * t:2], h.astype(np.float64)) and np.array_equal(y[1:2 * t:2], -2.0 * h.astype(np.float64))
    assert not np.any(y[2 * t:])
    # step -> cumulative tap sum
    x = np.ones(2 * n, dtype=np.float32)
    y = oracle.fir_f64(h, x, 1)
    cs = np.cumsum(h.astype(np.float64))
    assert np.allclose(y[0:2 * t:2], cs, rtol=0, atol=1e-15 * t)
    # decimation == filter then pick
    xr = rng.standard_normal(2 * n).astype(np.float32)
    full = oracle.fir_f64(h, xr, 1).reshape(-1, 2)
    dec = oracle.fir_f64(h, xr, d).reshape(-1, 2)
    assert np.array_equal(dec, full[::d])
    # complex tone: steady-state gain equals H(f) from the taps (float64)
    f = 0.2
    k = np.arange(n)
    tone = np.exp(2j * np.pi * f * k).astype(np.complex64)
    yt = oracle.fir_f64(h, tone, 1).view(np.complex128)
    hf = np.sum(h.astype(np.float64) * np.exp(-2j * np.pi * f * np.arange(t)))
    expect = hf * np.exp(2j * np.pi * f * k)
    # the tone fed in is rounded to float32 (2^-24 relative per component), the filter itself is exact to float64
    assert np.max(np.abs(yt[t:] - expect[t:])) <= 1.5 * 2.0 ** -24 * max(1.0, np.sum(np.abs(h)))
    conv = np.convolve(tone.astype(np.complex128), h.astype(np.float64))[:n]
    assert np.max(np.abs(yt - conv)) <= 1e-14 * max(1.0, np.sum(np.abs(h)))


def test_linearity_and_shift(oracle):
    rng = np.random.default_rng(5)
    h = oracle.bpf_design(127)
    a = rng.integers(-8, 8, 2 * 600).astype(np.float32)   # small integers: float64 sums are exact
    b = rng.integers(-8, 8, 2 * 600).astype(np.float32)
    hi = rng.integers(-4, 4, 127).astype(np.float32)
    ya, yb, yab = (oracle.fir_f64(hi, v, 1) for v in (a, b, a + 2 * b))
    assert np.array_equal(yab, ya + 2 * yb)
    sh = np.concatenate([np.zeros(2 * 7, dtype=np.float32), a])
    assert np.array_equal(oracle.fir_f64(h, sh, 1)[2 * 7:], oracle.fir_f64(h, a, 1))


@pytest.mark.parametrize("d", [1, 3, 4])
def test_streaming_equals_one_shot(oracle, d):
    h = oracle.bpf_design(255)
    x = oracle.synth_iq(3000)
    one = oracle.fir_f64(h, x, d)
    for cuts in [(1, 2, 250, 254, 255, 1001), (1500,), (0, 10, 10, 2999)]:
        st = oracle.OracleStream(h, d)
        parts, pos = [], 0
        for c in list(cuts) + [3000]:
            parts.append(st.process(x[2 * pos:2 * c]))
            pos = c
        assert np.array_equal(np.concatenate(parts), one)
        assert st.consumed == 3000


def test_out_count(oracle):
    for consumed in range(0, 9):
        for n in range(0, 12):
            for d in (1, 2, 4, 5):
                expect = len([i for i in range(consumed, consumed + n) if i % d == 0])
                assert oracle.out_count(consumed, n, d) == expect


@pytest.mark.parametrize("t,d", [(255, 1), (255, 4), (127, 1)])
def test_f32_models_within_tolerance(oracle, t, d):
    """The float32 order model (what the HIP kernels reproduce bit-for-bit) and the timed CPU baseline both meet
    SPEC §3 against the float64 oracle; a single 255-long chain does not meet the max bound (why segments exist)."""
    h = oracle.bpf_design(t)
    x = oracle.synth_iq(1 << 16)
    ref = oracle.fir_f64(h, x, d)
    l2, mx = oracle.err_metrics(oracle.fir_f32fma(h, x, d, seg_mode=1, seg_len=32), ref)
    assert l2 <= 2e-7 and mx <= 6e-7
    l2o, mxo = oracle.err_metrics(oracle.fir_f32_omp(h, x, d), ref)
    assert l2o <= 1e-6 and mxo <= 3e-6
    if t == 255 and d == 1:
        _, mx1 = oracle.err_metrics(oracle.fir_f32fma(h, x, d), ref)
        assert mx1 > mx


def test_tapsplit_order_model_matches_a_python_restatement(oracle):
    """Mode 3 of the float32 order model (tap-split kernel): lane q owns taps 4j+q, descending j, segments of 32 steps,
    quad sums combined as (q0+q1)+(q2+q3) — restated here with numpy float32 scalars on a small case."""
    rng = np.random.default_rng(3)
    t, d, n = 77, 3, 200
    h = rng.standard_normal(t).astype(np.float32)
    x = rng.integers(-64, 64, 2 * n).astype(np.float32) / np.float32(8)
    y = oracle.fir_f32fma(h, x, d, seg_mode=3, seg_len=32)
    xc = x.reshape(-1, 2)
    jn = (t + 3) // 4
    out = []
    for m in range(oracle.out_count(0, n, d)):
        nn = m * d
        lanes = []
        for q in range(4):
            tot, acc, have = np.zeros(2, np.float32), np.zeros(2, np.float32), False
            for j in range(jn - 1, -1, -1):
                k = 4 * j + q
                if k < t and nn - k >= 0:
                    # float32 fma: exact product in float64 (24+24 bits), one rounding of the sum to float32
                    acc = (xc[nn - k].astype(np.float64) * np.float64(h[k]) + acc.astype(np.float64)).astype(np.float32)
                if j % 32 == 0:
                    tot = acc.copy() if not have else (tot + acc).astype(np.float32)
                    have, acc = True, np.zeros(2, np.float32)
            lanes.append(tot)
        out.append(((lanes[0] + lanes[1]).astype(np.float32) + (lanes[2] + lanes[3]).astype(np.float32)).astype(np.float32))
    assert np.array_equal(y.reshape(-1, 2), np.array(out, dtype=np.float32))
    l2, mx = oracle.err_metrics(y, oracle.fir_f64(h, x, d))
    assert l2 <= 2e-7 and mx <= 6e-7


def test_complex_taps_oracle_matches_golden(oracle, gold):
    g = oracle.bpf_design_complex(255, 0.2, 0.1)
    assert np.array_equal(g, gold["ctaps_255"])                 # scipy-made fixture, bit-exact in float32
    for d in (1, 4):
        y = oracle.fir_ctaps_f64(g, gold["x"], d)
        assert np.max(np.abs(y - gold["yc_T255_D%d" % d])) <= 4e-15
        l2, mx = oracle.err_metrics(oracle.fir_ctaps_f32fma(g, gold["x"], d), y)
        assert l2 <= 2e-7 and mx <= 6e-7
    # real taps written as complex taps with zero imaginary part give the real-tap oracle exactly
    h = oracle.bpf_design(127)
    hc = np.zeros(254, dtype=np.float32)
    hc[0::2] = h
    assert np.array_equal(oracle.fir_ctaps_f64(hc, gold["x"], 3), oracle.fir_f64(h, gold["x"], 3))
    # the stop-band tone at +0.4 and the mirror image at -0.2 are rejected, the +0.2 tone passes with unit gain
    n = np.arange(4096)
    for f, expect in [(0.2, 1.0), (-0.2, 0.0), (0.4, 0.0)]:
        tone = np.exp(2j * np.pi * f * n).astype(np.complex64)
        y = oracle.fir_ctaps_f64(g, tone, 1).view(np.complex128)[300:]
        assert abs(np.mean(np.abs(y)) - expect) < 2e-4


def test_nco_oracle_matches_golden_and_identity(oracle, gold):
    """SPEC §3.2: the NCO oracle (mix by the definition, then filter) against the numpy/scipy-made fixture; the
    complex-taps identity the kernels use (g[k] = h[k] e^{+j theta k}, output rotated by e^{-j theta a}); phase
    continuity over a cut; frequency quantisation."""
    pw = int(gold["nco_phase_word"][0])
    assert pw == oracle.nco_phase_word(0.2) == 858993459
    assert oracle.nco_phase_word(-0.25) == 3 << 30 and oracle.nco_phase_word(0.0) == 0
    h = gold["taps_lp_255"]
    x = gold["x"]
    n = x.size // 2
    for d in (1, 4):
        y = oracle.fir_nco_f64(h, x, d, pw)
        assert np.max(np.abs(y - gold["ynco_T255_D%d" % d])) <= 4e-15
        # identity, in float64 throughout
        theta = 2.0 * np.pi * pw / 2.0 ** 32
        g = h.astype(np.float64) * np.exp(1j * theta * np.arange(h.size))
        full = np.convolve(x.astype(np.float64).view(np.complex128), g)[:n]
        a = np.arange(n, dtype=np.uint64)
        rot = np.exp(-2j * np.pi * (((a * np.uint64(pw)) & np.uint64(0xFFFFFFFF)).astype(np.float64) / 2.0 ** 32))
        assert np.max(np.abs((full * rot)[::d] - y.view(np.complex128))) <= 1e-13
        # a cut in the stream: history holds unmixed samples, the phase continues from the absolute index
        cut = 1501
        y1 = oracle.fir_nco_f64(h, x[:2 * cut], d, pw)
        hist = oracle.update_history(h.size, np.zeros(2 * (h.size - 1), np.float32), x[:2 * cut])
        y2 = oracle.fir_nco_f64(h, x[2 * cut:], d, pw, hist=hist, consumed=cut)
        assert np.array_equal(np.concatenate([y1, y2]), y)
    # phase word 0 = no NCO
    assert np.array_equal(oracle.fir_nco_f64(h, x, 4, 0), oracle.fir_f64(h, x, 4))


@pytest.mark.parametrize("d", [4, 12, 16, 64])
@pytest.mark.parametrize("centre", [300 / 4096.0, -0.5])
def test_bank_window_reference_equals_the_nco_oracle_past_2_32_samples(oracle, d, centre):
    """tests/bank_ref.py (the by-definition float64 form of a filter-bank channel on a window of a long stream, SPEC §3.3)
    against the C oracle: for a centre on the 1/4096 grid the two are the same numbers.  The window starts past 2^32
    samples, where the mix-down phase needs the 64-bit sample index; 2048 outputs, history from the stream."""
    import bank_ref
    t = 255
    taps = oracle.bpf_design(t, 0.0, 0.02)
    start = (1 << 32) + 1000 * d
    w = 2048 * d
    xs = oracle.synth_iq(t - 1 + w, 5, start - (t - 1))
    got = bank_ref.bank_window_ref(oracle, taps, xs, t, d, centre, start)
    ref = oracle.fir_nco_f64(taps, xs[2 * (t - 1):], d, oracle.nco_phase_word(centre), hist=xs[:2 * (t - 1)], consumed=start)
    assert got.shape == ref.shape == (2 * 2048,)
    assert np.max(np.abs(ref)) > 1e-3
    assert np.allclose(got, ref, rtol=0.0, atol=1e-12 * np.max(np.abs(ref)))
    # the stream's first samples: zeros in front of sample 0
    x0 = oracle.synth_iq(w, 5, 0)
    got0 = bank_ref.bank_window_ref(oracle, taps, np.concatenate([np.zeros(2 * (t - 1), np.float32), x0]), t, d, centre, 0)
    ref0 = oracle.fir_nco_f64(taps, x0, d, oracle.nco_phase_word(centre))
    assert np.allclose(got0, ref0, rtol=0.0, atol=1e-12 * np.max(np.abs(ref0)))
