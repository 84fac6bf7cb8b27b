// if_fir_arb_plan.h — host-side planning of the arbitrary-ratio resampler (docs/SPEC.md §12): validation, what
// one call emits from its stream position, the shape of a tile, a tile's base time and the tap table.  No HIP types: the shim,
// the kernel unit and tests/c/arb_plan_check.cpp (plain g++) all include this file, so what the checker walks is what the
// launcher and the kernel use.
//
//   P = 2^b,  K = ceil(T / P),  R = input samples per output sample x 2^32,  tau = time of the next output in 2^-32 input samples
//   q = floor(tau / 2^32),  f = tau mod 2^32,  p = f >> (32 - b),  mu = (f mod 2^(32 - b)) / 2^(32 - b)
//   y = sum_{j = 0}^{K - 1} [(1 - mu) h[p + j P] + mu h[p + 1 + j P]] x[q - j],      then tau += R
//
// The shim holds c (64 bits) and tau (96 bits, in an unsigned __int128).  The kernel sees neither: it gets tau_rel = tau - c 2^32
// (< 2^34) and R, and output i of the call sits at tau_rel + i R counted from the call's first input.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <cmath>

#include "if_fir_stream_plan.h"

namespace if_fir
{

typedef unsigned __int128 arb_u128;

constexpr int ARB_MIN_BITS = 4;
constexpr int ARB_MAX_BITS = 10;
constexpr int ARB_MAX_TAPS = 8192;
constexpr uint64_t ARB_MIN_STEP = (uint64_t)1 << 26; // 1/64 input samples per output
constexpr uint64_t ARB_MAX_STEP = (uint64_t)1 << 34; // 4
constexpr uint64_t ARB_MAX_SAMPLES = (uint64_t)1 << 36; // inputs of one call: 64 times as many outputs stay below 2^43
constexpr int ARB_THREADS = 256;                     // one workgroup
constexpr int ARB_R = 4;                             // outputs per lane: t, t + 256, t + 512, t + 768 of the tile
constexpr int ARB_TILE_OUT = ARB_THREADS * ARB_R;    // consecutive outputs of one tile

inline bool arb_valid(uint32_t T, uint32_t b, uint64_t R)
{
    return T >= 1 && T <= (uint32_t)ARB_MAX_TAPS && b >= (uint32_t)ARB_MIN_BITS && b <= (uint32_t)ARB_MAX_BITS && R >= ARB_MIN_STEP &&
           R <= ARB_MAX_STEP;
}

// taps per phase
inline int arb_phase_taps(int T, int b)
{
    return (T + (1 << b) - 1) >> b;
}

// row stride of the tap table in entries of 8 bytes: odd, so that the rows of 32 consecutive phases start on 32 different
// pairs of LDS banks (a ds_read_b64 serves 32 lanes per cycle over 64 banks)
inline int arb_row_stride(int K)
{
    return K | 1;
}

struct ArbShape
{
    int K;           // phase taps
    int KP;          // row stride of the tap table, entries
    int P;           // phases
    int tile_out;    // consecutive outputs of one tile
    int x_len;       // samples of a tile's window in LDS at this step
    int tap_entries; // P KP entries of (h[p + j P], h[p + 1 + j P])
};

// the window of a tile: its first output has q = q0 and a fraction f0 < 2^32, its last one q0 + ((tile_out - 1) R + f0) >> 32,
// and the taps reach K - 1 samples before q0
inline int arb_window(int K, uint64_t R)
{
    return (int)((((uint64_t)(ARB_TILE_OUT - 1) * R + 0xffffffffull) >> 32) + (uint64_t)K); // <= 4092 + 512
}

inline ArbShape arb_shape(int T, int b, uint64_t R)
{
    ArbShape s;
    s.P = 1 << b;
    s.K = arb_phase_taps(T, b);
    s.KP = arb_row_stride(s.K);
    s.tile_out = ARB_TILE_OUT;
    s.x_len = arb_window(s.K, R);
    s.tap_entries = s.P * s.KP;
    return s;
}

inline size_t arb_lds_bytes(const ArbShape &s)
{
    return ((size_t)s.tap_entries + (size_t)s.x_len) * 8;
}
// the largest arb_lds_bytes: 1024 rows of 9 entries (b = 10, T = 8192) is the largest table, 4092 + 512 samples the largest
// window; both bounds at once overestimate any real shape
constexpr int ARB_LDS_MAX = 8 * (1024 * 9 + 4092 + 512);

// outputs of a call that brings the inputs [c, c + n) with the next output at tau: every output with floor(tau / 2^32) < c + n,
// max(0, ceil(((c + n) 2^32 - tau) / R)).  false when c + n leaves 64 bits.
inline bool arb_out_count(uint64_t c, arb_u128 tau, uint64_t n, uint64_t R, uint64_t *count)
{
    if (c + n < c)
        return false;
    const arb_u128 end = (arb_u128)(c + n) << 32;
    *count = end > tau ? (uint64_t)((end - tau + (R - 1)) / R) : 0;
    return true;
}

// the state's invariant: c 2^32 <= tau < c 2^32 + 2^34
inline bool arb_state_ok(uint64_t c, arb_u128 tau)
{
    const arb_u128 lo = (arb_u128)c << 32;
    return tau >= lo && tau - lo < ((arb_u128)1 << 34);
}

// the time of output i of a call, counted from the call's first input: tau_rel + i R as a 64-bit integer part and a 32-bit
// fraction.  One 64 x 64 -> 128 multiply; i < 2^43 and R <= 2^34 keep the product below 2^77, so its high word fits 32 bits.
IF_FIR_STREAM_HD inline void arb_time(uint64_t tau_rel, uint64_t i, uint64_t R, int64_t *q, uint32_t *f)
{
#if defined(__HIP_DEVICE_COMPILE__)
    uint64_t hi = __umul64hi(i, R);
    const uint64_t prod = i * R;
#else
    const arb_u128 wide = (arb_u128)i * R;
    uint64_t hi = (uint64_t)(wide >> 64);
    const uint64_t prod = (uint64_t)wide;
#endif
    const uint64_t lo = prod + tau_rel;
    hi += lo < prod; // the carry of the 64-bit add
    *q = (int64_t)((hi << 32) | (lo >> 32));
    *f = (uint32_t)lo;
}

// output l of a tile whose base time has the fraction f0: its input index relative to the tile's q0, its phase and the
// fraction behind the phase, scaled to [0, 1) and rounded ONCE to float32
IF_FIR_STREAM_HD inline void arb_place(uint32_t f0, int l, uint64_t R, int b, int *dq, int *p, float *mu)
{
    const uint64_t t = (uint64_t)f0 + (uint64_t)l * R; // < 2^32 + 1023 2^34
    const uint32_t f = (uint32_t)t;
    *dq = (int)(t >> 32);
    *p = (int)(f >> (32 - b));
    const uint32_t low = f & ((1u << (32 - b)) - 1u);
    *mu = (float)low * (1.0f / (float)(1u << (32 - b))); // the product by a power of two is exact: one rounding, in (float)low
}

// the table: entry (p, j), p = 0 .. P - 1, j = 0 .. K - 1, at [(p KP + j) 2] holds the pair (h[p + j P], h[p + 1 + j P]), zero
// where the index reaches T: the rows p and p + 1 of the phase-major form side by side, so that one 8-byte read gives both
// and p + 1 never wraps (row P - 1 carries h[P + j P] as its second element).  out holds 2 P KP floats.  Nothing is rounded.
inline void arb_build_taps(const float *taps, int T, int b, float *out)
{
    const int P = 1 << b, K = arb_phase_taps(T, b), KP = arb_row_stride(K);
    for (int i = 0; i < 2 * P * KP; i++)
        out[i] = 0.0f;
    for (int p = 0; p < P; p++)
        for (int j = 0; j < K; j++)
            for (int e = 0; e < 2; e++)
            {
                const int k = p + e + j * P;
                if (k < T)
                    out[(p * KP + j) * 2 + e] = taps[k];
            }
}

// rint(in / out 2^32), 0 when that is outside [ARB_MIN_STEP, ARB_MAX_STEP] or the rates are not positive finite numbers
inline uint64_t arb_step_from_rates(double rate_in, double rate_out)
{
    if (!(rate_in > 0.0) || !(rate_out > 0.0) || !std::isfinite(rate_in) || !std::isfinite(rate_out))
        return 0;
    const double r = std::rint(rate_in / rate_out * 4294967296.0);
    if (!(r >= (double)ARB_MIN_STEP) || !(r <= (double)ARB_MAX_STEP))
        return 0;
    return (uint64_t)r;
}

} // namespace if_fir
