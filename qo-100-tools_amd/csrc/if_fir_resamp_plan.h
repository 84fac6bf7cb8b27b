// if_fir_resamp_plan.h — host-side planning of the rational L/M resampler (docs/SPEC.md §7): the shape of a
// tile, the phase-major tap table, and what one call emits from its stream position.  No HIP types: the shim, the kernel unit
// and tests/c/resamp_plan_check.cpp (plain g++) all include this file, so what the checker walks is what the launcher uses.
//
//   m M = q L + p,  0 <= p < L:   y[m] = sum_{j : p + j L < T} h[p + j L] x[q - j]
//
// L outputs always consume exactly M inputs (one PERIOD).  A call whose first input has absolute index c starts with output
// m0 = ceil(c L / M); t0 = m0 M - c L in [0, M) is the only thing of the stream position the kernel needs: output i of the call
// (i = 0 .. count - 1) sits at t0 + i M of the L-times rate counted from the call's first input, so with i = b L + r
//   p = (t0 + r M) mod L = p_r,     q = b M + (t0 + r M) / L = b M + dq_r      (q relative to the call's first input)
// and the pattern (p_r, dq_r), r = 0 .. L - 1, is the same for every period b of the call.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "if_fir_stream_plan.h"

namespace if_fir
{

constexpr int RESAMP_MAX_L = 64;
constexpr int RESAMP_MAX_M = 64;
constexpr int RESAMP_MAX_TAPS = 4096;
constexpr int RESAMP_THREADS = 256; // one workgroup
constexpr int RESAMP_R = 4;         // outputs of one phase per lane
constexpr int RESAMP_X_MAX = 8192;  // input samples (float2) of one tile in LDS, overlap included

// phase taps: every phase's row has K entries, zero where p + j L >= T
inline int resamp_phase_taps(int T, int L)
{
    return (T + L - 1) / L;
}

// row stride of the tap table in entries: odd, so that the rows of 32 consecutive phases start on 32 different LDS banks
// (64 for the 8-byte entries of complex taps)
inline int resamp_row_stride(int K)
{
    return K | 1;
}

inline int resamp_hist_len(int T, int L)
{
    return resamp_phase_taps(T, L) - 1;
}

struct ResampShape
{
    int K;        // phase taps
    int KP;       // row stride of the tap table, entries
    int W;        // lanes of the workgroup that compute: the largest multiple of L <= RESAMP_THREADS (a lane keeps its phase)
    int B;        // periods per tile
    int tile_out; // B L outputs
    int tile_in;  // B M inputs
    int x_len;    // tile_in + K - 1 samples in LDS
    int tap_entries; // L KP
};

inline ResampShape resamp_shape(int T, int L, int M)
{
    ResampShape s;
    s.K = resamp_phase_taps(T, L);
    s.KP = resamp_row_stride(s.K);
    s.W = (RESAMP_THREADS / L) * L;
    s.B = s.W * RESAMP_R / L;
    const int fit = (RESAMP_X_MAX - (s.K - 1)) / M; // >= (8192 - 4095) / 64 = 64
    if (s.B > fit)
        s.B = fit;
    s.tile_out = s.B * L;
    s.tile_in = s.B * M;
    s.x_len = s.tile_in + s.K - 1;
    s.tap_entries = L * s.KP;
    return s;
}

inline size_t resamp_lds_bytes(const ResampShape &s, int ctaps)
{
    // taps first (4 or 8 bytes per entry, rounded up to 8), then the tile's samples
    const size_t taps = ((size_t)s.tap_entries * (ctaps ? 8 : 4) + 7) & ~(size_t)7;
    return taps + (size_t)s.x_len * 8;
}
// the largest resamp_lds_bytes over every (T, L, M): 64 rows of 65 complex entries + RESAMP_X_MAX samples, rounded up
constexpr int RESAMP_LDS_MAX = 8 * (RESAMP_MAX_TAPS + 2 * RESAMP_MAX_L) + 8 * RESAMP_X_MAX;

// entry r of a call's period table
IF_FIR_STREAM_HD inline void resamp_period_entry(int t0, int r, int L, int M, int *p, int *dq)
{
    const int v = t0 + r * M; // < 64 + 63 * 64
    *p = v % L;
    *dq = v / L;              // <= M - 1
}

struct ResampCall
{
    uint64_t m0;    // absolute index of the call's first output (mod 2^64)
    uint64_t count; // outputs the call emits
    uint32_t t0;    // m0 M - c L
};

// a call with n inputs at stream position c.  ceil(c L / M) with c = a M + b is a L + ceil(b L / M): no product of a 64-bit
// count, so nothing overflows short of c + n itself (refused)
inline bool resamp_call(uint64_t c, uint64_t n, int L, int M, ResampCall *out)
{
    if (c + n < c)
        return false;
    const uint64_t uL = (uint64_t)L, uM = (uint64_t)M;
    const uint64_t a0 = c / uM, b0 = c % uM, a1 = (c + n) / uM, b1 = (c + n) % uM;
    const uint64_t f0 = (b0 * uL + uM - 1) / uM, f1 = (b1 * uL + uM - 1) / uM; // <= L
    if (a1 - a0 > (UINT64_MAX - f1) / uL)
        return false;
    out->m0 = a0 * uL + f0;
    out->count = (a1 - a0) * uL + f1 - f0;
    out->t0 = (uint32_t)(f0 * uM - b0 * uL);
    return true;
}

// the phase-major table g[p][j] = h[p + j L] (zero where p + j L >= T), rows KP entries apart; out holds L KP entries (floats,
// or (re, im) pairs with ctaps).  The taps are copied as given: nothing is rounded.
inline void resamp_build_taps(const float *taps, int T, int ctaps, int L, float *out)
{
    const int K = resamp_phase_taps(T, L), KP = resamp_row_stride(K), w = ctaps ? 2 : 1;
    for (int i = 0; i < L * KP * w; i++)
        out[i] = 0.0f;
    for (int k = 0; k < T; k++)
        for (int e = 0; e < w; e++)
            out[((k % L) * KP + k / L) * w + e] = taps[k * w + e];
}

} // namespace if_fir
