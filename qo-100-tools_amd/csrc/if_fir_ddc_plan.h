// if_fir_ddc_plan.h — host-side planning of the real-input down-converter (docs/SPEC.md §10): the shape of a
// tile, the tap table in the order the kernel reads it, and what one call emits from its stream position.  No HIP types: the
// shim, the kernel unit and tests/c/ddc_plan_check.cpp (plain g++) all include this file, so what the checker walks is what the
// launcher uses.
//
//   y[n] = e^{-j theta n} sum_k g[k] r[n - k],   g[k] = h[k] e^{+j theta k},   outputs at n = m D
//
// Polyphase form: k = rho + j D.  A tile's window of real samples lies in LDS de-interleaved into D rows (window sample w in row
// w mod D, column w / D); the window starts K D - 1 samples before the tile's first output, so output i of the tile reads, for
// the tap (rho, j), row D - 1 - rho, column K - 1 - j + i: row R = D - 1 - rho is a K-tap FIR over a contiguous run of its row.
// K = ceil(T / D) rounded up to a multiple of 4 (the rows are read 16 bytes at a time); taps beyond T are zero.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "if_fir_stream_plan.h"

namespace if_fir
{

constexpr int DDC_MAX_D = 64;
constexpr int DDC_MAX_TAPS = 4096;
constexpr int DDC_THREADS = 256;   // one workgroup
constexpr int DDC_R = 4;           // consecutive outputs per lane
constexpr int DDC_SEG = STREAM_SEG; // taps per accumulation segment at most (SPEC §10)
constexpr int DDC_X_MAX = 16384;   // real samples (float) of one tile's window in LDS, row padding included: 64 KB

// taps per phase row: ceil(T / D) rounded up to a multiple of 4
inline int ddc_row_taps(int T, int D)
{
    return ((T + D - 1) / D + 3) & ~3;
}

// whole rows joined into one accumulation segment: floor(16 / K) when a row has at most 16 taps, else a row is cut (1)
inline int ddc_rows_per_segment(int K)
{
    return K <= DDC_SEG ? DDC_SEG / K : 1;
}

struct DdcShape
{
    int K;        // taps per row, a multiple of 4
    int G;        // rows per segment
    int tile_out; // outputs per tile, a multiple of 4
    int tile_in;  // tile_out D inputs
    int cols;     // tile_out + K columns used in every row (the window is cols D samples; the last is read as padding only)
    int RS;       // row stride in floats: a multiple of 4 with RS / 4 odd
    int tap_entries; // D K complex entries
};

inline DdcShape ddc_shape(int T, int D)
{
    DdcShape s;
    s.K = ddc_row_taps(T, D);
    s.G = ddc_rows_per_segment(s.K);
    // the largest row stride that fits, then the columns it leaves for outputs
    int rs = (DDC_X_MAX / D) & ~3;      // >= 256
    if ((rs / 4) % 2 == 0)
        rs -= 4;
    int out = rs - s.K;                 // >= 252 - 64
    if (out > DDC_THREADS * DDC_R)
        out = DDC_THREADS * DDC_R;
    s.tile_out = out;
    s.tile_in = out * D;
    s.cols = out + s.K;
    s.RS = s.cols;
    if ((s.RS / 4) % 2 == 0)
        s.RS += 4;
    s.tap_entries = D * s.K;
    return s;
}

inline size_t ddc_lds_bytes(const DdcShape &s, int D)
{
    return (size_t)s.RS * D * 4;
}
constexpr int DDC_LDS_MAX = DDC_X_MAX * 4;
constexpr int DDC_LDS_PER_CU = STREAM_LDS_PER_CU;

// workgroups of this shape a CU holds at a time
inline int ddc_groups_per_cu(const DdcShape &s, int D) { return stream_groups_per_cu(ddc_lds_bytes(s, D)); }

struct DdcCall
{
    uint64_t first; // absolute index of the input sample under the call's first output (meaningful when count > 0)
    uint64_t count; // outputs the call emits
    uint32_t n0;    // offset of that sample in the call's input, 0 <= n0 < D
};

// a call with n inputs at stream position c: the outputs at absolute n in [c, c + n) with n mod D == 0; c + n past 2^64 is refused
inline bool ddc_call(uint64_t c, uint64_t n, int D, DdcCall *out)
{
    if (!stream_decim_call(c, n, (uint64_t)D, &out->n0, &out->count))
        return false;
    out->first = c + out->n0; // < c + n when count > 0
    return true;
}

// g[k] = h[k] e^{+j theta k}: out holds T (re, im) pairs
inline void ddc_mix_taps(const float *taps, int T, int ctaps, uint32_t word, float *out) { stream_mix_taps(taps, T, ctaps, word, out); }

// the table the kernel reads front to back: entry R K + e = g[rho + j D] with rho = D - 1 - R, j = K - 1 - e, zero where
// rho + j D >= T.  g: T (re, im) pairs; out holds D K pairs
inline void ddc_build_table(const float *g, int T, int D, float *out)
{
    const int K = ddc_row_taps(T, D);
    for (int i = 0; i < 2 * D * K; i++)
        out[i] = 0.0f;
    for (int k = 0; k < T; k++)
    {
        const int R = D - 1 - k % D, e = K - 1 - k / D;
        out[2 * (R * K + e)] = g[2 * k];
        out[2 * (R * K + e) + 1] = g[2 * k + 1];
    }
}

} // namespace if_fir
