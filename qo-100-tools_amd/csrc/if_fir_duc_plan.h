// if_fir_duc_plan.h — host-side planning of the real-output up-converter (docs/SPEC.md §11): the shape of a
// tile, the tap table in the order the kernel reads it, and what one call emits from its stream position.  No HIP types: the
// shim, the kernel unit and tests/c/duc_plan_check.cpp (plain g++) all include this file, so what the checker walks is what the
// launcher uses.
//
//   y[q L + p] = sum_j ( g_r[p + j L] x'_r[q - j]  -  g_i[p + j L] x'_i[q - j] ),   g[k] = h[k] e^{+j theta k},  x'[n] = x[n] e^{+j theta L n}
//
// A tile is Q whole input samples and the L Q outputs they produce.  Its window of rotated samples x' lies in LDS as (re, im)
// pairs and starts KP - 1 samples before the tile's first input, KP = K = ceil(T / L) rounded up to even (the window is read two
// samples at a time): output q of the tile finds the sample of the row entry e at window index q + e, and entry e of the phase
// row p holds the tap j = KP - 1 - e, stored as (g_r, -g_i); entries with p + j L >= T are zero.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "if_fir_stream_plan.h"

namespace if_fir
{

constexpr int DUC_MAX_L = 64;
constexpr int DUC_MAX_TAPS = 4096;
constexpr int DUC_THREADS = 256;     // one workgroup: 4 waves
constexpr int DUC_R = 4;             // consecutive input positions q per lane: a wave covers DUC_RUN of one phase
constexpr int DUC_RUN = 64 * DUC_R;  // 256
constexpr int DUC_SEG = STREAM_SEG;  // phase taps per accumulation segment at most (SPEC §7, §11)
constexpr int DUC_TILE_OUT_MAX = 16384; // outputs of one tile at most (their staging area: 64 KB of float32)
constexpr int DUC_Q_MAX = 1024;
constexpr int DUC_DIV_SHIFT = 20;    // a tile's output index n < 16384 over L <= 64: n / L = (n duc_div_magic(L)) >> 20

// phase taps of the definition: ceil(T / L)
inline int duc_phase_taps(int T, int L)
{
    return (T + L - 1) / L;
}

// entries of a table row: the phase taps rounded up to even (the zero entry is the OLDEST: it adds +0 to a segment that starts at +0)
inline int duc_row_taps(int T, int L)
{
    return (duc_phase_taps(T, L) + 1) & ~1;
}

inline uint32_t duc_div_magic(int L)
{
    return ((1u << DUC_DIV_SHIFT) + (uint32_t)L - 1) / (uint32_t)L;
}

struct DucShape
{
    int K;        // phase taps, ceil(T / L)
    int KP;       // entries of a table row, K rounded up to even
    int top;      // entries of a row's first (oldest) segment: K - 16 floor((K - 1) / 16), plus the zero entry when K is odd; even
    int Q;        // inputs per tile, a multiple of DUC_RUN
    int tile_out; // L Q outputs
    int window;   // Q + KP - 1 samples the fill writes; one more is read (never used) by the last lane's look-ahead
    int RS;       // stride in floats between the phases of the output staging area: Q + 4
    int x_floats; // 2 (Q + KP): the window, (re, im) pairs
    int tap_entries; // L KP (g_r, -g_i) pairs
};

inline DucShape duc_shape(int T, int L)
{
    DucShape s;
    s.K = duc_phase_taps(T, L);
    s.KP = duc_row_taps(T, L);
    s.top = stream_top_segment(s.K) + (s.KP - s.K);
    int runs = DUC_TILE_OUT_MAX / (DUC_RUN * L); // >= 1
    if (runs > DUC_Q_MAX / DUC_RUN)
        runs = DUC_Q_MAX / DUC_RUN;
    s.Q = runs * DUC_RUN;
    s.tile_out = s.Q * L;
    s.window = s.Q + s.KP - 1;
    s.RS = s.Q + 4;
    s.x_floats = 2 * (s.Q + s.KP);
    s.tap_entries = L * s.KP;
    return s;
}

// LDS: the window, then the staging area of the tile's outputs (phase-major, one float each)
inline size_t duc_lds_bytes(const DucShape &s, int L)
{
    return ((size_t)s.x_floats + (size_t)s.RS * L) * 4;
}
// an upper bound for every shape (the longest window and the largest staging area do not occur together)
constexpr int DUC_LDS_MAX = (2 * (DUC_Q_MAX + DUC_MAX_TAPS) + (DUC_RUN + 4) * DUC_MAX_L) * 4;
constexpr int DUC_LDS_PER_CU = STREAM_LDS_PER_CU;

// workgroups of this shape a CU holds at a time
inline int duc_groups_per_cu(const DucShape &s, int L) { return stream_groups_per_cu(duc_lds_bytes(s, L)); }

// a call with n inputs at stream position c (inputs since init/reset) emits the n L outputs from c L on; refused when
// (c + n) L does not fit 64 bits
inline bool duc_call(uint64_t c, uint64_t n, int L, uint64_t *count)
{
    if (c + n < c || c + n > UINT64_MAX / (uint64_t)L)
        return false;
    *count = n * (uint64_t)L;
    return true;
}

// g[k] = h[k] e^{+j theta k} stored as (g_r, -g_i) (the negation is exact: stream_mix_taps has rounded already); P = 0:
// (h_r, -h_i).  out holds T pairs
inline void duc_mix_taps(const float *taps, int T, int ctaps, uint32_t word, float *out)
{
    stream_mix_taps(taps, T, ctaps, word, out);
    for (int k = 0; k < T; k++)
        out[2 * k + 1] = -out[2 * k + 1];
}

// the table the kernel reads front to back: entry p KP + e = the pair of the tap p + j L with j = KP - 1 - e, zero where
// p + j L >= T.  g: the T pairs of duc_mix_taps; out holds L KP pairs
inline void duc_build_table(const float *g, int T, int L, float *out)
{
    const int KP = duc_row_taps(T, L);
    for (int i = 0; i < 2 * L * KP; i++)
        out[i] = 0.0f;
    for (int k = 0; k < T; k++)
    {
        const int p = k % L, e = KP - 1 - k / L;
        out[2 * (p * KP + e)] = g[2 * k];
        out[2 * (p * KP + e) + 1] = g[2 * k + 1];
    }
}

// output sample in float32 to int16 (SPEC §11): times 2^15 (exact), to nearest even, saturated (not a number: 0); the kernel
// calls this very function
IF_FIR_STREAM_HD inline int16_t duc_to_i16(float v)
{
    const float s = nearbyintf(v * 32768.0f);
    return (int16_t)(s < -32768.0f ? -32768.0f : s > 32767.0f ? 32767.0f : s == s ? s : 0.0f);
}

} // namespace if_fir
