// if_fir_subup_plan.h — host-side planning of the per-bin interpolating FIR stage over frames (docs/SPEC.md §16, DESIGN.md
// §3.21): the size rules with their messages, what one call emits from its stream position, how the (input frame, phase, bin)
// space of a call is dealt to lanes and workgroups, and the zero-padded tap-major table.  No HIP types: the shim, the kernel
// unit and tests/c/subup_plan_check.cpp (plain g++) all include this file, so what the checker walks is what the launcher uses.
//
//   y_j[m R + p] = e^{+j theta_j (m R + p)} sum_{i<J} h_r[p + i R] x_j[m - i],   x_j[m] = in[m B + j],   J = ceil(T / R)
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include "if_fir_stream_plan.h"

namespace if_fir
{

constexpr uint32_t SUBUP_MAX_BINS = 4096;
constexpr uint32_t SUBUP_MAX_TAPS = 2048;
constexpr uint32_t SUBUP_MAX_INTERPOLATION = 64;
constexpr uint32_t SUBUP_MAX_J = 32;                     // input frames an output weighs: ceil(T / R)
constexpr uint64_t SUBUP_MAX_FRAMES = (uint64_t)1 << 32; // of one call
constexpr int SUBUP_THREADS = 256;                       // one workgroup
constexpr int SUBUP_Q = 32;                              // consecutive input frames of one (bin, phase) a lane walks
// workgroups a CU holds at a time (no LDS; if_fir_subup.resources.txt): 230 VGPRs and 2 waves a SIMD with a window of 32 frames,
// 137 and 3 with 16, at most 84 with the smaller ones, where 4 are launched
constexpr int subup_groups_per_cu(int bucket)
{
    return bucket > 16 ? 2 : bucket > 8 ? 3 : 4;
}

inline uint32_t subup_j(uint32_t T, uint32_t R)
{
    return (T + R - 1) / R;
}

// the compile-time bound of the kernel's window for J frames: the next power of two (1, 2, 4, 8, 16, 32)
inline int subup_bucket(uint32_t J)
{
    int b = 1;
    while ((uint32_t)b < J)
        b *= 2;
    return b;
}

// The size rules of an init, in the order the shim checks them: the message (without its "if_fir_subup_init: " head) of the
// first rule broken goes to msg (256 bytes), or true.  have_taps: pfTaps is not NULL
inline bool subup_config_ok(uint32_t B, uint32_t T, uint32_t rows, uint32_t R, uint64_t max_frames, bool have_taps, char *msg)
{
    if (B < 1 || B > SUBUP_MAX_BINS)
        snprintf(msg, 256, "bins must be 1..%u (got %u)", SUBUP_MAX_BINS, B);
    else if (!have_taps || T < 1 || T > SUBUP_MAX_TAPS)
        snprintf(msg, 256, "taps must be 1..%u (got %u)%s", SUBUP_MAX_TAPS, T, have_taps ? "" : ", pfTaps is NULL");
    else if (rows != 1 && rows != B)
        snprintf(msg, 256, "tap rows must be 1 or the %u bins (got %u)", B, rows);
    else if (R < 1 || R > SUBUP_MAX_INTERPOLATION)
        snprintf(msg, 256, "interpolation must be 1..%u (got %u)", SUBUP_MAX_INTERPOLATION, R);
    else if (subup_j(T, R) > SUBUP_MAX_J)
        snprintf(msg, 256, "taps per phase J = ceil(%u / %u) = %u exceed %u", T, R, subup_j(T, R), SUBUP_MAX_J);
    else if (max_frames == 0 || max_frames > SUBUP_MAX_FRAMES)
        snprintf(msg, 256, "ullMaxFrames must be 1..2^32 (got %llu)", (unsigned long long)max_frames);
    else
        return true;
    return false;
}

struct SubUpCall
{
    uint64_t count; // output frames the call emits: F R
    uint32_t n0;    // low 32 bits of the first one's absolute index: (c R) mod 2^32
};

// a call with F frames at stream position c (input frames since init/reset): the outputs n in [c R, (c + F) R); refused when
// (c + F) R would pass 2^64 - 1.  The kernel is given call-relative frames and n0, never c.
inline bool subup_call(uint64_t c, uint64_t F, uint32_t R, SubUpCall *out)
{
    if (c + F < c || c + F > UINT64_MAX / R)
        return false;
    out->count = F * R;
    out->n0 = (uint32_t)(c * R); // (wraps mod 2^64, a multiple of 2^32)
    return true;
}

// The (input frame, phase, bin) space of a call dealt to lanes: an ITEM is one (bin j, phase p) over a RUN of SUBUP_Q
// consecutive input frames, that is SUBUP_Q outputs R frames apart; items are numbered with the bin fastest, then the phase,
// item = (run R + p) B + j, so consecutive lanes read consecutive bins of a frame and write consecutive elements of the output
// (output frame m R + p, bin j lies at (m R) B + (p B + j)) whatever B is, and only the last tile has idle lanes.  A TILE is
// SUBUP_THREADS consecutive items: what a workgroup takes per turn of its stride loop.
struct SubUpTiles
{
    uint64_t runs;  // ceil(F / SUBUP_Q)
    uint64_t items; // runs R B
    uint64_t tiles; // ceil(items / SUBUP_THREADS)
};

inline SubUpTiles subup_tiles(uint32_t B, uint32_t R, uint64_t F)
{
    SubUpTiles t;
    t.runs = F / SUBUP_Q + (F % SUBUP_Q ? 1 : 0);
    t.items = t.runs * R * B; // <= 2^27 2^6 2^12
    t.tiles = t.items / SUBUP_THREADS + (t.items % SUBUP_THREADS ? 1 : 0);
    return t;
}

// item -> (first input frame of the call, phase, bin)
IF_FIR_STREAM_HD inline void subup_item_place(uint64_t item, uint32_t B, uint32_t R, uint64_t *m0, uint32_t *p, uint32_t *j)
{
    const uint64_t t = item / B;
    *j = (uint32_t)(item - t * B);
    *p = (uint32_t)(t % R);
    *m0 = (t / R) * SUBUP_Q;
}

// the table is TAP-MAJOR and padded with zeros to J R taps: h_r[k] at entry k rows + r (a wave's lanes read consecutive bins,
// or all one entry), 0 for T <= k < J R: a lane's J taps are the entries p + i R, i < J, whatever p
inline size_t subup_table_place(uint32_t k, uint32_t r, uint32_t rows)
{
    return (size_t)k * rows + r;
}

inline size_t subup_table_floats(uint32_t T, uint32_t rows, uint32_t R)
{
    return (size_t)subup_j(T, R) * R * rows;
}

// taps is rows x T, out holds subup_table_floats()
inline void subup_build_table(const float *taps, uint32_t T, uint32_t rows, uint32_t R, float *out)
{
    const uint32_t padded = subup_j(T, R) * R;
    for (uint32_t k = 0; k < padded; k++)
        for (uint32_t r = 0; r < rows; r++)
            out[subup_table_place(k, r, rows)] = k < T ? taps[(size_t)r * T + k] : 0.0f;
}

} // namespace if_fir
