// if_fir_sub_plan.h — host-side planning of the per-channel FIR stage over filter-bank frames (docs/SPEC.md §15, DESIGN.md
// §3.20): the size rules with their messages, what one call emits from its stream position, how the (output, bin) plane of a
// call is dealt to lanes and workgroups, and the tap-major table of NCO-shifted taps.  No HIP types: the shim, the kernel unit and
// tests/c/sub_plan_check.cpp (plain g++) all include this file, so what the checker walks is what the launcher uses.
//
//   y_j[n] = e^{-j theta_j n R} sum_k g_j[k] x_j[n R - k],   g_j[k] = h_r[k] e^{+j theta_j k},   x_j[a] = in[a B + j]
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include "if_fir_stream_plan.h"

namespace if_fir
{

constexpr uint32_t SUB_MAX_BINS = 4096;
constexpr uint32_t SUB_MAX_TAPS = 128;
constexpr uint32_t SUB_MAX_DECIMATION = 64;
constexpr uint64_t SUB_MAX_FRAMES = (uint64_t)1 << 32; // of one call
constexpr int SUB_THREADS = 256;                       // one workgroup
constexpr int SUB_OUT = 4;                             // consecutive outputs of one bin a lane computes in registers
constexpr int SUB_UNROLL = 4;                          // taps of a segment in flight: SUB_UNROLL (SUB_OUT + 1) loads per lane
constexpr int SUB_GROUPS_PER_CU = 2;                   // no LDS; the kernel's registers hold 2 waves a SIMD (if_fir_sub.resources.txt)

// The size rules of an init, in the order the shim checks them: the message (without its "if_fir_sub_init: " head) of the first
// rule broken goes to msg (256 bytes), or true.  have_taps: pfTaps is not NULL
inline bool sub_config_ok(uint32_t B, uint32_t T, uint32_t rows, uint32_t R, uint64_t max_frames, bool have_taps, char *msg)
{
    if (B < 1 || B > SUB_MAX_BINS)
        snprintf(msg, 256, "bins must be 1..%u (got %u)", SUB_MAX_BINS, B);
    else if (!have_taps || T < 1 || T > SUB_MAX_TAPS)
        snprintf(msg, 256, "taps must be 1..%u (got %u)%s", SUB_MAX_TAPS, T, have_taps ? "" : ", pfTaps is NULL");
    else if (rows != 1 && rows != B)
        snprintf(msg, 256, "tap rows must be 1 or the %u bins (got %u)", B, rows);
    else if (R < 1 || R > SUB_MAX_DECIMATION)
        snprintf(msg, 256, "decimation must be 1..%u (got %u)", SUB_MAX_DECIMATION, R);
    else if (max_frames == 0 || max_frames > SUB_MAX_FRAMES)
        snprintf(msg, 256, "ullMaxFrames must be 1..2^32 (got %llu)", (unsigned long long)max_frames);
    else
        return true;
    return false;
}

struct SubCall
{
    uint64_t count; // output frames the call emits
    uint32_t n0;    // offset in the call's input of the frame under the first of them, 0 <= n0 < R
    uint32_t a0;    // low 32 bits of that frame's absolute index (meaningful when count > 0)
};

// a call with F frames at stream position c (frames since init/reset): the outputs at absolute a in [c, c + F) with a mod R == 0;
// c + F past 2^64 is refused.  The kernel is given n0 and a0, never c.
inline bool sub_call(uint64_t c, uint64_t F, uint32_t R, SubCall *out)
{
    if (!stream_decim_call(c, F, (uint64_t)R, &out->n0, &out->count))
        return false;
    out->a0 = (uint32_t)(c + out->n0);
    return true;
}

// The (output, bin) plane of a call dealt to lanes: an ITEM is SUB_OUT consecutive outputs of one bin; items are numbered with
// the bin fastest, item = (o / SUB_OUT) B + j, so consecutive lanes read and write consecutive bins whatever B is and only the
// last tile has idle lanes.  A TILE is SUB_THREADS consecutive items: what a workgroup takes per turn of its stride loop.
struct SubTiles
{
    uint64_t runs;  // runs of SUB_OUT outputs: ceil(count / SUB_OUT)
    uint64_t items; // runs B
    uint64_t tiles; // ceil(items / SUB_THREADS)
};

inline SubTiles sub_tiles(uint32_t B, uint64_t count)
{
    SubTiles t;
    t.runs = count / SUB_OUT + (count % SUB_OUT ? 1 : 0);
    t.items = t.runs * B; // <= 2^30 2^12
    t.tiles = t.items / SUB_THREADS + (t.items % SUB_THREADS ? 1 : 0);
    return t;
}

// item -> (first output, bin)
inline void sub_item_place(uint64_t item, uint32_t B, uint64_t *o0, uint32_t *j)
{
    *o0 = (item / B) * SUB_OUT;
    *j = (uint32_t)(item % B);
}

// the table is TAP-MAJOR: g_j[k] at entry k B + j (a wave's lanes read consecutive bins)
inline size_t sub_table_place(uint32_t k, uint32_t j, uint32_t B)
{
    return (size_t)k * B + j;
}

// the whole table for the phase words word[0 .. B-1]: taps is rows x T (rows = 1: one row for all bins), out holds T B (re, im)
// pairs, row is scratch for T pairs.  stream_mix_taps: float64, rounded once, word 0 gives g = h exactly
inline void sub_build_table(const float *taps, uint32_t T, uint32_t rows, uint32_t B, const uint32_t *word, float *row, float *out)
{
    for (uint32_t j = 0; j < B; j++)
    {
        stream_mix_taps(taps + (rows == 1 ? 0 : (size_t)j * T), (int)T, 0, word[j], row);
        for (uint32_t k = 0; k < T; k++)
        {
            out[2 * sub_table_place(k, j, B)] = row[2 * k];
            out[2 * sub_table_place(k, j, B) + 1] = row[2 * k + 1];
        }
    }
}

} // namespace if_fir
