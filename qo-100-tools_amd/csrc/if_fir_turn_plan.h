// if_fir_turn_plan.h — host-side planning of the corner turn (docs/SPEC.md §20): the rules of an init and of a
// call with their messages, the bin list and its inverse, the tile a shape gets, which (frame, column) pairs a workgroup owns
// in each of its two phases, and every element offset.  No HIP types: the shim, the kernel unit and tests/c/turn_plan_check.cpp
// (plain g++) all include this file, so what the checker walks is what the launcher uses.
//
//   TO_STREAMS:  out[c P + a] = conv(in[a B + sel[c]])                           columns = the C channels
//   TO_FRAMES:   out[a B + i] = conv(in[inv[i] P + a]), +0 where inv[i] is none    columns = the B bins
//
// A TILE is TURN_TILE = 4096 elements: X columns by 4096 / X frames, X the power of two at or above min(columns, 64).  A narrow
// selection so gets more frames per tile and a wave of the frame-side phase spans 64 / X frames: no lane idles.  A tile is
// exchanged through LDS as tile[f][j] with rows of pitch X | 1 elements.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "if_fir_stream_plan.h"

namespace if_fir
{

constexpr int TURN_THREADS = 256;                       // one workgroup
constexpr int TURN_TILE = 4096;                         // elements of a tile
constexpr int TURN_ITEMS = TURN_TILE / TURN_THREADS;    // elements a thread moves in each phase
constexpr int TURN_MAX_COLS = 64;                       // columns of the widest tile: one wave of the frame-side phase
constexpr uint32_t TURN_MAX_BINS = 8192;
constexpr uint64_t TURN_MAX_CALL_FRAMES = (uint64_t)1 << 32;
constexpr uint64_t TURN_MAX_PITCH = (uint64_t)1 << 40;  // 8192 rows of it, in bytes, stay far below 2^63
constexpr uint16_t TURN_NONE = 0xffff;                  // inv[i]: no channel lists bin i
constexpr uint32_t TURN_TO_STREAMS = 0, TURN_TO_FRAMES = 1;

// The rules of an init in the order the shim checks them: the configuration in the order of SPEC §20's table, then the list
// (sel: C indices, or nullptr for the span), then ullMaxFrames.  The message (without its "if_fir_turn_init: " head) of the
// first rule broken goes to msg (256 bytes), or true.
inline bool turn_config_ok(uint32_t direction, uint32_t B, uint32_t C, uint32_t first, uint32_t in_format, uint32_t out_format,
                           const uint32_t *sel, uint64_t max_frames, char *msg)
{
    if (direction > TURN_TO_FRAMES)
        snprintf(msg, 256, "unknown direction %u", direction);
    else if (B < 1 || B > TURN_MAX_BINS)
        snprintf(msg, 256, "bins must be 1..%u (got %u)", TURN_MAX_BINS, B);
    else if (C < 1 || C > B)
        snprintf(msg, 256, "channels must be 1..%u, the frame's bins (got %u)", B, C);
    else if ((uint64_t)first + C > B)
        snprintf(msg, 256, "bins [%u, %llu) of the span are outside the frame's %u", first, (unsigned long long)((uint64_t)first + C), B);
    else if (in_format > 1)
        snprintf(msg, 256, "unknown input format %u", in_format);
    else if (out_format > 1)
        snprintf(msg, 256, "unknown output format %u", out_format);
    else
    {
        if (sel)
        {
            if (first != 0)
            {
                snprintf(msg, 256, "ulFirst must be 0 beside a list of bins (got %u)", first);
                return false;
            }
            uint16_t place[TURN_MAX_BINS];
            memset(place, 0xff, sizeof place);
            for (uint32_t c = 0; c < C; c++)
            {
                if (sel[c] >= B)
                {
                    snprintf(msg, 256, "bin %u at place %u of the list is outside the frame's %u", sel[c], c, B);
                    return false;
                }
                if (place[sel[c]] != TURN_NONE)
                {
                    snprintf(msg, 256, "bin %u is listed twice (places %u and %u)", sel[c], (unsigned)place[sel[c]], c);
                    return false;
                }
                place[sel[c]] = (uint16_t)c;
            }
        }
        if (max_frames == 0 || max_frames > TURN_MAX_CALL_FRAMES)
            snprintf(msg, 256, "ullMaxFrames must be 1..2^32 (got %llu)", (unsigned long long)max_frames);
        else
            return true;
    }
    return false;
}

// the list of an accepted configuration, sel[c] (C values), and its inverse, inv[i] (B values, TURN_NONE where no channel lists i)
inline void turn_maps(uint32_t B, uint32_t C, uint32_t first, const uint32_t *list, uint16_t *sel, uint16_t *inv)
{
    for (uint32_t i = 0; i < B; i++)
        inv[i] = TURN_NONE;
    for (uint32_t c = 0; c < C; c++)
    {
        sel[c] = (uint16_t)(list ? list[c] : first + c);
        inv[sel[c]] = (uint16_t)c;
    }
}

// The rules of a call, in the order the shim checks them before it looks at the pointers
inline bool turn_call_ok(uint64_t frames, uint64_t pitch, uint64_t max_frames, char *msg)
{
    if (pitch < frames)
        snprintf(msg, 256, "a row pitch of %llu elements is below the call's %llu frames", (unsigned long long)pitch, (unsigned long long)frames);
    else if (pitch > TURN_MAX_PITCH)
        snprintf(msg, 256, "a row pitch of %llu elements is above 2^40", (unsigned long long)pitch);
    else if (frames > max_frames)
        snprintf(msg, 256, "%llu frames exceed ullMaxFrames %llu of init", (unsigned long long)frames, (unsigned long long)max_frames);
    else
        return true;
    return false;
}

// ---- the tile map ---------------------------------------------------------------------------------------------------------------
// A tile has X = 2^xs columns, the power of two at or above min(cols, 64), cols = C (TO_STREAMS) or B (TO_FRAMES).  The map
// is written with the shift, so that the kernel divides by no run-time value.
IF_FIR_STREAM_HD inline int turn_tile_shift(uint32_t cols)
{
    int xs = 0;
    while ((1 << xs) < TURN_MAX_COLS && ((uint32_t)1 << xs) < cols)
        xs++;
    return xs;
}

// frames of a tile, 64 .. 4096
IF_FIR_STREAM_HD inline int turn_tile_frames(int xs)
{
    return TURN_TILE >> xs;
}

// elements between the tile's rows in LDS: odd, so that the lanes of a column access (stride pitch elements) fall on distinct
// banks; X = 1 has one column and needs none
IF_FIR_STREAM_HD inline int turn_lds_pitch(int xs)
{
    return (1 << xs) | 1;
}

// LDS elements of a tile, at most 6144 (X = 2)
IF_FIR_STREAM_HD inline int turn_lds_elements(int xs)
{
    return turn_tile_frames(xs) * turn_lds_pitch(xs);
}

// tiles of a call: tiles_x column tiles (the fastest index) times the frame tiles
IF_FIR_STREAM_HD inline int64_t turn_tiles(uint32_t cols, uint64_t F, int xs, int64_t *tiles_x)
{
    *tiles_x = (int64_t)(((uint64_t)cols + ((uint64_t)1 << xs) - 1) >> xs);
    const uint64_t TF = (uint64_t)turn_tile_frames(xs);
    return *tiles_x * (int64_t)((F + TF - 1) / TF);
}

// tile t: its first column and its first frame
IF_FIR_STREAM_HD inline void turn_tile_origin(int64_t t, int64_t tiles_x, int xs, uint32_t *x0, uint64_t *a0)
{
    const int64_t ft = t / tiles_x;
    *x0 = (uint32_t)(t - ft * tiles_x) << xs;
    *a0 = (uint64_t)ft * (uint64_t)turn_tile_frames(xs);
}

// item k (0 .. TURN_ITEMS - 1) of thread `tid` in the phase whose lanes run ALONG A FRAME (its columns): column j and frame f
// inside the tile.  256 / X frames per step; j does not depend on k
IF_FIR_STREAM_HD inline void turn_item_along_frame(int k, int tid, int xs, int *j, int *f)
{
    const int idx = k * TURN_THREADS + tid;
    *j = idx & ((1 << xs) - 1);
    *f = idx >> xs;
}

// the same in the phase whose lanes run ALONG A ROW (its frames): the tile has 2^(12 - xs) >= 64 frames, so a wave has one column
IF_FIR_STREAM_HD inline void turn_item_along_row(int k, int tid, int xs, int *j, int *f)
{
    const int idx = k * TURN_THREADS + tid;
    *f = idx & (turn_tile_frames(xs) - 1);
    *j = idx >> (12 - xs);
}

// where an item lies in the LDS tile
IF_FIR_STREAM_HD inline int turn_lds_index(int j, int f, int xs)
{
    return f * turn_lds_pitch(xs) + j;
}

// element offsets, 64 bits: a B + i < 2^45, c P + a < 2^54 at the legal sizes
IF_FIR_STREAM_HD inline uint64_t turn_frame_offset(uint64_t a, uint32_t B, uint32_t i)
{
    return a * (uint64_t)B + i;
}

IF_FIR_STREAM_HD inline uint64_t turn_row_offset(uint32_t c, uint64_t P, uint64_t a)
{
    return (uint64_t)c * P + a;
}

static_assert(TURN_TILE == 1 << 12 && TURN_ITEMS * TURN_THREADS == TURN_TILE, "turn_item_along_row shifts by 12 - xs");

} // namespace if_fir
