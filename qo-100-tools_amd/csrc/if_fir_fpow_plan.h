// if_fir_fpow_plan.h — host-side planning of the frame power stage (docs/SPEC.md §19): the size rules with their
// messages, which chunks and output frames a call touches from its stream position, what it carries on, and the size of the
// workspace of chunk sums.  No HIP types: the shim, the kernel unit and tests/c/fpow_plan_check.cpp (plain g++) all include this
// file, so what the checker walks is what the launcher uses.
//
//   output frame f = input frames f K .. f K + K - 1;  a frame's per-frame powers e_a are summed in CHUNKS of FPOW_CHUNK = 8
//   counted from the frame's first input frame (the last chunk is shorter when 8 does not divide K).
//
// A chunk sum is sequential from +0, so a call that ends inside a chunk carries the partial sum and the next call goes on adding:
// the state between calls is (position, the open frame's accumulator of finished chunks, the open chunk's partial sum).  How
// many chunks the accumulator holds and how many frames the partial are read off the position: (c mod K) / 8 and (c mod K) mod 8.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include "if_fir_stream_plan.h"

namespace if_fir
{

constexpr int FPOW_CHUNK = 8;                           // input frames per chunk (SPEC §19, as §8's segments)
constexpr int FPOW_THREADS = 256;                       // one workgroup
constexpr int FPOW_GROUPS_PER_CU = 8;                   // no LDS; the kernels' registers hold 8 waves a SIMD (if_fir_fpow.resources.txt)
constexpr uint32_t FPOW_MAX_BINS = 8192;
constexpr uint32_t FPOW_MAX_GROUP = 64;
constexpr uint32_t FPOW_MAX_FRAMES = 65535;             // K
constexpr uint64_t FPOW_MAX_CALL_FRAMES = (uint64_t)1 << 32;
constexpr uint64_t FPOW_MAX_WORK = (uint64_t)1 << 29;   // float32 values of the workspace (§8's rule)

// chunks of one output frame
IF_FIR_STREAM_HD inline uint32_t fpow_chunks_per_frame(uint32_t K)
{
    return (K + FPOW_CHUNK - 1) / FPOW_CHUNK;
}

// the most chunks a call of up to n frames can touch, whatever the stream position: every chunk touched holds a frame of the
// call, and a call touches at most n / K + 2 output frames
inline uint64_t fpow_max_chunks(uint64_t n, uint32_t K)
{
    const uint64_t by_frame = (n / K + 2) * fpow_chunks_per_frame(K);
    return n < by_frame ? n : by_frame;
}

// The size rules of an init, in the order the shim checks them: the message (without its "if_fir_fpow_init: " head) of the first
// rule broken goes to msg (256 bytes), or true.  norm_ok / ref_ok: the value is finite and > 0 (the caller tests the floats)
inline bool fpow_config_ok(uint32_t B, uint32_t first, uint32_t G, uint32_t Bo, uint32_t K, bool norm_ok, bool ref_ok, uint32_t format,
                           uint64_t max_frames, char *msg)
{
    if (B < 1 || B > FPOW_MAX_BINS)
        snprintf(msg, 256, "bins must be 1..%u (got %u)", FPOW_MAX_BINS, B);
    else if (G < 1 || G > FPOW_MAX_GROUP)
        snprintf(msg, 256, "group must be 1..%u (got %u)", FPOW_MAX_GROUP, G);
    else if (Bo < 1 || (uint64_t)first + (uint64_t)G * Bo > B)
        snprintf(msg, 256, "elements [%u, %llu) of %u output bins in groups of %u are outside the frame's %u (ulOutBins >= 1)", first,
                 (unsigned long long)((uint64_t)first + (uint64_t)G * Bo), Bo, G, B);
    else if (K < 1 || K > FPOW_MAX_FRAMES)
        snprintf(msg, 256, "frames per output frame must be 1..%u (got %u)", FPOW_MAX_FRAMES, K);
    else if (!norm_ok)
        snprintf(msg, 256, "fNorm must be a finite value > 0");
    else if (!ref_ok)
        snprintf(msg, 256, "fRefPower must be a finite value > 0");
    else if (format > 1)
        snprintf(msg, 256, "unknown input format %u", format);
    else if (max_frames == 0 || max_frames > FPOW_MAX_CALL_FRAMES)
        snprintf(msg, 256, "ullMaxFrames must be 1..2^32 (got %llu)", (unsigned long long)max_frames);
    else if (fpow_max_chunks(max_frames, K) * Bo > FPOW_MAX_WORK)
        snprintf(msg, 256, "a call of ullMaxFrames = %llu frames would need %llu chunk sums of %u bins; the workspace is limited to 2^29 "
                           "values: lower ullMaxFrames", (unsigned long long)max_frames, (unsigned long long)fpow_max_chunks(max_frames, K), Bo);
    else
        return true;
    return false;
}

struct FpowPlan
{
    uint64_t chunks;      // chunks the call touches (finished or not), counted from the open one
    uint64_t done;        // of these, the first `done` are finished by the call
    uint64_t frames;      // output frames the call completes
    uint64_t touched;     // output frames the call touches: frames, and one more when it leaves a frame open
    uint32_t chunk0;      // index, inside its output frame, of the call's first chunk (> 0: the open frame has an accumulator)
    uint32_t skip;        // input frames of that chunk summed by earlier calls (> 0: the open chunk has a partial sum)
    uint32_t open_chunks; // finished chunks of the open frame after the call (read by the plan checker and the shim)
    uint32_t open_frames; // input frames in the open chunk's partial sum after the call
};

// a call with F frames at stream position c (input frames since init/reset); c + F past 2^64 is refused, nothing written
inline bool fpow_plan(uint64_t c, uint64_t F, uint32_t K, FpowPlan *out)
{
    if (c + F < c || K == 0 || F > FPOW_MAX_CALL_FRAMES)
        return false;
    const uint32_t r = (uint32_t)(c % K), cpf = fpow_chunks_per_frame(K);
    const uint64_t end = (uint64_t)r + F; // < 2^16 + 2^32, counted from the open frame's first input frame
    const uint64_t fe = end / K;
    const uint32_t re = (uint32_t)(end % K);
    out->chunk0 = r / FPOW_CHUNK;
    out->skip = r % FPOW_CHUNK;
    out->open_chunks = re / FPOW_CHUNK;
    out->open_frames = re % FPOW_CHUNK;
    out->frames = fe;
    out->touched = F ? fe + (re ? 1 : 0) : 0;
    out->done = fe * cpf + out->open_chunks - out->chunk0;
    out->chunks = F ? out->done + (out->open_frames ? 1 : 0) : 0;
    if (F == 0)
        out->done = 0;
    return true;
}

// chunk q of a call (plan's chunk0 and skip, r = chunk0 * 8 + skip = c mod K): the rows of the call's input it sums,
// [*row0, *row0 + *count) clipped to the call's F frames (count >= 1 for q < plan.chunks), and whether it starts from the carried
// partial sum.  32-bit chunk index: an init refuses a context whose largest call could touch more than 2^29 chunks
IF_FIR_STREAM_HD inline void fpow_chunk_entry(uint32_t chunk0, uint32_t skip, uint32_t q, uint32_t K, uint64_t F, uint64_t *row0,
                                              uint32_t *count, bool *from_partial)
{
    const uint32_t cpf = fpow_chunks_per_frame(K);
    const uint32_t g = chunk0 + q, t = g / cpf, ci = g % cpf;
    const uint32_t left = K - ci * FPOW_CHUNK;
    const uint32_t len = left < (uint32_t)FPOW_CHUNK ? left : (uint32_t)FPOW_CHUNK;
    const uint64_t r = (uint64_t)chunk0 * FPOW_CHUNK + skip;
    const uint64_t beg = (uint64_t)t * K + (uint64_t)ci * FPOW_CHUNK; // from the open frame's first input frame
    const uint64_t lo = beg > r ? beg - r : 0;                         // (beg < r only for q = 0)
    uint64_t hi = beg + len - r;
    if (hi > F)
        hi = F;
    *row0 = lo;
    *count = (uint32_t)(hi - lo);
    *from_partial = q == 0 && skip > 0;
}

// output frame t of a call (0 = the open one): its finished chunks of this call are the call-relative [*lo, *hi); *complete when
// the call finishes its last chunk
IF_FIR_STREAM_HD inline void fpow_frame_entry(uint32_t chunk0, uint64_t done, uint32_t t, uint32_t K, uint64_t *lo, uint64_t *hi,
                                              bool *complete)
{
    const uint64_t cpf = fpow_chunks_per_frame(K);
    const uint64_t fbeg = (uint64_t)t * cpf, end = fbeg + cpf - chunk0;
    *lo = fbeg > chunk0 ? fbeg - chunk0 : 0;
    *complete = end <= done;
    *hi = *complete ? end : done;
}

// the scale of SPEC §19: 1 / (K G fNorm) in float64, rounded once
inline float fpow_scale(uint32_t K, uint32_t G, float norm)
{
    return (float)(1.0 / ((double)K * (double)G * (double)norm));
}

} // namespace if_fir
