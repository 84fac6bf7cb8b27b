// if_fir_psd_plan.h — host-side planning of the streaming power-spectrum estimator (docs/SPEC.md §8): which
// segments, chunks and frames a call completes from its stream position, and what it carries on.  No HIP types: the shim, the
// kernel unit and tests/c/psd_plan_check.cpp (plain g++) all include this file, so what the checker walks is what the launcher uses.
//
//   segment s = stream samples [s H, s H + N);  frame f = segments f K .. f K + K - 1;  a frame's segments are summed in CHUNKS of
//   PSD_CHUNK = 8 counted from the frame's first segment (the last chunk is shorter when 8 does not divide K).
//
// A chunk is only ever summed whole, so a call processes every chunk whose last sample it has and carries the samples of the
// first chunk it could not finish: fewer than 7 H + N of them.  The state between calls is (position, carried samples); the
// first segment of the open chunk is (position - carried) / H.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "if_fir_stream_plan.h"

namespace if_fir
{

constexpr int PSD_CHUNK = 8;      // segments per chunk (SPEC §8)
constexpr int PSD_THREADS = 256;  // one workgroup
constexpr int PSD_MIN_N = 256;
constexpr int PSD_MAX_N = 4096;
constexpr uint32_t PSD_MAX_SEGMENTS = 65535;
constexpr uint64_t PSD_MAX_CALL_SEGMENTS = (uint64_t)1 << 31; // segments of one call: psd_chunk_entry counts them in 32 bits

inline bool psd_size_ok(uint32_t N) { return stream_size_ok(N, PSD_MIN_N); }

// chunks of one frame
IF_FIR_STREAM_HD inline uint32_t psd_chunks_per_frame(uint32_t K)
{
    return (K + PSD_CHUNK - 1) / PSD_CHUNK;
}

struct PsdPlan
{
    uint64_t seg0;        // first segment of the open chunk = the first segment this call sums (read by the plan checker only)
    uint64_t segments;    // segments the call sums (whole chunks only)
    uint64_t chunks;      // chunks the call sums
    uint64_t frames;      // frames the call completes
    uint64_t carry;       // samples carried after the call: < 7 H + N
    uint32_t chunk0;      // index, inside its frame, of the call's first chunk (> 0: the open frame has an accumulator)
    uint32_t open_chunks; // chunks of the open frame already summed after the call (0: no accumulator is carried; read by the
                          // plan checker only)
};

// a call with n samples at stream position pos, `carried` samples of which are kept in the context.  Nothing multiplies a 64-bit
// count by anything that can overflow: every product below is bounded by pos + n, which is checked first.
inline bool psd_plan(uint64_t pos, uint64_t carried, uint64_t n, uint32_t N, uint32_t H, uint32_t K, PsdPlan *out)
{
    if (pos + n < pos || carried > pos || H == 0 || K == 0 || N == 0 || (pos - carried) % H)
        return false;
    const uint64_t total = pos + n;
    const uint64_t s0 = (pos - carried) / H;
    // segments 0 .. avail - 1 are complete at `total`
    const uint64_t avail = total < N ? 0 : (total - N) / H + 1;
    // the last chunk boundary at or before avail: boundaries sit at f K + min(8 c, K)
    const uint64_t fa = avail / K, ra = avail % K;
    uint64_t b = fa * K + (ra / PSD_CHUNK) * PSD_CHUNK;
    if (b < s0)
        b = s0; // (cannot happen from a state this function produced: s0 is a boundary <= the earlier avail)
    const uint64_t f0 = s0 / K, r0 = s0 % K;
    if (r0 % PSD_CHUNK)
        return false;
    const uint64_t cpf = psd_chunks_per_frame(K);
    const uint64_t fb = b / K, rb = b % K;
    out->seg0 = s0;
    out->segments = b - s0;
    out->chunks = (fb - f0) * cpf + rb / PSD_CHUNK - r0 / PSD_CHUNK;
    out->frames = fb - f0;
    out->carry = total - b * H; // b H <= avail H <= total - N + H <= total
    out->chunk0 = (uint32_t)(r0 / PSD_CHUNK);
    out->open_chunks = (uint32_t)(rb / PSD_CHUNK);
    return true;
}

// chunk c of a call whose first chunk is chunk0 of its frame: the chunk's first segment counted from the call's first segment,
// its segment count and the frame it belongs to counted from the call's first frame (the frame is for the plan checker: the
// frame kernel finds its chunks itself).  32-bit: if_fir_psd_init refuses a context whose largest call could reach
// PSD_MAX_CALL_SEGMENTS segments
IF_FIR_STREAM_HD inline void psd_chunk_entry(uint32_t chunk0, uint32_t c, uint32_t K, uint32_t *seg_rel, uint32_t *count, uint32_t *frame_rel)
{
    const uint32_t cpf = psd_chunks_per_frame(K);
    const uint32_t g = chunk0 + c, f = g / cpf, ci = g % cpf;
    const uint32_t left = K - ci * PSD_CHUNK;
    *seg_rel = f * K + ci * PSD_CHUNK - chunk0 * PSD_CHUNK;
    *count = left < (uint32_t)PSD_CHUNK ? left : (uint32_t)PSD_CHUNK;
    *frame_rel = f;
}

// the most chunks / frames a call of up to n samples can sum, whatever the stream position (carry < 7 H + N)
inline uint64_t psd_max_segments(uint64_t n, uint32_t H)
{
    return n / H + PSD_CHUNK + 1;
}
inline uint64_t psd_max_frames(uint64_t n, uint32_t H, uint32_t K)
{
    return psd_max_segments(n, H) / K + 1;
}
inline uint64_t psd_max_chunks(uint64_t n, uint32_t H, uint32_t K)
{
    const uint64_t segs = psd_max_segments(n, H), by_frame = (segs / K + 2) * psd_chunks_per_frame(K);
    return segs < by_frame ? segs : by_frame;
}

// the in-place decimation-in-frequency transform of the chunk kernel runs radix-4 passes and, for N = 512 and 2048, one last
// radix-2 pass; bin k ends at this position of the block (its digits reversed)
IF_FIR_STREAM_HD inline uint32_t psd_bin_position(uint32_t k, uint32_t N)
{
    uint32_t pos = 0, len = N;
    while (len > 1)
    {
        const uint32_t r = len >= 4 ? 4 : 2;
        pos += (k % r) * (len / r);
        k /= r;
        len /= r;
    }
    return pos;
}

} // namespace if_fir
