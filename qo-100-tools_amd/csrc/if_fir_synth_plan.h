// if_fir_synth_plan.h — host-side planning of the polyphase synthesis bank (docs/SPEC.md §14): the size rules,
// what a call emits from its stream position, how a long call is cut into chunks of a fixed workspace, the tap table in the
// order the kernel reads it and where the transform leaves the slot an output needs.  No HIP types: the shim, the kernel unit
// and tests/c/synth_plan_check.cpp (plain g++) all include this file, so what the checker walks is what the launcher uses.
//
//   y[n] = sum_k e^{+j 2 pi k n / M} sum_m h[n - m L] X_k[m],   n = absolute output index, 0 <= n - m L < T
//
// Fold form: y[n] = sum_{j<J} h[t_j] v_{m_j}[n mod M], m_j = floor(n / L) - j, t_j = (n mod L) + j L (terms with t_j >= T
// skipped), J = ceil(T / L).  v_m[s] = sum_k X_k[m] e^{+j 2 pi k s / M} = F_m[(M - s) mod M], F_m the FORWARD M-point transform
// of frame m: the shared transform as it stands, read at the mirrored bin.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "if_fir_psd_plan.h" // psd_bin_position: the shared transform's bin order

namespace if_fir
{

constexpr int SYNTH_THREADS = 256;        // one workgroup
constexpr int SYNTH_MAX_ROWS = 16;        // T <= 16 M
constexpr int SYNTH_MAX_TERMS = 32;       // J = ceil(T / L)
constexpr int SYNTH_BATCH_POINTS = STREAM_BANK_POINTS; // a workgroup transforms at least this many points at a time
constexpr uint64_t SYNTH_MAX_CALL = (uint64_t)1 << 32;         // frames of one call
constexpr uint64_t SYNTH_WORKSPACE_DEFAULT = (uint64_t)128 << 20; // bytes of transformed frames a chunk may hold (measured: DESIGN.md §3.19)
constexpr uint64_t SYNTH_WORKSPACE_MAX = (uint64_t)1 << 30;      // (a chunk's outputs are counted in 32 bits)

enum
{
    SYNTH_ROUTE_PLAN = 0,      // the plan's choice
    SYNTH_ROUTE_WORKSPACE = 1, // transform to a device workspace, then the taps: every legal configuration
    SYNTH_ROUTE_LDS = 2,       // one kernel with a ring of transformed batches in LDS: where synth_lds_route_fits
};

inline bool synth_size_ok(uint32_t M) { return stream_size_ok(M, 64); }

// terms of an output's chain: J = ceil(T / L)
inline uint32_t synth_terms(uint32_t T, uint32_t L)
{
    return (T + L - 1) / L;
}

// M, T and L of a legal configuration (J <= 32 included)
inline bool synth_config_ok(uint32_t M, uint32_t T, uint32_t L)
{
    return synth_size_ok(M) && T >= 1 && T <= (uint32_t)SYNTH_MAX_ROWS * M && L >= 1 && L <= M &&
           synth_terms(T, L) <= (uint32_t)SYNTH_MAX_TERMS;
}

// frames a workgroup transforms together
constexpr uint32_t synth_batch(uint32_t M) { return stream_bank_batch(M); }

// LDS of one workgroup of the transform kernel
constexpr size_t synth_lds_bytes(uint32_t M) { return stream_bank_lds_bytes(M); }
constexpr int SYNTH_LDS_PER_CU = STREAM_LDS_PER_CU;

// workgroups a CU holds at a time
constexpr int synth_groups_per_cu(uint32_t M) { return stream_groups_per_cu(synth_lds_bytes(M)); }

// LDS the one-kernel route would need: a ring of ceil((J-1)/B) + 1 transformed batches, the twiddles and the places; it fits
// where two workgroups of it share a CU
inline size_t synth_lds_route_bytes(uint32_t M, uint32_t J)
{
    const uint32_t B = synth_batch(M);
    return (size_t)((J - 1 + B - 1) / B + 1) * B * M * 8 + (size_t)M * 8 + (size_t)M * 2;
}
inline bool synth_lds_route_fits(uint32_t M, uint32_t J)
{
    return 2 * synth_lds_route_bytes(M, J) <= (size_t)SYNTH_LDS_PER_CU;
}

// workgroups of the one-kernel route a CU holds at a time; 0 where not one fits (synth_route refuses the route there)
inline int synth_lds_route_groups_per_cu(uint32_t M, uint32_t J)
{
    return synth_lds_route_bytes(M, J) > (size_t)SYNTH_LDS_PER_CU ? 0 : stream_groups_per_cu(synth_lds_route_bytes(M, J));
}

// the plan prefers the LDS ring where at least four workgroups of it share a CU: measured, it wins there (M = 64 and 256 of the
// bench rows, 17 and 34 KB) and loses at two workgroups a CU ((1024, 8 M, 1024), 74 KB: 1.23 ms against 0.84 ms); DESIGN.md §3.19
inline bool synth_lds_route_preferred(uint32_t M, uint32_t J)
{
    return synth_lds_route_fits(M, J) && synth_lds_route_groups_per_cu(M, J) >= 4;
}

// the route of a configuration: forced = SYNTH_ROUTE_PLAN gives the plan's choice; a forced LDS route that does not fit, or an
// unknown route, is refused (0)
inline uint32_t synth_route(uint32_t M, uint32_t J, uint32_t forced)
{
    if (forced == SYNTH_ROUTE_PLAN)
        return synth_lds_route_preferred(M, J) ? (uint32_t)SYNTH_ROUTE_LDS : (uint32_t)SYNTH_ROUTE_WORKSPACE;
    if (forced == SYNTH_ROUTE_WORKSPACE)
        return SYNTH_ROUTE_WORKSPACE;
    return forced == SYNTH_ROUTE_LDS && synth_lds_route_fits(M, J) ? (uint32_t)SYNTH_ROUTE_LDS : 0u;
}

// the one-kernel route deals RUNS of consecutive batches (a batch = synth_batch(M) frames, batch q = frames q B ..) to
// workgroups: `groups` workgroups at most, every run but the last of the same length
inline uint64_t synth_run_batches(uint64_t batches, uint64_t groups)
{
    return groups ? (batches + groups - 1) / groups : batches;
}

// frames the workspace holds for a budget of `bytes`: at least the J a single frame's outputs need
inline uint64_t synth_workspace_frames(uint64_t bytes, uint32_t M, uint32_t J)
{
    if (bytes > SYNTH_WORKSPACE_MAX)
        bytes = SYNTH_WORKSPACE_MAX;
    const uint64_t fit = bytes / ((uint64_t)M * 8);
    return fit > J ? fit : J;
}
// frames of the call one chunk emits the outputs of: the workspace less the J - 1 frames before them
inline uint64_t synth_chunk_frames(uint64_t workspace_frames, uint32_t J)
{
    return workspace_frames - (J - 1);
}

// a call of F frames takes ceil(F / chunk_frames) chunks; they are made equally long (the last may be shorter by less than
// their count) so that no chunk is a nearly empty pair of launches
inline uint64_t synth_even_chunk_frames(uint64_t F, uint64_t chunk_frames)
{
    const uint64_t chunks = (F + chunk_frames - 1) / chunk_frames;
    return chunks ? (F + chunks - 1) / chunks : chunk_frames;
}

struct SynthCall
{
    uint64_t outputs; // F L
    uint32_t smod;    // (c L) mod M: all the kernel learns of the stream position
    uint32_t carry;   // input frames kept for the next call: J - 1
};

// a call with F frames at frame index c: refused when (c + F) L would pass 2^64
inline bool synth_call(uint64_t c, uint64_t F, uint32_t M, uint32_t L, uint32_t T, SynthCall *out)
{
    if (c + F < c || L == 0 || M == 0 || T == 0 || c + F > UINT64_MAX / L)
        return false;
    out->outputs = F * L;
    out->smod = (uint32_t)((c * L) % M); // (c L < 2^64 here)
    out->carry = synth_terms(T, L) - 1;
    return true;
}

struct SynthChunk
{
    uint64_t first;   // first frame of the call whose outputs this chunk emits
    uint64_t frames;  // how many
    uint32_t smod;    // (absolute index of the chunk's first output) mod M
};

inline uint64_t synth_chunks(uint64_t F, uint64_t chunk_frames)
{
    return (F + chunk_frames - 1) / chunk_frames;
}
// chunk i of a call of F frames whose first output has index smod modulo M.  Its workspace holds the transforms of the frames
// first - (J-1) .. first + frames - 1 of the call (negative: the carried history), frame first - (J-1) in row 0
inline SynthChunk synth_chunk(uint64_t i, uint64_t F, uint64_t chunk_frames, uint32_t M, uint32_t L, uint32_t smod)
{
    SynthChunk ch;
    ch.first = i * chunk_frames;
    ch.frames = F - ch.first < chunk_frames ? F - ch.first : chunk_frames;
    ch.smod = (uint32_t)((smod + (ch.first % M) * L) % M);
    return ch;
}

// the table the kernel reads: entry j L + p = h[j L + p], zero where the index reaches T.  out holds J L floats.  Output n
// takes entries p + j L, p = n mod L, j = 0 .. J-1 in that order: consecutive outputs read consecutive entries
inline void synth_build_taps(const float *h, uint32_t T, uint32_t L, float *out)
{
    const uint32_t J = synth_terms(T, L);
    for (uint32_t t = 0; t < J * L; t++)
        out[t] = t < T ? h[t] : 0.0f;
}

// where the forward transform leaves what output slot s = n mod M needs: bin (M - s) mod M
inline uint32_t synth_slot_place(uint32_t s, uint32_t M)
{
    return psd_bin_position((M - s) % M, M);
}

// input element of channel k in a frame of a span that starts at first_bin (-M/2 <= first_bin < M): element j holds channel
// (first_bin + j) mod M, so j = (k - first_bin) mod M (M is a power of two); the span holds the channel when j < bins.  The
// kernels call this
IF_FIR_STREAM_HD inline uint32_t synth_channel_index(int32_t first_bin, uint32_t k, uint32_t M)
{
    return (uint32_t)((int32_t)k - first_bin) & (M - 1);
}

} // namespace if_fir
