// if_fir_rsynth_plan.h — host-side planning of the real-output polyphase synthesis bank (docs/SPEC.md §18): the
// size rules, the workspace of REAL transformed frames (4 M bytes a frame, half of §14's), where the half-size transform leaves
// the slot pair an output needs and the pre-tangle twiddles.  What a call emits from its stream position, how a long call is cut
// into chunks and the tap table are §14's word for word: if_fir_synth_plan.h, shared, not restated.  No HIP types: the shim, the
// kernel unit and tests/c/rsynth_plan_check.cpp (plain g++) all include this file, so what the checker walks is what the
// launcher uses.
//
//   y[n] = sum_m h[n - m L] ( Re X_0[m] + (-1)^n Re X_H[m] + 2 sum_{0<k<H} Re( X_k[m] e^{+j 2 pi k n / M} ) ),   H = M / 2
//
// Fold form: y[n] = sum_{j<J} h[t_j] v_{m_j}[n mod M] as in if_fir_synth_plan.h, with v_m[s] = sum_{k<M} X_k e^{+j 2 pi k s / M}
// REAL (X_{M-k} = conj X_k).  z[n] = v[2n] + j v[2n+1], n < H, is the inverse H-point transform of
//
//   Z_k = (X_k + conj X_{H-k}) + j W^k (X_k - conj X_{H-k}),   W = e^{+j 2 pi / M},   Z_0 = (Re X_0 + Re X_H, Re X_0 - Re X_H)
//
// and the inverse transform is the shared FORWARD one read at the mirrored bin: z[n] = F[(H - n) mod H].
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "if_fir_synth_plan.h" // synth_terms, synth_call, synth_chunk, synth_build_taps: §14's, shared; psd_bin_position

namespace if_fir
{

constexpr int RSYNTH_THREADS = SYNTH_THREADS; // one workgroup
constexpr int RSYNTH_MIN_M = 128;             // the transform is H = M/2 points: 64 .. 4096, so M = 128 .. 8192
constexpr int RSYNTH_MAX_ROWS = SYNTH_MAX_ROWS;   // T <= 16 M
constexpr int RSYNTH_MAX_TERMS = SYNTH_MAX_TERMS; // J = ceil(T / L)
constexpr uint64_t RSYNTH_MAX_CALL = SYNTH_MAX_CALL;                   // frames of one call
constexpr uint64_t RSYNTH_WORKSPACE_DEFAULT = SYNTH_WORKSPACE_DEFAULT; // bytes of transformed frames a chunk may hold
constexpr uint64_t RSYNTH_WORKSPACE_MAX = SYNTH_WORKSPACE_MAX;         // (a chunk's outputs are counted in 32 bits)

inline bool rsynth_size_ok(uint32_t M) { return M % 2 == 0 && stream_size_ok(M / 2, RSYNTH_MIN_M / 2); }

// M, T and L of a legal configuration (J <= 32 included)
inline bool rsynth_config_ok(uint32_t M, uint32_t T, uint32_t L)
{
    return rsynth_size_ok(M) && T >= 1 && T <= (uint32_t)RSYNTH_MAX_ROWS * M && L >= 1 && L <= M &&
           synth_terms(T, L) <= (uint32_t)RSYNTH_MAX_TERMS;
}

// the input span: channels first_bin .. first_bin + bins - 1 of 0 .. M/2, no wrap (§17's output span)
inline bool rsynth_span_ok(uint32_t first_bin, uint32_t bins, uint32_t M)
{
    return bins >= 1 && (uint64_t)first_bin + bins <= (uint64_t)M / 2 + 1;
}

// frames a workgroup transforms together: at least STREAM_BANK_POINTS points of the M/2-point transform
constexpr uint32_t rsynth_batch(uint32_t M) { return stream_bank_batch(M / 2); }

// lane items of a frame's pre-tangle: k = 0 .. H/2, item k makes Z_k and Z_{H-k} from X_k and X_{H-k}
constexpr uint32_t rsynth_pair_items(uint32_t M) { return M / 4 + 1; }

// LDS of one workgroup of the transform kernel: the batch's points, the transform's twiddles and the bin places, as the other
// banks at H points.  The pre-tangle twiddles stay in the L2-resident table, as §17's untangling twiddles do: in LDS they would
// cost a workgroup per CU from M = 2048 up (at M = 8192 one of two; measured there: 0.70 against 0.55 ms)
constexpr size_t rsynth_lds_bytes(uint32_t M) { return stream_bank_lds_bytes(M / 2); }

// workgroups a CU holds at a time
constexpr int rsynth_groups_per_cu(uint32_t M) { return stream_groups_per_cu(rsynth_lds_bytes(M)); }

// frames the workspace holds for a budget of `bytes`: a row is M floats; at least the J a single frame's outputs need
inline uint64_t rsynth_workspace_frames(uint64_t bytes, uint32_t M, uint32_t J)
{
    if (bytes > RSYNTH_WORKSPACE_MAX)
        bytes = RSYNTH_WORKSPACE_MAX;
    const uint64_t fit = bytes / ((uint64_t)M * 4);
    return fit > J ? fit : J;
}

// where the forward H-point transform leaves z[n] = v[2n] + j v[2n+1], n < H = M/2: bin (H - n) mod H
inline uint32_t rsynth_slot_place(uint32_t n, uint32_t M)
{
    return psd_bin_position((M / 2 - n) % (M / 2), M / 2);
}

// the pre-tangle twiddles W^k = e^{+j 2 pi k / M}, k = 0 .. H/2, as (re, im) pairs: float64 cos and sin, rounded once.  The
// kernel takes W^{H-k} = (-re, im) of entry k.  out holds M/4 + 1 pairs
inline void rsynth_build_twiddles(uint32_t M, float *out)
{
    for (uint32_t k = 0; k <= M / 4; k++)
    {
        const double ang = 6.283185307179586476925286766559 * (double)k / (double)M;
        out[2 * k] = (float)cos(ang);
        out[2 * k + 1] = (float)sin(ang);
    }
}

} // namespace if_fir
