// if_fir_pfb_plan.h — host-side planning of the polyphase filter bank (docs/SPEC.md §13): which frames a call
// emits from its stream position, how the frames are dealt to workgroups, the tap table in the order the kernel reads it and
// where the transform leaves a bin.  No HIP types: the shim, the kernel unit and tests/c/pfb_plan_check.cpp (plain g++) all
// include this file, so what the checker walks is what the launcher uses.
//
//   y_k[m] = sum_{t<T} h[t] x[a-t] e^{-j 2 pi k (a-t) / M},   a = m D
//
// Fold form: slot s of an M-point buffer holds u[s] = sum of h[t] x[a-t] over the t < T with (a - t) mod M == s; y_k[m] is the
// forward M-point transform of u.  With t = t0 + r M, t0 = M-1-q: slot (a + 1 + q) mod M sums its K = ceil(T/M) terms in the
// order r = 0, 1, ..., K-1.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "if_fir_psd_plan.h" // psd_bin_position: the shared transform's bin order

namespace if_fir
{

constexpr int PFB_THREADS = 256;        // one workgroup
constexpr int PFB_MIN_M = 64;
constexpr int PFB_MAX_M = 4096;
constexpr int PFB_MAX_ROWS = 16;        // K = ceil(T / M)
constexpr int PFB_BATCH_POINTS = STREAM_BANK_POINTS; // a workgroup transforms at least this many points at a time
constexpr uint64_t PFB_MAX_CALL = (uint64_t)1 << 40; // samples of one call

inline bool pfb_size_ok(uint32_t M) { return stream_size_ok(M, PFB_MIN_M); }

// rows of the tap table: K = ceil(T / M)
inline uint32_t pfb_rows(uint32_t T, uint32_t M)
{
    return (T + M - 1) / M;
}

// frames a workgroup folds and transforms together
constexpr uint32_t pfb_batch(uint32_t M) { return stream_bank_batch(M); }

// consecutive frames one workgroup owns: whole batches, at least 8 frames (consecutive frames read overlapping inputs)
constexpr uint32_t pfb_group_frames(uint32_t M)
{
    return 2 * pfb_batch(M) > 8u ? 2 * pfb_batch(M) : 8u;
}

struct PfbCall
{
    uint64_t frames; // frames the call emits
    uint64_t groups; // runs of pfb_group_frames frames (the last may be short)
    uint32_t n0;     // offset in the call's input of the sample under its first frame, 0 <= n0 < D (meaningful when frames > 0)
    uint32_t cmod;   // c mod M: all the kernel learns of the stream position
    uint32_t carry;  // samples kept for the next call: T - 1
};

// a call with n inputs at stream position c: the frames m with m D in [c, c + n).  Nothing overflows short of c + n itself
// (refused)
inline bool pfb_call(uint64_t c, uint64_t n, uint32_t M, uint32_t D, uint32_t T, PfbCall *out)
{
    if (D == 0 || M == 0 || T == 0 || !stream_decim_call(c, n, D, &out->n0, &out->frames))
        return false;
    const uint64_t gf = pfb_group_frames(M);
    out->groups = out->frames / gf + (out->frames % gf ? 1 : 0);
    out->cmod = (uint32_t)(c % M);
    out->carry = T - 1;
    return true;
}

// the table the kernel reads front to back: entry r M + q = h[r M + (M-1-q)], the taps of a row time-reversed, zero where the
// index reaches T.  out holds pfb_rows(T, M) M floats
inline void pfb_build_taps(const float *h, uint32_t T, uint32_t M, float *out)
{
    const uint32_t K = pfb_rows(T, M);
    for (uint32_t r = 0; r < K; r++)
        for (uint32_t q = 0; q < M; q++)
        {
            const uint32_t t = r * M + (M - 1 - q);
            out[(size_t)r * M + q] = t < T ? h[t] : 0.0f;
        }
}

// where the transform leaves output bin j of a span that starts at first_bin (-M/2 <= first_bin < M): channel (first_bin + j) mod M
inline uint32_t pfb_bin_channel(int32_t first_bin, uint32_t j, uint32_t M)
{
    return (uint32_t)(((int64_t)first_bin + (int64_t)j + (int64_t)M) % (int64_t)M);
}
inline uint32_t pfb_bin_place(int32_t first_bin, uint32_t j, uint32_t M)
{
    return psd_bin_position(pfb_bin_channel(first_bin, j, M), M);
}

// LDS of one workgroup
constexpr size_t pfb_lds_bytes(uint32_t M) { return stream_bank_lds_bytes(M); }
constexpr int PFB_LDS_PER_CU = STREAM_LDS_PER_CU;

// workgroups a CU holds at a time
constexpr int pfb_groups_per_cu(uint32_t M) { return stream_groups_per_cu(pfb_lds_bytes(M)); }

} // namespace if_fir
