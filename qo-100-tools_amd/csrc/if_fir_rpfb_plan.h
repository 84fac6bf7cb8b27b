// if_fir_rpfb_plan.h — host-side planning of the real-input polyphase filter bank (docs/SPEC.md §17): which
// frames a call emits from its stream position, how the frames are dealt to workgroups, the tap table in the order the kernel
// reads it, where the half-size transform leaves a bin and its partner, and the untangling twiddles.  No HIP types: the shim, the
// kernel unit and tests/c/rpfb_plan_check.cpp (plain g++) all include this file, so what the checker walks is what the launcher
// uses.
//
//   y_k[m] = sum_{t<T} h[t] r[a-t] e^{-j 2 pi k (a-t) / M},   a = m D,   k = 0 .. M/2
//
// Fold form: slot s of an M-point REAL buffer holds u[s] = sum of h[t] r[a-t] over the t < T with (a - t) mod M == s, summed as
// in if_fir_pfb_plan.h (slot (a + 1 + q) mod M, rows r = 0 .. K-1).  With H = M/2, z[n] = u[2n] + j u[2n+1] and Z = DFT_H(z):
//
//   y_k = (Z[k] + conj Z[H-k]) / 2 + W_M^k (Z[k] - conj Z[H-k]) / (2j),   Z[H] = Z[0],   W_M^k = e^{-j 2 pi k / M}
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "if_fir_pfb_plan.h" // the tap table and its rows are §13's; psd_bin_position: the shared transform's bin order

namespace if_fir
{

constexpr int RPFB_THREADS = 256;        // one workgroup
constexpr int RPFB_MIN_M = 128;          // the transform is M/2 points: 64 .. 4096
constexpr int RPFB_MAX_M = 8192;
constexpr int RPFB_MAX_ROWS = PFB_MAX_ROWS; // K = ceil(T / M)
constexpr uint64_t RPFB_MAX_CALL = (uint64_t)1 << 40; // samples of one call

inline bool rpfb_size_ok(uint32_t M) { return M % 2 == 0 && stream_size_ok(M / 2, RPFB_MIN_M / 2); }

// rows of the tap table: K = ceil(T / M)
inline uint32_t rpfb_rows(uint32_t T, uint32_t M) { return pfb_rows(T, M); }

// frames a workgroup folds and transforms together: at least STREAM_BANK_POINTS points of the M/2-point transform
constexpr uint32_t rpfb_batch(uint32_t M) { return stream_bank_batch(M / 2); }

// consecutive frames one workgroup owns: whole batches, at least 8 frames (consecutive frames read overlapping inputs)
constexpr uint32_t rpfb_group_frames(uint32_t M)
{
    return 2 * rpfb_batch(M) > 8u ? 2 * rpfb_batch(M) : 8u;
}

// the output span: channels first_bin .. first_bin + bins - 1 of 0 .. M/2, no wrap
inline bool rpfb_span_ok(uint32_t first_bin, uint32_t bins, uint32_t M)
{
    return bins >= 1 && (uint64_t)first_bin + bins <= (uint64_t)M / 2 + 1;
}

struct RpfbCall
{
    uint64_t frames; // frames the call emits
    uint64_t groups; // runs of rpfb_group_frames frames (the last may be short)
    uint32_t n0;     // offset in the call's input of the sample under its first frame, 0 <= n0 < D (meaningful when frames > 0)
    uint32_t cmod;   // c mod M: all the kernel learns of the stream position
    uint32_t carry;  // samples kept for the next call: T - 1
};

// a call with n inputs at stream position c: the frames m with m D in [c, c + n).  Nothing overflows short of c + n itself
// (refused)
inline bool rpfb_call(uint64_t c, uint64_t n, uint32_t M, uint32_t D, uint32_t T, RpfbCall *out)
{
    if (D == 0 || M == 0 || T == 0 || !stream_decim_call(c, n, D, &out->n0, &out->frames))
        return false;
    const uint64_t gf = rpfb_group_frames(M);
    out->groups = out->frames / gf + (out->frames % gf ? 1 : 0);
    out->cmod = (uint32_t)(c % M);
    out->carry = T - 1;
    return true;
}

// the table the kernel reads front to back: §13's (entry r M + q = h[r M + (M-1-q)], zero where the index reaches T)
inline void rpfb_build_taps(const float *h, uint32_t T, uint32_t M, float *out) { pfb_build_taps(h, T, M, out); }

// where the M/2-point transform leaves Z[k] and its partner Z[M/2 - k], for channel k = 0 .. M/2 (Z[M/2] = Z[0])
inline uint32_t rpfb_bin_place(uint32_t k, uint32_t M)
{
    return psd_bin_position(k % (M / 2), M / 2);
}
inline uint32_t rpfb_partner_place(uint32_t k, uint32_t M)
{
    return psd_bin_position((M / 2 - k % (M / 2)) % (M / 2), M / 2);
}
// the kernel's table, entry k < M/2: the place of Z[k] in the low 16 bits, of its partner in the high 16 (channel M/2 reads
// entry 0: the kernel takes channels 0 and M/2 from Z[0] alone).  out holds M/2 words
inline void rpfb_build_places(uint32_t M, uint32_t *out)
{
    for (uint32_t k = 0; k < M / 2; k++)
        out[k] = rpfb_bin_place(k, M) | rpfb_partner_place(k, M) << 16;
}

// the untangling twiddles W_M^k = e^{-j 2 pi k / M}, k = 0 .. M/2, as (re, im) pairs: float64 cos and sin, rounded once.
// out holds M/2 + 1 pairs
inline void rpfb_build_twiddles(uint32_t M, float *out)
{
    for (uint32_t k = 0; k <= M / 2; k++)
    {
        const double ang = -6.283185307179586476925286766559 * (double)k / (double)M;
        out[2 * k] = (float)cos(ang);
        out[2 * k + 1] = (float)sin(ang);
    }
}

// LDS of one workgroup: the batch's transform points and the transform's twiddles (float2 each), the table of places (a word
// per k < M/2).  The untangling twiddles stay in the L2-resident table
constexpr size_t rpfb_lds_bytes(uint32_t M)
{
    return (size_t)rpfb_batch(M) * (M / 2) * 8 + (size_t)(M / 2) * 8 + (size_t)(M / 2) * 4;
}
constexpr int RPFB_LDS_PER_CU = STREAM_LDS_PER_CU;

// workgroups a CU holds at a time
constexpr int rpfb_groups_per_cu(uint32_t M) { return stream_groups_per_cu(rpfb_lds_bytes(M)); }

} // namespace if_fir
