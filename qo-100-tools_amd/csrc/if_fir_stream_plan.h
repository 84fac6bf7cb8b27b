// if_fir_stream_plan.h — what the plan headers if_fir_X_plan.h of the streaming families (STREAM_FAMILIES in the Makefile) share:
// the plan-layer counterpart of if_fir_stream_ctx.h and if_fir_stream_dev.h, under the same rule -- nothing here branches on
// which family includes it.  No HIP types: the shims, the kernel units and the plan checkers under tests/c (plain g++; this
// header's own is tests/c/stream_plan_check.cpp) all include it through the plan headers.  IF_FIR_STREAM_HD marks the
// functions a kernel calls too.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define IF_FIR_STREAM_HD __host__ __device__
#else
#define IF_FIR_STREAM_HD
#endif

namespace if_fir
{

constexpr int STREAM_LDS_PER_CU = 160 * 1024; // gfx950

// workgroups of lds_bytes (> 0) of LDS each a CU holds at a time: what its LDS fits, at most 8 (32 waves), at least 1
constexpr int stream_groups_per_cu(size_t lds_bytes)
{
    const size_t fit = (size_t)STREAM_LDS_PER_CU / lds_bytes;
    return fit > 8 ? 8 : fit < 1 ? 1 : (int)fit;
}

// a decimating call with n inputs at stream position c: the outputs at absolute index a in [c, c + n) with a mod D == 0 (D > 0).
// *n0 = the offset in the call's input of the sample under the first of them, 0 <= n0 < D; *count = how many.  Nothing
// overflows short of c + n itself (refused, nothing written)
inline bool stream_decim_call(uint64_t c, uint64_t n, uint64_t D, uint32_t *n0, uint64_t *count)
{
    if (c + n < c)
        return false;
    *n0 = (uint32_t)((D - c % D) % D);
    *count = n > *n0 ? (n - *n0 - 1) / D + 1 : 0;
    return true;
}

// the NCO-shifted taps g[k] = h[k] e^{+j theta k}, theta = 2 pi P / 2^32, in float64 (the phase (P k) mod 2^32 is an exact
// integer), rounded once; P = 0: g = h.  taps: T floats, or T (re, im) pairs with ctaps; out holds T (re, im) pairs
inline void stream_mix_taps(const float *taps, int T, int ctaps, uint32_t word, float *out)
{
    for (int k = 0; k < T; k++)
    {
        const double hr = ctaps ? (double)taps[2 * k] : (double)taps[k], hi = ctaps ? (double)taps[2 * k + 1] : 0.0;
        const double a = 6.283185307179586476925286766559 * ((double)(uint32_t)(word * (uint32_t)k) / 4294967296.0);
        out[2 * k] = word ? (float)(hr * cos(a) - hi * sin(a)) : (float)hr;
        out[2 * k + 1] = word ? (float)(hr * sin(a) + hi * cos(a)) : (float)hi;
    }
}

// SPEC §7's accumulation order: K taps in descending j, in segments of STREAM_SEG from +0 of which the HIGHEST (the first one
// summed) takes what 16 does not divide: 1..16 taps
constexpr int STREAM_SEG = 16;
IF_FIR_STREAM_HD inline int stream_top_segment(int K)
{
    return K - ((K - 1) / STREAM_SEG) * STREAM_SEG;
}

// a transform size of if_fir_lds_fft_dev.h: a power of two in [min_size, 4096]
inline bool stream_size_ok(uint32_t size, uint32_t min_size)
{
    return size >= min_size && size <= 4096 && (size & (size - 1)) == 0;
}

// The two polyphase banks' transform in LDS.  Frames of M points a workgroup of 256 transforms together: at least
// STREAM_BANK_POINTS points, so that every lane has a butterfly in every pass (1024 / M frames when M < 1024)
constexpr int STREAM_BANK_POINTS = 1024;
constexpr uint32_t stream_bank_batch(uint32_t M)
{
    return M >= (uint32_t)STREAM_BANK_POINTS ? 1u : (uint32_t)STREAM_BANK_POINTS / M;
}
// LDS of such a workgroup: the batch's points, the twiddles (float2 each) and the bin places (uint16)
constexpr size_t stream_bank_lds_bytes(uint32_t M)
{
    return (size_t)stream_bank_batch(M) * M * 8 + (size_t)M * 8 + (size_t)M * 2;
}

} // namespace if_fir
