// if_fir_lds_fft_dev.h — the in-place LDS transform the power-spectrum estimator (if_fir_psd.hip), the polyphase filter bank
// (if_fir_pfb.hip), the polyphase synthesis bank (if_fir_synth.hip) and the real-input bank (if_fir_rpfb.hip, at M/2 points) share, under the rule of if_fir_stream_dev.h: nothing here branches on which family includes it.
//
// TOTAL complex points in LDS hold TOTAL / N independent blocks of N points each, block b at [b N, b N + N).  Every block gets the
// same forward decimation-in-frequency transform: radix-4 passes that meet at workgroup barriers and, when N is an odd power of
// two, one last radix-2 pass.  Bin k of a block ends at psd_bin_position(k, N) of that block (if_fir_psd_plan.h).  The twiddle
// table tw holds exp(-2 pi i t / N), t < N.  A block's arithmetic is the same instructions in the same order whichever block of
// the buffer it is and whichever thread runs a butterfly.
#pragma once
#include <hip/hip_runtime.h>

#include "if_fir_stream_dev.h"

namespace if_fir
{

__device__ __forceinline__ stream_v2f lds_fft_cmul(const stream_v2f a, const stream_v2f w)
{
    return stream_v2f{fmaf(a.x, w.x, -a.y * w.y), fmaf(a.x, w.y, a.y * w.x)};
}

// one in-place radix-4 decimation-in-frequency pass over sub-blocks of LEN: butterfly j of a sub-block reads and writes the
// same four places j, j + LEN/4, j + LEN/2, j + 3 LEN/4, so passes only need a barrier between them
template <int TOTAL, int N, int LEN, int THREADS>
__device__ __forceinline__ void lds_fft_pass4(stream_v2f *__restrict__ x, const stream_v2f *__restrict__ tw, int tid)
{
    constexpr int Q = LEN / 4, STEP = N / LEN;
    for (int b = tid; b < TOTAL / 4; b += THREADS)
    {
        const int j = b % Q, base = (b / Q) * LEN + j;
        const stream_v2f a0 = x[base], a1 = x[base + Q], a2 = x[base + 2 * Q], a3 = x[base + 3 * Q];
        const stream_v2f t0 = a0 + a2, t1 = a0 - a2, t2 = a1 + a3, d = a1 - a3;
        const stream_v2f t3 = {d.y, -d.x}; // -i (a1 - a3)
        stream_v2f y0 = t0 + t2, y1 = t1 + t3, y2 = t0 - t2, y3 = t1 - t3;
        if constexpr (Q > 1)
        {
            y1 = lds_fft_cmul(y1, tw[j * STEP]);
            y2 = lds_fft_cmul(y2, tw[2 * j * STEP]);
            y3 = lds_fft_cmul(y3, tw[3 * j * STEP]);
        }
        x[base] = y0;
        x[base + Q] = y1;
        x[base + 2 * Q] = y2;
        x[base + 3 * Q] = y3;
    }
}

// all passes, from sub-blocks of LEN (call with LEN = N) down; a barrier after each, the last one included
template <int TOTAL, int N, int LEN, int THREADS>
__device__ __forceinline__ void lds_fft_passes(stream_v2f *__restrict__ x, const stream_v2f *__restrict__ tw, int tid)
{
    if constexpr (LEN >= 4)
    {
        lds_fft_pass4<TOTAL, N, LEN, THREADS>(x, tw, tid);
        __syncthreads();
        lds_fft_passes<TOTAL, N, LEN / 4, THREADS>(x, tw, tid);
    }
    else if constexpr (LEN == 2)
    {
        for (int b = tid; b < TOTAL / 2; b += THREADS)
        {
            const stream_v2f a0 = x[2 * b], a1 = x[2 * b + 1];
            x[2 * b] = a0 + a1;
            x[2 * b + 1] = a0 - a1;
        }
        __syncthreads();
    }
}

} // namespace if_fir
