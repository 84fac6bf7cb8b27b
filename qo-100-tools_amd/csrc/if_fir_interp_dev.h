// if_fir_interp_dev.h — device code the interpolator (if_fir_interp.hip) and the channel combiner (if_fir_combiner.hip) share:
// the sample loads, the radix-2 / radix-4 butterflies and the Stockham pass over an LDS block of up to 4096 points.  (The NCO
// phasor nco_phasor() is in if_fir_kernels.h.)  Index algebra of the passes: tools/fft_model.py (stockham, interp_block).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "if_fir_interp.h"

// LDS reads as single ds_read_b64, as in the decimator's overlap-save units (if_fir_fft_dev.h, IF_FIR_LDS_SINGLE_READS): the
// machine-level pairing is switched off per kernel here, the IR-level vectorizer for the whole unit (csrc/Makefile, NOPAIR)
#if defined(__HIP_DEVICE_COMPILE__)
#define IF_FIR_INTERP_SINGLE_READS __attribute__((target("no-load-store-opt")))
#else
#define IF_FIR_INTERP_SINGLE_READS
#endif

namespace if_fir
{

constexpr int INTERP_THREADS = 256;

__device__ __forceinline__ float2 ip_cmul(float2 a, float2 b)
{
    return make_float2(fmaf(a.x, b.x, -a.y * b.y), fmaf(a.x, b.y, a.y * b.x));
}

__device__ __forceinline__ float2 ip_cvt_i16(int w)
{
    return make_float2((float)(short)(w & 0xffff) * (1.0f / 32768.0f), (float)(w >> 16) * (1.0f / 32768.0f));
}

// input sample j of this call (float32): j < 0 from the history (hist[hist_len + j]), j >= N reads 0
template <bool I16>
__device__ __forceinline__ float2 ip_load(const void *__restrict__ in, const float2 *__restrict__ hist, int hist_len, int64_t N,
                                          int64_t j)
{
    if (j < 0)
        return (j + hist_len >= 0) ? hist[j + hist_len] : make_float2(0.f, 0.f);
    if (j >= N)
        return make_float2(0.f, 0.f);
    if constexpr (I16)
        return ip_cvt_i16(static_cast<const int *>(in)[j]);
    else
        return static_cast<const float2 *>(in)[j];
}

// radix-R butterfly; forward = exp(-j ...), INV = exp(+j ...)
template <int R, bool INV>
__device__ __forceinline__ void ip_bfly(float2 (&v)[R])
{
    if constexpr (R == 2)
    {
        const float2 a = v[0], b = v[1];
        v[0] = make_float2(a.x + b.x, a.y + b.y);
        v[1] = make_float2(a.x - b.x, a.y - b.y);
    }
    else
    {
        const float2 t0 = make_float2(v[0].x + v[2].x, v[0].y + v[2].y), t1 = make_float2(v[0].x - v[2].x, v[0].y - v[2].y);
        const float2 t2 = make_float2(v[1].x + v[3].x, v[1].y + v[3].y), t3 = make_float2(v[1].x - v[3].x, v[1].y - v[3].y);
        // -j t3 (forward) / +j t3 (inverse)
        const float2 m = INV ? make_float2(-t3.y, t3.x) : make_float2(t3.y, -t3.x);
        v[0] = make_float2(t0.x + t2.x, t0.y + t2.y);
        v[2] = make_float2(t0.x - t2.x, t0.y - t2.y);
        v[1] = make_float2(t1.x + m.x, t1.y + m.y);
        v[3] = make_float2(t1.x - m.x, t1.y - m.y);
    }
}

// One Stockham pass over nf points (tools/fft_model.py, stockham): j = 0 .. nf/R - 1, k = j mod ns,
//   v[r] = src(j + r nf/R) W_{ns R}^(r k),  V = DFT_R(v),  dst((j - k) R + k + r ns, V[r]).
// Every input is read before the workgroup barrier, every output written after it: src and dst may be the same LDS buffer.
template <int R, bool INV, class Src, class Dst>
__device__ __forceinline__ void ip_pass(int nf, int ns, const float2 *__restrict__ tw, Src src, Dst dst)
{
    constexpr int Q = INTERP_N / 4 / INTERP_THREADS; // j per thread at most (nf / R <= 1024)
    const int nr = nf / R;
    float2 v[Q][R];
#pragma unroll
    for (int q = 0; q < Q; q++)
    {
        const int j = (int)threadIdx.x + q * INTERP_THREADS;
        if (j < nr)
#pragma unroll
            for (int r = 0; r < R; r++)
                v[q][r] = src(j + r * nr);
    }
    __syncthreads();
    const int tstep = INTERP_N / (ns * R);
#pragma unroll
    for (int q = 0; q < Q; q++)
    {
        const int j = (int)threadIdx.x + q * INTERP_THREADS;
        if (j < nr)
        {
            const int k = j & (ns - 1);
            if (ns > 1)
#pragma unroll
                for (int r = 1; r < R; r++)
                {
                    float2 w = tw[(unsigned)(r * k * tstep)];
                    if (INV)
                        w.y = -w.y;
                    v[q][r] = ip_cmul(v[q][r], w);
                }
            ip_bfly<R, INV>(v[q]);
            const int base = (j - k) * R + k;
#pragma unroll
            for (int r = 0; r < R; r++)
                dst(base + r * ns, v[q][r]);
        }
    }
    __syncthreads();
}

} // namespace if_fir
