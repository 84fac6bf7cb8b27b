// if_fir_interp_dev.h — what the interpolator (if_fir_interp.hip) and the channel combiner (if_fir_combiner.hip) share: the
// sample load, the history writer, the generic kernels' tap sum of one channel, the radix-2 / radix-4 butterflies, the Stockham
// pass over an LDS block of up to 4096 points with the pass sequences of a block, and the grid of an overlap-save launch.  (What
// every streaming family shares is in if_fir_stream_dev.h, the NCO phasor nco_phasor() in if_fir_kernels.h.)  Index algebra of
// the passes: tools/fft_model.py (stockham, interp_block).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "if_fir_interp.h"
#include "if_fir_kernels.h"
#include "if_fir_stream_dev.h"

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
// (not stream_load of if_fir_stream_dev.h: the two forms, early returns here and one assignment there, compile to different code
// in every kernel that uses them, and neither change has been timed -- DESIGN.md §3.11, Device side)
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

// one channel's next history = the last hist_len samples of (history || input), converted to float32
template <bool I16>
__device__ __forceinline__ void ip_history(const void *__restrict__ in, const float2 *__restrict__ hist, float2 *__restrict__ hist_out,
                                           int hist_len, int64_t N)
{
    for (int i = threadIdx.x; i < hist_len; i += blockDim.x)
        hist_out[i] = ip_load<I16>(in, hist, hist_len, N, N - hist_len + i);
}

// the generic kernels' sum for output i of one channel: the call's output i has phase i mod L (every call starts on a multiple of
// L), tap k meets input (i - k) / L.  Partial sums of 32 taps added into the total with a compensated (two-sum) addition: one
// running float32 sum over 3000 taps drifts past the SPEC tolerance.
template <bool I16, bool CT>
__device__ __forceinline__ float2 ip_phase_sum(const void *__restrict__ in, const float2 *__restrict__ hist, int hist_len,
                                               const float *__restrict__ taps, int T, int L, int64_t N, int64_t i)
{
    float ar = 0.f, ai = 0.f, cr = 0.f, ci = 0.f;
    int k = (int)(i % L);
    while (k < T)
    {
        float pr = 0.f, pi = 0.f;
        for (int c = 0; c < 32 && k < T; c++, k += L)
        {
            const float2 x = ip_load<I16>(in, hist, hist_len, N, (i - k) / L);
            if constexpr (CT)
            {
                const float hr = taps[2 * k], hi = taps[2 * k + 1];
                pr = fmaf(hr, x.x, fmaf(-hi, x.y, pr));
                pi = fmaf(hr, x.y, fmaf(hi, x.x, pi));
            }
            else
            {
                const float h = taps[k];
                pr = fmaf(h, x.x, pr);
                pi = fmaf(h, x.y, pi);
            }
        }
        two_sum_add(ar, cr, pr);
        two_sum_add(ai, ci, pi);
    }
    return make_float2(ar + cr, ai + ci);
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

// the forward transform of nf points in place: one radix-2 pass first when log2(nf) is odd, then radix-4 passes.  (The combiner
// calls it; fir_interp_kernel has the same lines written out, because through this function its small form compiled to slower
// code: DESIGN.md §3.11, Device side.)
template <class Src, class Dst>
__device__ __forceinline__ void ip_forward(int nf, const float2 *__restrict__ tw, Src src, Dst dst)
{
    int ns = 1;
    if (nf & 0x2aaa)
    {
        ip_pass<2, false>(nf, ns, tw, src, dst);
        ns = 2;
    }
#pragma unroll 1
    for (; ns < nf; ns *= 4)
        ip_pass<4, false>(nf, ns, tw, src, dst);
}

// the 4096-point inverse's middle passes, ns = 4 .. 256 (the first one takes the product with H, the last one stores the outputs)
template <class Src, class Dst>
__device__ __forceinline__ void ip_inverse_mid(const float2 *__restrict__ tw, Src src, Dst dst)
{
#pragma unroll 1
    for (int ns = 4; ns < INTERP_N / 4; ns *= 4)
        ip_pass<4, true>(INTERP_N, ns, tw, src, dst);
}

// an overlap-save launch over M outputs in blocks that keep A of them: persistent workgroups, two per CU (up to 256 VGPRs per
// lane: two waves per SIMD); at least one, which writes the history.  (The kernels use static LDS: nothing to set per kernel.)
inline hipError_t ip_fft_grid(int device, int64_t M, int A, int grid_limit, int64_t *nblocks, unsigned *groups)
{
    static DeviceSetup setup;
    int cus = 0;
    const hipError_t e = device_setup(setup, device, nullptr, 0, &cus);
    if (e != hipSuccess)
        return e;
    *nblocks = (M + A - 1) / A;
    *groups = stream_persistent_groups(cus, 2, *nblocks, grid_limit);
    return hipSuccess;
}

} // namespace if_fir
