// if_fir_pfb.hip — polyphase filter bank (weighted overlap-add analysis bank): all M channels of a stream in one pass, for gfx950
// (docs/SPEC.md §13).
//
//   y_k[m] = sum_{t<T} h[t] x[a-t] e^{-j 2 pi k (a-t) / M},   a = m D (absolute index)
//
// pfb_kernel<M, I16>: a WORKGROUP owns runs of pfb_group_frames(M) consecutive frames and takes them B = pfb_batch(M) at a time
// (B M >= 1024 points, so every lane has a butterfly in every pass: 16 frames at once for M = 64, one for M >= 1024).  Per batch:
// lane item (frame, q) sums h[t] x[a-t] over t = M-1-q + r M, r = 0 .. K-1 in that order (coalesced global loads along q, int16
// converted on the way, samples before the call from the carried history; the time-reversed taps from the L2-resident table)
// and stores the sum in LDS slot (a + 1 + q) mod M of its frame: the fold by absolute index.  Then the in-place transform of
// if_fir_lds_fft_dev.h over all B blocks at once (twiddles from a float64-built table staged in LDS once per workgroup), and
// the selected bins leave as float2, coalesced along the bin index.
// pfb_carry_kernel: the last T - 1 samples of (history || call) go to the other ping-pong buffer as float32.
// A frame's arithmetic depends on its own T inputs, the taps and a mod M only -- not on the call, the batch or the workgroup it
// falls into -- so a stream cut anywhere gives the same bits.  The kernel sees call-relative positions and c mod M, never c.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <mutex>

#include "if_fir_kernels.h"
#include "if_fir_lds_fft_dev.h"
#include "if_fir_pfb.h"
#include "if_fir_stream_dev.h"

namespace if_fir
{

template <int M, bool I16>
__global__ __launch_bounds__(PFB_THREADS) IF_FIR_SINGLE_READS void pfb_kernel(
    const void *__restrict__ in, const float2 *__restrict__ hist, const float *__restrict__ taps, const float2 *__restrict__ twiddle,
    const uint16_t *__restrict__ bin_pos, float2 *__restrict__ out, int T, int K, int D, int bins, int hist_len, uint32_t n0,
    uint32_t cmod, int64_t frames, int64_t groups, int64_t n)
{
    constexpr int B = (int)pfb_batch(M), TOTAL = B * M, R = TOTAL / PFB_THREADS, GF = (int)pfb_group_frames(M);
    extern __shared__ __attribute__((aligned(16))) char smem[];
    stream_v2f *x = reinterpret_cast<stream_v2f *>(smem);
    stream_v2f *tw = x + TOTAL;
    uint16_t *where = reinterpret_cast<uint16_t *>(tw + M);
    const int tid = threadIdx.x;
    for (int e = tid; e < M; e += PFB_THREADS)
    {
        const float2 t = twiddle[e];
        tw[e] = stream_v2f{t.x, t.y};
        where[e] = e < bins ? bin_pos[e] : (uint16_t)0;
    }

    for (int64_t g = blockIdx.x; g < groups; g += gridDim.x)
    {
        const int64_t f_first = g * GF, f_end = frames - f_first < GF ? frames : f_first + GF;
        for (int64_t f0 = f_first; f0 < f_end; f0 += B)
        {
            stream_v2f acc[R];
            int64_t a_rel[R]; // the frame's newest sample, counted from the call's first
            bool live[R];
#pragma unroll
            for (int i = 0; i < R; i++)
            {
                const int e = tid + i * PFB_THREADS;
                const int64_t f = f0 + (B == 1 ? 0 : e / M);
                acc[i] = stream_v2f{0.f, 0.f};
                live[i] = f < f_end;
                a_rel[i] = (int64_t)n0 + f * D;
            }
            for (int r = 0; r < K; r++)
            {
#pragma unroll
                for (int i = 0; i < R; i++)
                {
                    const int q = (tid + i * PFB_THREADS) % M;
                    const int t = M - 1 - q + r * M;
                    if (live[i] && t < T)
                    {
                        const float h = taps[r * M + q];
                        const stream_v2f v = stream_load<I16>(in, hist, hist_len, n, a_rel[i] - t);
                        acc[i].x = fmaf(h, v.x, acc[i].x);
                        acc[i].y = fmaf(h, v.y, acc[i].y);
                    }
                }
            }
            __syncthreads(); // the previous batch has been stored (and, the first time, the twiddles are staged)
#pragma unroll
            for (int i = 0; i < R; i++)
            {
                const int e = tid + i * PFB_THREADS;
                const int q = e % M;
                const uint32_t s = (uint32_t)((uint64_t)a_rel[i] + cmod + 1u + (uint32_t)q) & (uint32_t)(M - 1);
                x[(e / M) * M + (int)s] = acc[i];
            }
            __syncthreads();
            lds_fft_passes<TOTAL, M, M, PFB_THREADS>(x, tw, tid);
            const int nb = f_end - f0 < B ? (int)(f_end - f0) : B;
            float2 *dst = out + (size_t)f0 * (size_t)bins;
            for (int e = tid; e < nb * bins; e += PFB_THREADS)
            {
                const int fb = B == 1 ? 0 : e / bins;
                const stream_v2f v = x[fb * M + where[e - fb * bins]];
                dst[e] = make_float2(v.x, v.y);
            }
        }
    }
}

template <bool I16>
__global__ __launch_bounds__(PFB_THREADS) void pfb_carry_kernel(const void *__restrict__ in, const float2 *__restrict__ hist,
                                                                float2 *__restrict__ hist_out, int64_t hist_len, int64_t n)
{
    // the last hist_len samples of (hist || call) (its own loop: through a shared helper it compiles to other code, profiles/stream_plan_ab.txt)
    for (int64_t i = (int64_t)blockIdx.x * PFB_THREADS + threadIdx.x; i < hist_len; i += (int64_t)gridDim.x * PFB_THREADS)
    {
        const stream_v2f v = stream_load<I16>(in, hist, hist_len, n, n - hist_len + i);
        hist_out[i] = make_float2(v.x, v.y);
    }
}

template <int M, bool I16>
static hipError_t launch_frames(const PfbArgs &a)
{
    int cus = 0;
    constexpr int lds = (int)pfb_lds_bytes(M);
    const hipError_t e = stream_kernel_setup<&pfb_kernel<M, I16>>(a.device, lds, &cus);
    if (e != hipSuccess)
        return e;
    const unsigned groups = stream_persistent_groups(cus, pfb_groups_per_cu(M), (int64_t)a.call.groups, a.grid_limit);
    hipLaunchKernelGGL((pfb_kernel<M, I16>), dim3(groups), dim3(PFB_THREADS), lds, a.stream, a.in, a.hist, a.taps, a.twiddle, a.bin_pos,
                       a.out, a.T, a.K, a.D, a.bins, a.hist_len, a.call.n0, a.call.cmod, (int64_t)a.call.frames, (int64_t)a.call.groups, a.n);
    return hipGetLastError();
}

template <bool I16>
static hipError_t launch_t(const PfbArgs &a)
{
    if (a.call.frames > 0)
    {
        hipError_t e;
        switch (a.M)
        {
        case 64: e = launch_frames<64, I16>(a); break;
        case 128: e = launch_frames<128, I16>(a); break;
        case 256: e = launch_frames<256, I16>(a); break;
        case 512: e = launch_frames<512, I16>(a); break;
        case 1024: e = launch_frames<1024, I16>(a); break;
        case 2048: e = launch_frames<2048, I16>(a); break;
        case 4096: e = launch_frames<4096, I16>(a); break;
        default: e = hipErrorInvalidValue;
        }
        if (e != hipSuccess)
            return e;
    }
    if (a.hist_len > 0)
    {
        const unsigned groups = stream_generic_groups(a.hist_len, PFB_THREADS, 0);
        hipLaunchKernelGGL((pfb_carry_kernel<I16>), dim3(groups), dim3(PFB_THREADS), 0, a.stream, a.in, a.hist, a.hist_out,
                           (int64_t)a.hist_len, a.n);
        return hipGetLastError();
    }
    return hipSuccess;
}

hipError_t launch_pfb(const PfbArgs &a)
{
    const uint64_t gf = a.M > 0 ? pfb_group_frames((uint32_t)a.M) : 1;
    if (!pfb_size_ok((uint32_t)a.M) || a.T < 1 || a.T > PFB_MAX_ROWS * a.M || a.K != (int)pfb_rows((uint32_t)a.T, (uint32_t)a.M) || a.D < 1 ||
        a.D > a.M || a.bins < 1 || a.bins > a.M || a.hist_len != a.T - 1 || a.n < 1 || (uint64_t)a.n > PFB_MAX_CALL ||
        a.call.n0 >= (uint32_t)a.D || a.call.cmod >= (uint32_t)a.M ||
        a.call.frames != ((uint64_t)a.n > a.call.n0 ? ((uint64_t)a.n - a.call.n0 - 1) / (uint64_t)a.D + 1 : 0) ||
        a.call.groups != (a.call.frames + gf - 1) / gf)
        return hipErrorInvalidValue;
    return a.in_i16 ? launch_t<true>(a) : launch_t<false>(a);
}

} // namespace if_fir
