// if_fir_psd.hip — streaming averaged periodogram (Welch) with the WB detector's dB-to-code scale, for gfx950 (docs/SPEC.md §8,
// DESIGN.md §3.13).
//
//   S_s[k] = | sum_n w[n] x[s H + n] e^{-2 pi i k n / N} |^2,     P[k] = (sum_{s in frame} S_s[k]) / (K sum_n w[n]^2)
//
// psd_chunk_kernel<N, I16>: a WORKGROUP owns whole chunks of up to 8 consecutive segments of one frame (if_fir_psd_plan.h).  Per
// segment: coalesced global loads (int16 converted on the way, samples before the call from the carried buffer), the window from
// registers, the in-place decimation-in-frequency transform of if_fir_lds_fft_dev.h in LDS (radix-4 passes that meet at workgroup barriers, one last radix-2
// pass for N = 512 and 2048; twiddles from a float64-built table staged in LDS once per workgroup), then fma(re, re, im im) of the
// selected bins only, added in segment order onto per-lane registers.  One float32 chunk sum per selected bin goes to the work buffer.
// psd_frame_kernel: one thread per (frame, bin) adds the chunk sums in chunk order onto the carried accumulator; a completed frame
// is scaled once and mapped to its code in float64, an open one stores its accumulator for the next call.
// psd_carry_kernel: the samples of the open chunk go to the other ping-pong buffer as float32.
// Every sum is made by the same instructions in the same order whatever the call, so a stream cut anywhere gives the same bits.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <mutex>

#include "if_fir_kernels.h"
#include "if_fir_lds_fft_dev.h"
#include "if_fir_psd.h"
#include "if_fir_stream_dev.h"

namespace if_fir
{

template <int N, bool I16>
__global__ __launch_bounds__(PSD_THREADS) void psd_chunk_kernel(const void *__restrict__ in, const float2 *__restrict__ carry,
                                                                const float *__restrict__ window, const float2 *__restrict__ twiddle,
                                                                const uint16_t *__restrict__ bin_pos, float *__restrict__ work, int H,
                                                                int K, int bins, uint32_t chunk0, uint32_t chunks, int64_t n,
                                                                int64_t carried)
{
    constexpr int R = N / PSD_THREADS; // samples, and at most bins, per lane
    extern __shared__ __attribute__((aligned(16))) char smem[];
    stream_v2f *x = reinterpret_cast<stream_v2f *>(smem);
    stream_v2f *tw = x + N;
    const int tid = threadIdx.x;
    float w[R];
    int where[R];
#pragma unroll
    for (int i = 0; i < R; i++)
    {
        const int e = tid + i * PSD_THREADS;
        const float2 t = twiddle[e];
        tw[e] = stream_v2f{t.x, t.y};
        w[i] = window[e];
        where[i] = e < bins ? (int)bin_pos[e] : 0;
    }

    for (uint32_t c = blockIdx.x; c < chunks; c += gridDim.x)
    {
        uint32_t seg_rel, count, frame_rel;
        psd_chunk_entry(chunk0, c, (uint32_t)K, &seg_rel, &count, &frame_rel);
        float sum[R];
#pragma unroll
        for (int i = 0; i < R; i++)
            sum[i] = 0.f;
        for (uint32_t s = 0; s < count; s++)
        {
            const int64_t first = ((int64_t)seg_rel + s) * H - carried;
            __syncthreads(); // the previous segment has been read (and, the first time, the twiddles are staged)
#pragma unroll
            for (int i = 0; i < R; i++)
            {
                const int e = tid + i * PSD_THREADS;
                x[e] = stream_load<I16>(in, carry, carried, n, first + e) * w[i];
            }
            __syncthreads();
            lds_fft_passes<N, N, N, PSD_THREADS>(x, tw, tid);
#pragma unroll
            for (int i = 0; i < R; i++)
            {
                const stream_v2f v = x[where[i]];
                sum[i] += fmaf(v.x, v.x, v.y * v.y);
            }
        }
        float *dst = work + (size_t)c * bins;
#pragma unroll
        for (int i = 0; i < R; i++)
        {
            const int e = tid + i * PSD_THREADS;
            if (e < bins)
                dst[e] = sum[i];
        }
    }
}

// thread (frame t of the call, bin b): the frame's chunks of this call in chunk order onto the accumulator
__global__ __launch_bounds__(PSD_THREADS) void psd_frame_kernel(const float *__restrict__ work, const float *__restrict__ acc,
                                                                float *__restrict__ acc_out, uint16_t *__restrict__ codes,
                                                                float *__restrict__ power, int bins, uint32_t cpf, uint32_t chunk0,
                                                                uint32_t chunks, uint32_t touched, float scale, double ref_power)
{
    const uint64_t idx = (uint64_t)blockIdx.x * PSD_THREADS + threadIdx.x;
    if (idx >= (uint64_t)touched * bins)
        return;
    const uint32_t t = (uint32_t)(idx / bins), b = (uint32_t)(idx % bins);
    // chunks of the call that belong to frame t: call-relative [lo, hi)
    const uint64_t fbeg = (uint64_t)t * cpf, fend = fbeg + cpf;
    const uint64_t lo = fbeg > chunk0 ? fbeg - chunk0 : 0;
    const uint64_t end = fend - chunk0;
    const bool complete = end <= chunks;
    const uint64_t hi = complete ? end : chunks;
    float a = (t == 0 && chunk0 > 0) ? acc[b] : 0.f;
    for (uint64_t c = lo; c < hi; c++)
        a += work[c * bins + b];
    if (!complete)
    {
        acc_out[b] = a;
        return;
    }
    const float p = a * scale;
    if (power)
        power[(size_t)t * bins + b] = p;
    // the detector's scale (wb_detect.hip): fft_zero_scale_power = -3.35 dB, fft_full_scale_power = 16.7 dB over 65535 codes
    const double slope = (16.7 - (-3.35)) / 65535;
    const double db = 10.0 * log10((double)p / ref_power); // p = 0: -inf, code 0
    double code = rint((db - (-3.35)) / slope);
    code = code > 0.0 ? code : 0.0; // (also takes -inf, and a NaN were there one)
    code = code < 65535.0 ? code : 65535.0;
    codes[(size_t)t * bins + b] = (uint16_t)code;
}

template <bool I16>
__global__ __launch_bounds__(PSD_THREADS) void psd_carry_kernel(const void *__restrict__ in, const float2 *__restrict__ carry,
                                                                float2 *__restrict__ carry_out, int64_t carried, int64_t n,
                                                                int64_t keep)
{
    // the last `keep` samples of (carried || call)
    for (int64_t i = (int64_t)blockIdx.x * PSD_THREADS + threadIdx.x; i < keep; i += (int64_t)gridDim.x * PSD_THREADS)
    {
        const stream_v2f v = stream_load<I16>(in, carry, carried, n, n - keep + i);
        carry_out[i] = make_float2(v.x, v.y);
    }
}

template <int N, bool I16>
static hipError_t launch_chunks(const PsdArgs &a)
{
    int cus = 0;
    constexpr int lds = 2 * N * (int)sizeof(float2);
    const hipError_t e = stream_kernel_setup<&psd_chunk_kernel<N, I16>>(a.device, lds, &cus);
    if (e != hipSuccess)
        return e;
    // a grid-stride loop over the chunks; the twiddles are staged once per workgroup, 160 KiB of LDS hold 160 / (16 N / 1024) of them
    // (the caller launches only with chunks > 0: at most one workgroup per chunk; the grid limit is 0 outside the development hook)
    const unsigned groups = stream_persistent_groups(cus, N >= 4096 ? 2 : N >= 2048 ? 4 : 8, (int64_t)a.plan.chunks, a.grid_limit);
    hipLaunchKernelGGL((psd_chunk_kernel<N, I16>), dim3(groups), dim3(PSD_THREADS), lds, a.stream, a.in, a.carry, a.window,
                       a.twiddle, a.bin_pos, a.work, a.H, a.K, a.bins, a.plan.chunk0, (uint32_t)a.plan.chunks, a.n, a.carried);
    return hipGetLastError();
}

template <bool I16>
static hipError_t launch_t(const PsdArgs &a)
{
    if (a.plan.chunks > 0)
    {
        hipError_t e;
        switch (a.N)
        {
        case 256: e = launch_chunks<256, I16>(a); break;
        case 512: e = launch_chunks<512, I16>(a); break;
        case 1024: e = launch_chunks<1024, I16>(a); break;
        case 2048: e = launch_chunks<2048, I16>(a); break;
        case 4096: e = launch_chunks<4096, I16>(a); break;
        default: e = hipErrorInvalidValue;
        }
        if (e != hipSuccess)
            return e;
        const uint32_t cpf = psd_chunks_per_frame((uint32_t)a.K);
        const uint64_t touched = (a.plan.chunk0 + a.plan.chunks + cpf - 1) / cpf;
        const uint64_t threads = touched * (uint64_t)a.bins;
        hipLaunchKernelGGL(psd_frame_kernel, dim3((unsigned)((threads + PSD_THREADS - 1) / PSD_THREADS)), dim3(PSD_THREADS), 0, a.stream,
                           a.work, a.acc, a.acc_out, a.codes, a.power, a.bins, cpf, a.plan.chunk0, (uint32_t)a.plan.chunks,
                           (uint32_t)touched, a.scale, a.ref_power);
        e = hipGetLastError();
        if (e != hipSuccess)
            return e;
    }
    if (a.plan.carry > 0)
    {
        const int64_t keep = (int64_t)a.plan.carry;
        int64_t groups = (keep + PSD_THREADS - 1) / PSD_THREADS;
        hipLaunchKernelGGL((psd_carry_kernel<I16>), dim3((unsigned)groups), dim3(PSD_THREADS), 0, a.stream, a.in, a.carry, a.carry_out,
                           a.carried, a.n, keep);
        return hipGetLastError();
    }
    return hipSuccess;
}

hipError_t launch_psd(const PsdArgs &a)
{
    if (!psd_size_ok((uint32_t)a.N) || a.H < 1 || a.H > a.N || a.K < 1 || a.K > (int)PSD_MAX_SEGMENTS || a.bins < 1 || a.bins > a.N ||
        a.n < 0 || a.carried < 0 || a.plan.chunks >= ((uint64_t)1 << 31) || a.plan.carry > a.carried + (uint64_t)a.n ||
        a.plan.carry >= (uint64_t)(PSD_CHUNK - 1) * a.H + a.N)
        return hipErrorInvalidValue;
    return a.in_i16 ? launch_t<true>(a) : launch_t<false>(a);
}

} // namespace if_fir
