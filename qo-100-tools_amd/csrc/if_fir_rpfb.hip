// if_fir_rpfb.hip — real-input polyphase filter bank: the M/2 + 1 distinct channels of a REAL stream in one pass, for gfx950
// (docs/SPEC.md §17).
//
//   y_k[m] = sum_{t<T} h[t] r[a-t] e^{-j 2 pi k (a-t) / M},   a = m D (absolute index),   k = 0 .. M/2
//
// rpfb_kernel<M, I16>: a WORKGROUP owns runs of rpfb_group_frames(M) consecutive frames and takes them B = rpfb_batch(M) at a
// time (B M/2 >= 1024 transform points: 16 frames at once for M = 128, one for M >= 2048).  Per batch: lane item (frame, q, q+1),
// q even, sums h[t] r[a-t] over t = M-1-q + r M, r = 0 .. K-1 in that order for each of its two slots (coalesced global loads
// along q, two samples = 8 or 4 bytes a lane, int16 converted on the way, samples before the call from the carried history; the
// time-reversed taps from the L2-resident table, two a lane) and stores each sum as ONE float in slot (a + 1 + q) mod M of its
// frame's LDS block: the fold by absolute index, one component, every slot's chain the one of SPEC §13.  Read as
// float2 the block is z[n] = u[2n] + j u[2n+1] already, and the in-place transform of if_fir_lds_fft_dev.h runs over all B
// blocks of M/2 points at once.  The untangling pass then reads Z at the places of k and M/2 - k and writes channel k of the
// span as float2, coalesced along the bin index; channels 0 and M/2 come from Re Z[0] +- Im Z[0] alone.
// rpfb_carry_kernel: the last T - 1 samples of (history || call) go to the other ping-pong buffer as float32.
// Every frame is transformed on its own (two real frames never share a complex transform), so a frame's arithmetic depends on
// its own T inputs, the taps and a mod M only -- not on the call, the batch or the workgroup it falls into -- and a stream cut
// anywhere gives the same bits.  The kernel sees call-relative positions and c mod M, never c.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "if_fir_kernels.h"
#include "if_fir_lds_fft_dev.h"
#include "if_fir_rpfb.h"
#include "if_fir_stream_dev.h"

namespace if_fir
{

template <int M, bool I16>
__global__ __launch_bounds__(RPFB_THREADS) IF_FIR_SINGLE_READS void rpfb_kernel(
    const void *__restrict__ in, const float *__restrict__ hist, const float *__restrict__ taps, const float2 *__restrict__ twiddle,
    const uint32_t *__restrict__ places, const float2 *__restrict__ untangle, float2 *__restrict__ out, int T, int K, int D,
    int first_bin, int bins, int hist_len, uint32_t n0, uint32_t cmod, int64_t frames, int64_t groups, int64_t n)
{
    constexpr int H = M / 2, B = (int)rpfb_batch(M), TOTAL = B * H, R2 = B * H / RPFB_THREADS, GF = (int)rpfb_group_frames(M);
    extern __shared__ __attribute__((aligned(16))) char smem[];
    stream_v2f *x = reinterpret_cast<stream_v2f *>(smem);
    float *u = reinterpret_cast<float *>(smem); // the same points as real slots: u[2n], u[2n+1] = x[n]
    stream_v2f *tw = x + TOTAL;
    uint32_t *where = reinterpret_cast<uint32_t *>(tw + H);
    const int tid = threadIdx.x;
    for (int e = tid; e < H; e += RPFB_THREADS)
    {
        const float2 t = twiddle[e];
        tw[e] = stream_v2f{t.x, t.y};
        where[e] = places[e];
    }

    for (int64_t g = blockIdx.x; g < groups; g += gridDim.x)
    {
        const int64_t f_first = g * GF, f_end = frames - f_first < GF ? frames : f_first + GF;
        for (int64_t f0 = f_first; f0 < f_end; f0 += B)
        {
            // a lane item is the PAIR of slots (q, q + 1), q even: one 8-byte tap load and one 8- or 4-byte sample load per row
            // serve two chains (the fold is bound by load instructions, not by bytes: DESIGN.md §3.22)
            stream_v2f acc[R2];
            int64_t a_rel[R2]; // the frame's newest sample, counted from the call's first
            bool live[R2];
#pragma unroll
            for (int i = 0; i < R2; i++)
            {
                const int e = tid + i * RPFB_THREADS;
                const int64_t f = f0 + (B == 1 ? 0 : e / H);
                acc[i] = stream_v2f{0.f, 0.f};
                live[i] = f < f_end;
                a_rel[i] = (int64_t)n0 + f * D;
            }
            for (int r = 0; r < K; r++)
            {
#pragma unroll
                for (int i = 0; i < R2; i++)
                {
                    const int q = 2 * ((tid + i * RPFB_THREADS) % H);
                    const int t = M - 1 - q + r * M; // of slot q; slot q + 1 has t - 1
                    if (live[i] && t - 1 < T)
                    {
                        const float2 h = reinterpret_cast<const float2 *>(taps)[(r * M + q) / 2];
                        const stream_v2f v = stream_load_real2<I16>(in, hist, hist_len, n, a_rel[i] - t);
                        if (t < T)
                            acc[i].x = fmaf(h.x, v.x, acc[i].x);
                        acc[i].y = fmaf(h.y, v.y, acc[i].y);
                    }
                }
            }
            __syncthreads(); // the previous batch has been stored (and, the first time, the tables are staged)
#pragma unroll
            for (int i = 0; i < R2; i++)
            {
                const int e = tid + i * RPFB_THREADS;
                const int q = 2 * (e % H);
                const uint32_t s = (uint32_t)((uint64_t)a_rel[i] + cmod + 1u + (uint32_t)q) & (uint32_t)(M - 1);
                u[(e / H) * M + (int)s] = acc[i].x;
                u[(e / H) * M + (int)((s + 1u) & (uint32_t)(M - 1))] = acc[i].y;
            }
            __syncthreads();
            lds_fft_passes<TOTAL, H, H, RPFB_THREADS>(x, tw, tid);
            // untangling: E = (Z[k] + conj Z[H-k]) / 2, O = (Z[k] - conj Z[H-k]) / (2j), y = E + O W_M^k (SPEC §17's order)
            const int nb = f_end - f0 < B ? (int)(f_end - f0) : B;
            float2 *dst = out + (size_t)f0 * (size_t)bins;
            for (int e = tid; e < nb * bins; e += RPFB_THREADS)
            {
                const int fb = B == 1 ? 0 : e / bins;
                const int k = first_bin + (e - fb * bins);
                const stream_v2f *z = x + fb * H;
                if (k == 0 || k == H)
                {
                    const stream_v2f z0 = z[0];
                    dst[e] = make_float2(k == 0 ? z0.x + z0.y : z0.x - z0.y, 0.f);
                }
                else
                {
                    const uint32_t w = where[k];
                    const stream_v2f a = z[w & 0xffffu], b = z[w >> 16];
                    const float2 wk = untangle[k];
                    const stream_v2f ev = {0.5f * (a.x + b.x), 0.5f * (a.y - b.y)};
                    const stream_v2f od = {0.5f * (a.y + b.y), -0.5f * (a.x - b.x)};
                    const stream_v2f p = lds_fft_cmul(od, stream_v2f{wk.x, wk.y});
                    dst[e] = make_float2(ev.x + p.x, ev.y + p.y);
                }
            }
        }
    }
}

template <bool I16>
__global__ __launch_bounds__(RPFB_THREADS) void rpfb_carry_kernel(const void *__restrict__ in, const float *__restrict__ hist,
                                                                  float *__restrict__ hist_out, int64_t hist_len, int64_t n)
{
    // the last hist_len samples of (hist || call)
    for (int64_t i = (int64_t)blockIdx.x * RPFB_THREADS + threadIdx.x; i < hist_len; i += (int64_t)gridDim.x * RPFB_THREADS)
        hist_out[i] = stream_load_real<I16>(in, hist, hist_len, n, n - hist_len + i);
}

template <int M, bool I16>
static hipError_t launch_frames(const RpfbArgs &a)
{
    int cus = 0;
    constexpr int lds = (int)rpfb_lds_bytes(M);
    const hipError_t e = stream_kernel_setup<&rpfb_kernel<M, I16>>(a.device, lds, &cus);
    if (e != hipSuccess)
        return e;
    const unsigned groups = stream_persistent_groups(cus, rpfb_groups_per_cu(M), (int64_t)a.call.groups, a.grid_limit);
    hipLaunchKernelGGL((rpfb_kernel<M, I16>), dim3(groups), dim3(RPFB_THREADS), lds, a.stream, a.in, a.hist, a.taps, a.twiddle, a.places,
                       a.untangle, a.out, a.T, a.K, a.D, a.first_bin, a.bins, a.hist_len, a.call.n0, a.call.cmod, (int64_t)a.call.frames,
                       (int64_t)a.call.groups, a.n);
    return hipGetLastError();
}

template <bool I16>
static hipError_t launch_t(const RpfbArgs &a)
{
    if (a.call.frames > 0)
    {
        hipError_t e;
        switch (a.M)
        {
        case 128: e = launch_frames<128, I16>(a); break;
        case 256: e = launch_frames<256, I16>(a); break;
        case 512: e = launch_frames<512, I16>(a); break;
        case 1024: e = launch_frames<1024, I16>(a); break;
        case 2048: e = launch_frames<2048, I16>(a); break;
        case 4096: e = launch_frames<4096, I16>(a); break;
        case 8192: e = launch_frames<8192, I16>(a); break;
        default: e = hipErrorInvalidValue;
        }
        if (e != hipSuccess)
            return e;
    }
    if (a.hist_len > 0)
    {
        const unsigned groups = stream_generic_groups(a.hist_len, RPFB_THREADS, 0);
        hipLaunchKernelGGL((rpfb_carry_kernel<I16>), dim3(groups), dim3(RPFB_THREADS), 0, a.stream, a.in, a.hist, a.hist_out,
                           (int64_t)a.hist_len, a.n);
        return hipGetLastError();
    }
    return hipSuccess;
}

hipError_t launch_rpfb(const RpfbArgs &a)
{
    const uint64_t gf = a.M > 0 ? rpfb_group_frames((uint32_t)a.M) : 1;
    if (!rpfb_size_ok((uint32_t)a.M) || a.T < 1 || a.T > RPFB_MAX_ROWS * a.M || a.K != (int)rpfb_rows((uint32_t)a.T, (uint32_t)a.M) ||
        a.D < 1 || a.D > a.M || a.first_bin < 0 || a.bins < 1 || !rpfb_span_ok((uint32_t)a.first_bin, (uint32_t)a.bins, (uint32_t)a.M) ||
        a.hist_len != a.T - 1 || a.n < 1 || (uint64_t)a.n > RPFB_MAX_CALL || a.call.n0 >= (uint32_t)a.D || a.call.cmod >= (uint32_t)a.M ||
        a.call.frames != ((uint64_t)a.n > a.call.n0 ? ((uint64_t)a.n - a.call.n0 - 1) / (uint64_t)a.D + 1 : 0) ||
        a.call.groups != (a.call.frames + gf - 1) / gf)
        return hipErrorInvalidValue;
    return a.in_i16 ? launch_t<true>(a) : launch_t<false>(a);
}

} // namespace if_fir
