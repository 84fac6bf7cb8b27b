// if_fir_arb.hip — arbitrary-ratio resampler for gfx950: a polyphase filter of P = 2^b phases whose taps are interpolated
// linearly between neighbouring phases, at a step R that is any 64-bit number (docs/SPEC.md §12).
//
//   q = floor(tau / 2^32), f = tau mod 2^32, p = f >> (32 - b), mu = (f mod 2^(32 - b)) / 2^(32 - b)
//   y = sum_j [(1 - mu) h[p + j P] + mu h[p + 1 + j P]] x[q - j],   then tau += R
//
// fir_arb_kernel: a WORKGROUP owns tiles of ARB_TILE_OUT = 1024 consecutive outputs.  A tile's base time comes from one
// 64 x 64 -> 128 multiply (arb_time, if_fir_arb_plan.h); its window of arb_window(K, R) input samples goes through coalesced
// global loads into LDS (int16 converted on the way; a window inside the call with plain loads, one that touches the call's
// edges through the bounds-checked stream_load, which also serves the history), next to the tap table.  Lane t computes the
// outputs t, t + 256, t + 512, t + 768 of the tile, so every store of the workgroup is one run.  Unlike the rational resampler
// every output has a phase of its own: the table holds, for phase p and tap j, the PAIR (h[p + j P], h[p + 1 + j P]), so one
// 8-byte LDS read gives the taps of both neighbouring phases and one more gives the sample.
// Arithmetic per output (SPEC §12, order A): two dot products, A over phase p and B over phase p + 1, each in SPEC §7's order --
// taps in descending j, segments of 16 from +0, added in the order they complete with a compensated (two-sum) addition -- then
// y = fma(mu, B - A, A).  The same instructions whatever the tile, the lane or the call, on values that depend only on the
// output's own (q, p, mu): a stream cut anywhere gives the same bits.
// The first workgroup writes the next call's history into the other ping-pong buffer before anything else.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <mutex>
#include <type_traits>

#include "if_fir_arb.h"
#include "if_fir_kernels.h"
#include "if_fir_stream_dev.h"

namespace if_fir
{

// one tap position on the ARB_R outputs of a lane: the pair of taps and the sample, two packed FMAs on (I, Q)
__device__ __forceinline__ void arb_tap(const stream_v2f *__restrict__ tl, const stream_v2f *__restrict__ xs, const int (&r0)[ARB_R],
                                        const int (&x0)[ARB_R], int j, int e, stream_v2f (&sa)[ARB_R], stream_v2f (&sb)[ARB_R])
{
#pragma unroll
    for (int k = 0; k < ARB_R; k++)
    {
        const stream_v2f h = tl[r0[k] + j];
        const stream_v2f x = xs[x0[k] + e];
        const stream_v2f ha = {h.x, h.x}, hb = {h.y, h.y};
        sa[k] = __builtin_elementwise_fma(ha, x, sa[k]);
        sb[k] = __builtin_elementwise_fma(hb, x, sb[k]);
    }
}

// (single LDS reads, if_fir_stream_dev.h: the inner loop is bound by its LDS reads)
template <bool I16>
__global__ __launch_bounds__(ARB_THREADS) IF_FIR_SINGLE_READS void fir_arb_kernel(const void *__restrict__ in, float2 *__restrict__ out,
                                                                                   const float2 *__restrict__ hist, float2 *__restrict__ hist_out,
                                                                                   const float *__restrict__ taps, int bits, int K, int KP, int x_len,
                                                                                   uint64_t R, uint64_t tau_rel, int64_t N, int64_t count,
                                                                                   int64_t ntiles)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const int hist_len = K - 1;
    if (blockIdx.x == 0) // (its own loop: through a shared helper it compiles to other code, profiles/stream_plan_ab.txt)
        for (int i = tid; i < hist_len; i += ARB_THREADS)
        {
            const stream_v2f v = stream_load<I16>(in, hist, hist_len, N, N - hist_len + i);
            hist_out[i] = make_float2(v.x, v.y);
        }
    if ((int64_t)blockIdx.x >= ntiles)
        return; // (uniform per workgroup: a call without outputs only moves the history)
    const int tap_entries = (1 << bits) * KP;
    stream_v2f *tl = reinterpret_cast<stream_v2f *>(smem);
    stream_v2f *xs = tl + tap_entries;
    for (int i = tid; i < tap_entries; i += ARB_THREADS)
        tl[i] = reinterpret_cast<const stream_v2f *>(taps)[i];
    const int top = stream_top_segment(K);

    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x)
    {
        __syncthreads(); // the previous tile has been read
        int64_t q0;
        uint32_t f0;
        arb_time(tau_rel, (uint64_t)tile * ARB_TILE_OUT, R, &q0, &f0);
        const int64_t first = q0 - (K - 1); // >= -hist_len
        if (first >= 0 && first + x_len <= N)
            // the whole window lies inside the call: plain loads
            for (int s = tid; s < x_len; s += ARB_THREADS)
                xs[s] = stream_sample<I16>(in, first + s);
        else
            for (int s = tid; s < x_len; s += ARB_THREADS)
                xs[s] = stream_load<I16>(in, hist, hist_len, N, first + s);
        __syncthreads();

        // the lane's ARB_R places: LDS index of the OLDEST sample of output k (tap j = K - 1; tap j reads x0 + (K - 1 - j)), the
        // row of its phase and its fraction.  A place past the call's last output computes on the window like any other (its
        // indices stay inside both arrays) and stores nothing.
        int x0[ARB_R], r0[ARB_R];
        float mu[ARB_R];
#pragma unroll
        for (int k = 0; k < ARB_R; k++)
        {
            int p;
            arb_place(f0, tid + k * ARB_THREADS, R, bits, &x0[k], &p, &mu[k]);
            r0[k] = p * KP;
        }

        stream_v2f acc_a[ARB_R], lost_a[ARB_R], acc_b[ARB_R], lost_b[ARB_R];
#pragma unroll
        for (int k = 0; k < ARB_R; k++)
            acc_a[k] = lost_a[k] = acc_b[k] = lost_b[k] = stream_v2f{0.f, 0.f};
        // e = K - 1 - j counts up from the oldest sample while j walks down through the segments
        int e = 0;
        for (int len = top; e < K; len = STREAM_SEG)
        {
            stream_v2f sa[ARB_R], sb[ARB_R];
#pragma unroll
            for (int k = 0; k < ARB_R; k++)
                sa[k] = sb[k] = stream_v2f{0.f, 0.f};
            const int end = e + len;
            for (; e + 8 <= end; e += 8)
            {
#pragma unroll
                for (int u = 0; u < 8; u++)
                    arb_tap(tl, xs, r0, x0, K - 1 - e - u, e + u, sa, sb);
            }
            for (; e < end; e++)
                arb_tap(tl, xs, r0, x0, K - 1 - e, e, sa, sb);
#pragma unroll
            for (int k = 0; k < ARB_R; k++)
            {
                two_sum_add(acc_a[k], lost_a[k], sa[k]);
                two_sum_add(acc_b[k], lost_b[k], sb[k]);
            }
        }
        const int64_t obase = tile * ARB_TILE_OUT;
#pragma unroll
        for (int k = 0; k < ARB_R; k++)
        {
            const stream_v2f a = acc_a[k] + lost_a[k], b = acc_b[k] + lost_b[k];
            const stream_v2f m = {mu[k], mu[k]};
            const stream_v2f y = __builtin_elementwise_fma(m, b - a, a);
            const int64_t o = obase + tid + k * ARB_THREADS;
            if (o < count)
                out[o] = make_float2(y.x, y.y);
        }
    }
}

template <bool I16>
static hipError_t launch_t(const ArbArgs &a)
{
    int cus = 0;
    const hipError_t e = stream_kernel_setup<&fir_arb_kernel<I16>>(a.device, ARB_LDS_MAX, &cus);
    if (e != hipSuccess)
        return e;
    const ArbShape s = arb_shape(a.T, a.bits, a.step);
    const int64_t ntiles = (a.count + s.tile_out - 1) / s.tile_out;
    // a grid-stride loop over the tiles on at most 8 workgroups per CU (the tap table is staged once per workgroup); at least
    // one, which writes the history
    const unsigned groups = stream_persistent_groups(cus, 8, ntiles, a.grid_limit);
    hipLaunchKernelGGL((fir_arb_kernel<I16>), dim3(groups), dim3(ARB_THREADS), arb_lds_bytes(s), a.stream, a.in,
                       static_cast<float2 *>(a.out), a.hist, a.hist_out, a.taps, a.bits, s.K, s.KP, s.x_len, a.step, a.tau_rel, a.N, a.count,
                       ntiles);
    return hipGetLastError();
}

hipError_t launch_arb(const ArbArgs &a)
{
    if (a.T < 1 || a.bits < 0 || !arb_valid((uint32_t)a.T, (uint32_t)a.bits, a.step) || a.N < 1 || a.N > (int64_t)ARB_MAX_SAMPLES ||
        a.count < 0 || a.tau_rel >= ((uint64_t)1 << 34))
        return hipErrorInvalidValue;
    return a.in_i16 ? launch_t<true>(a) : launch_t<false>(a);
}

} // namespace if_fir
