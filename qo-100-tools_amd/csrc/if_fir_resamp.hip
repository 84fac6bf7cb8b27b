// if_fir_resamp.hip — rational L/M resampler for gfx950: one polyphase pass (docs/SPEC.md §7).
//
//   m M = q L + p,  0 <= p < L:   y[m] = sum_{j : p + j L < T} h[p + j L] x[q - j]
//
// fir_resamp_kernel: a WORKGROUP owns tiles of B whole periods = B L outputs <-> B M inputs (+ K - 1 inputs of overlap before
// them, K = ceil(T / L)); the shape comes from resamp_shape (if_fir_resamp_plan.h).  Per tile: the inputs go through coalesced
// global loads into LDS (int16 converted on the way, samples before the call from the history buffer), then lane t of the first
// W = (256 / L) L lanes computes the outputs t, t + W, t + 2 W, t + 3 W of the tile.  W is a multiple of L, so all of them have
// the lane's phase p: one tap read from the phase-major table in LDS feeds RESAMP_R packed FMAs on (I, Q), and for every k the
// lanes store consecutive outputs.  Arithmetic per output (SPEC §7): phase taps in descending j, segments of 16 from +0, added
// in the order they complete with a compensated (two-sum) addition -- the same instructions whatever the tile, the lane or the
// call, so a stream cut anywhere gives the same bits.
// The first workgroup writes the next call's history into the other ping-pong buffer before anything else.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <mutex>
#include <type_traits>

#include "if_fir_kernels.h"
#include "if_fir_resamp.h"
#include "if_fir_stream_dev.h"

namespace if_fir
{

// one tap on RESAMP_R outputs: real h -> one packed FMA each; complex (hr, hi) -> SPEC §3's generic complex formula,
// re = fma(-xi, hi, fma(xr, hr, re)), im = fma(xi, hr, fma(xr, hi, im)), as two packed FMAs
template <bool CT, typename TAP>
__device__ __forceinline__ void rs_tap(const TAP h, const stream_v2f *__restrict__ xs, const int (&x0)[RESAMP_R], int e,
                                       stream_v2f (&seg)[RESAMP_R])
{
#pragma unroll
    for (int k = 0; k < RESAMP_R; k++)
    {
        const stream_v2f x = xs[x0[k] + e];
        if constexpr (CT)
        {
            const stream_v2f xr = {x.x, x.x}, xi = {-x.y, x.y}, hs = {h.y, h.x};
            seg[k] = __builtin_elementwise_fma(xr, h, seg[k]);
            seg[k] = __builtin_elementwise_fma(xi, hs, seg[k]);
        }
        else
        {
            const stream_v2f hh = {h, h};
            seg[k] = __builtin_elementwise_fma(hh, x, seg[k]);
        }
    }
}

// (single LDS reads, if_fir_stream_dev.h: the inner loop is bound by its LDS reads, so this is the kernel's rate)
template <bool I16, bool CT>
__global__ __launch_bounds__(RESAMP_THREADS) IF_FIR_SINGLE_READS void fir_resamp_kernel(const void *__restrict__ in, float2 *__restrict__ out,
                                                                   const float2 *__restrict__ hist, float2 *__restrict__ hist_out,
                                                                   const float *__restrict__ taps, int L, int M, int K, int KP, int B,
                                                                   int t0, int64_t N, int64_t count, int64_t ntiles)
{
    using tap_t = typename std::conditional<CT, stream_v2f, float>::type;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const int hist_len = K - 1;
    if (blockIdx.x == 0) // (its own loop: through a shared helper it compiles to other code, profiles/stream_plan_ab.txt)
        for (int i = tid; i < hist_len; i += RESAMP_THREADS)
        {
            const stream_v2f v = stream_load<I16>(in, hist, hist_len, N, N - hist_len + i);
            hist_out[i] = make_float2(v.x, v.y);
        }
    if ((int64_t)blockIdx.x >= ntiles)
        return; // (uniform per workgroup: a call without outputs only moves the history)
    const int tap_entries = L * KP;
    tap_t *tl = reinterpret_cast<tap_t *>(smem);
    stream_v2f *xs = reinterpret_cast<stream_v2f *>(smem + (((size_t)tap_entries * sizeof(tap_t) + 7) & ~(size_t)7));
    for (int i = tid; i < tap_entries; i += RESAMP_THREADS)
        tl[i] = reinterpret_cast<const tap_t *>(taps)[i];

    // the lane's phase and its RESAMP_R places in a tile
    const int W = (RESAMP_THREADS / L) * L;
    const int tile_out = B * L, tile_in = B * M, x_len = tile_in + K - 1;
    int p, dq;
    resamp_period_entry(t0, tid % L, L, M, &p, &dq);
    const tap_t *row = tl + p * KP;
    int x0[RESAMP_R];    // LDS index of the OLDEST sample of output k (tap j = K - 1); tap j reads x0 + (K - 1 - j)
    bool mine[RESAMP_R];
#pragma unroll
    for (int k = 0; k < RESAMP_R; k++)
    {
        const int i = tid + k * W;
        mine[k] = tid < W && i < tile_out;
        x0[k] = mine[k] ? (i / L) * M + dq : 0; // (idle places read the tile's first K samples and store nothing)
    }
    const int top = stream_top_segment(K);

    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x)
    {
        __syncthreads(); // the previous tile has been read
        const int64_t first = tile * tile_in - (K - 1);
        for (int s = tid; s < x_len; s += RESAMP_THREADS)
            xs[s] = stream_load<I16>(in, hist, hist_len, N, first + s);
        __syncthreads();

        // the total and what its additions lost (two-sum): plain adds of 32-tap segments left 1.01e-6 of the peak on 1023 complex
        // phase taps, past SPEC §3's bound (docs/SPEC.md §7)
        stream_v2f acc[RESAMP_R], lost[RESAMP_R];
#pragma unroll
        for (int k = 0; k < RESAMP_R; k++)
            acc[k] = lost[k] = stream_v2f{0.f, 0.f};
        // e = K - 1 - j counts up from the oldest sample while j walks down through the segments
        int e = 0;
        for (int len = top; e < K; len = STREAM_SEG)
        {
            stream_v2f seg[RESAMP_R];
#pragma unroll
            for (int k = 0; k < RESAMP_R; k++)
                seg[k] = stream_v2f{0.f, 0.f};
            const int end = e + len;
            for (; e + 8 <= end; e += 8)
            {
#pragma unroll
                for (int u = 0; u < 8; u++)
                    rs_tap<CT>(row[K - 1 - e - u], xs, x0, e + u, seg);
            }
            for (; e < end; e++)
                rs_tap<CT>(row[K - 1 - e], xs, x0, e, seg);
#pragma unroll
            for (int k = 0; k < RESAMP_R; k++)
                two_sum_add(acc[k], lost[k], seg[k]);
        }
#pragma unroll
        for (int k = 0; k < RESAMP_R; k++)
            acc[k] += lost[k];
        const int64_t obase = tile * tile_out;
#pragma unroll
        for (int k = 0; k < RESAMP_R; k++)
        {
            const int64_t o = obase + tid + k * W;
            if (mine[k] && o < count)
                out[o] = make_float2(acc[k].x, acc[k].y);
        }
    }
}

template <bool I16, bool CT>
static hipError_t launch_t(const ResampArgs &a)
{
    int cus = 0;
    const hipError_t e = stream_kernel_setup<&fir_resamp_kernel<I16, CT>>(a.device, RESAMP_LDS_MAX, &cus);
    if (e != hipSuccess)
        return e;
    const ResampShape s = resamp_shape(a.T, a.L, a.M);
    const int64_t ntiles = (a.count + s.tile_out - 1) / s.tile_out;
    // a grid-stride loop over the tiles on at most 8 workgroups per CU (more gain nothing: the tap table is staged once per
    // workgroup); at least one, which writes the history
    const unsigned groups = stream_persistent_groups(cus, 8, ntiles, a.grid_limit);
    hipLaunchKernelGGL((fir_resamp_kernel<I16, CT>), dim3(groups), dim3(RESAMP_THREADS), resamp_lds_bytes(s, a.ctaps), a.stream,
                       a.in, static_cast<float2 *>(a.out), a.hist, a.hist_out, a.taps, a.L, a.M, s.K, s.KP, s.B, a.t0, a.N, a.count, ntiles);
    return hipGetLastError();
}

hipError_t launch_resamp(const ResampArgs &a)
{
    if (a.T < 1 || a.T > RESAMP_MAX_TAPS || a.L < 1 || a.L > RESAMP_MAX_L || a.M < 1 || a.M > RESAMP_MAX_M || a.N < 1 || a.count < 0 ||
        a.t0 < 0 || a.t0 >= a.M)
        return hipErrorInvalidValue;
    if (a.in_i16)
        return a.ctaps ? launch_t<true, true>(a) : launch_t<true, false>(a);
    return a.ctaps ? launch_t<false, true>(a) : launch_t<false, false>(a);
}

} // namespace if_fir
