// if_fir_sub.hip — per-channel FIR stage over filter-bank frames for gfx950: every bin of a frame-major stream filtered by its own
// FIR row, decimated and mixed by its own NCO in one pass (docs/SPEC.md §15).
//
//   y_j[n] = e^{-j theta_j n R} sum_k g_j[k] x_j[n R - k],   g_j[k] = h_r[k] e^{+j theta_j k},   x_j[a] = in[a B + j]
//   (the identity of SPEC §3.2 per bin; a = absolute frame index)
//
// fir_sub_kernel: LANES RUN ALONG BINS.  The (output, bin) plane of a call is cut into items of SUB_OUT consecutive outputs of
// one bin, numbered with the bin fastest (sub_tiles, if_fir_sub_plan.h): lane t of a tile takes item tile * 256 + t, so a wave
// reads one run of 64 consecutive elements of a frame (512 bytes, 256 for int16) per tap and output and one run of the tap-major
// table per tap, whatever B is; only the call's last tile has idle lanes.  A lane keeps its SUB_OUT outputs in registers: a tap
// read serves SUB_OUT complex multiply-adds.  No LDS: what neighbouring outputs share of the frames (T / R reads of every
// element) comes from the caches.  Items whose frames all lie inside the call take plain loads; the items at the ends of a call
// go through the bounds-checked stream_load (frames before the call from the history buffer, zeros before the stream) -- the same
// values, and the arithmetic does not know which loaded them.
// Arithmetic per output (SPEC §15): taps in descending k (oldest frame first) in segments of STREAM_SEG from +0, the highest one
// taking what 16 does not divide; finished segments joined by the compensated addition of two_sum_add, its correction added
// once at the end; then the rotation by the phasor of the output's own absolute frame index, skipped for a bin whose word is 0.
// The same instructions whatever the tile, the lane or the call, so a stream cut anywhere gives the same bits.  The kernel sees
// call-relative frames and the low 32 bits of the first output's absolute index, never the position.
// sub_carry_kernel: the last T - 1 frames of (history || call) go to the other ping-pong buffer as float32.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <mutex>

#include "if_fir_kernels.h"
#include "if_fir_stream_dev.h"
#include "if_fir_sub.h"

namespace if_fir
{

// `len` taps from k down on the lane's SUB_OUT outputs, into seg.  tp = the table at the lane's bin (entry k at tp[k B]);
// e0 = the element under output 0 at tap 0, step = R B elements from one output to the next
template <bool I16, bool CHECKED>
__device__ __forceinline__ void sub_segment(const void *__restrict__ in, const float2 *__restrict__ hist, const float2 *__restrict__ tp,
                                            int B, int k, int len, int64_t e0, int64_t step, int64_t hist_len, int64_t N,
                                            stream_v2f (&seg)[SUB_OUT])
{
#pragma unroll SUB_UNROLL
    for (int u = 0; u < len; u++, k--)
    {
        const float2 g = tp[(int64_t)k * B];
        const int64_t e = e0 - (int64_t)k * B;
#pragma unroll
        for (int i = 0; i < SUB_OUT; i++)
        {
            const stream_v2f x = CHECKED ? stream_load<I16>(in, hist, hist_len, N, e + i * step) : stream_sample<I16>(in, e + i * step);
            seg[i].x = fmaf(-x.y, g.y, fmaf(x.x, g.x, seg[i].x));
            seg[i].y = fmaf(x.y, g.x, fmaf(x.x, g.y, seg[i].y));
        }
    }
}

template <bool I16, bool CHECKED>
__device__ __forceinline__ void sub_item(const void *__restrict__ in, float2 *__restrict__ out, const float2 *__restrict__ hist,
                                         const float2 *__restrict__ taps, uint32_t word, int B, int T, int R, int top, int64_t row0,
                                         int j, int64_t o0, uint32_t a0, int64_t hist_len, int64_t N, int64_t count)
{
    stream_v2f acc[SUB_OUT], lost[SUB_OUT], seg[SUB_OUT];
#pragma unroll
    for (int i = 0; i < SUB_OUT; i++)
        acc[i] = lost[i] = stream_v2f{0.f, 0.f};
    const int64_t e0 = row0 * B + j, step = (int64_t)R * B;
    for (int k = T - 1, len = top; k >= 0; k -= len, len = STREAM_SEG)
    {
#pragma unroll
        for (int i = 0; i < SUB_OUT; i++)
            seg[i] = stream_v2f{0.f, 0.f};
        sub_segment<I16, CHECKED>(in, hist, taps + j, B, k, len, e0, step, hist_len, N, seg);
#pragma unroll
        for (int i = 0; i < SUB_OUT; i++)
            two_sum_add(acc[i], lost[i], seg[i]);
    }
#pragma unroll
    for (int i = 0; i < SUB_OUT; i++)
    {
        const int64_t o = o0 + i;
        stream_v2f v = acc[i] + lost[i];
        if (word)
        {
            // the phase of the output's own absolute frame index: -(P a) mod 2^32, a = a0 + o R
            const float2 w = nco_phasor(0u - word * (a0 + (uint32_t)o * (uint32_t)R));
            v = stream_v2f{fmaf(v.x, w.x, -v.y * w.y), fmaf(v.x, w.y, v.y * w.x)};
        }
        if (o < count)
            out[o * B + j] = make_float2(v.x, v.y);
    }
}

template <bool I16>
__global__ __launch_bounds__(SUB_THREADS) void fir_sub_kernel(const void *__restrict__ in, float2 *__restrict__ out,
                                                              const float2 *__restrict__ hist, const float2 *__restrict__ taps,
                                                              const uint32_t *__restrict__ words, int B, int T, int R, int n0, uint32_t a0,
                                                              int64_t F, int64_t count, int64_t items, int64_t ntiles)
{
    const int top = stream_top_segment(T);
    const int64_t hist_len = (int64_t)(T - 1) * B, N = F * B;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x)
    {
        const int64_t item = tile * SUB_THREADS + threadIdx.x;
        if (item >= items)
            continue; // (no barrier in this kernel)
        const int64_t run = item / B;
        const int j = (int)(item - run * B);
        const int64_t o0 = run * SUB_OUT, row0 = (int64_t)n0 + o0 * R;
        const uint32_t word = words[j];
        // every frame the item's SUB_OUT outputs weigh lies inside the call (then they are all outputs of the call, too)
        if (row0 - (T - 1) >= 0 && row0 + (int64_t)(SUB_OUT - 1) * R < F)
            sub_item<I16, false>(in, out, hist, taps, word, B, T, R, top, row0, j, o0, a0, hist_len, N, count);
        else
            sub_item<I16, true>(in, out, hist, taps, word, B, T, R, top, row0, j, o0, a0, hist_len, N, count);
    }
}

template <bool I16>
__global__ __launch_bounds__(SUB_THREADS) void sub_carry_kernel(const void *__restrict__ in, const float2 *__restrict__ hist,
                                                                float2 *__restrict__ hist_out, int64_t hist_len, int64_t N)
{
    // the last hist_len elements of (hist || call) (its own loop, as pfb_carry_kernel's)
    for (int64_t i = (int64_t)blockIdx.x * SUB_THREADS + threadIdx.x; i < hist_len; i += (int64_t)gridDim.x * SUB_THREADS)
    {
        const stream_v2f v = stream_load<I16>(in, hist, hist_len, N, N - hist_len + i);
        hist_out[i] = make_float2(v.x, v.y);
    }
}

template <bool I16>
static hipError_t launch_t(const SubArgs &a)
{
    const SubTiles t = sub_tiles((uint32_t)a.B, a.call.count);
    if (t.tiles > 0)
    {
        int cus = 0;
        const hipError_t e = stream_kernel_setup<&fir_sub_kernel<I16>>(a.device, 0, &cus);
        if (e != hipSuccess)
            return e;
        // a grid-stride loop over the tiles on as many workgroups as are resident at a time
        const unsigned groups = stream_persistent_groups(cus, SUB_GROUPS_PER_CU, (int64_t)t.tiles, a.grid_limit);
        hipLaunchKernelGGL((fir_sub_kernel<I16>), dim3(groups), dim3(SUB_THREADS), 0, a.stream, a.in, a.out, a.hist, a.taps, a.words, a.B,
                           a.T, a.R, (int)a.call.n0, a.call.a0, a.F, (int64_t)a.call.count, (int64_t)t.items, (int64_t)t.tiles);
        const hipError_t le = hipGetLastError();
        if (le != hipSuccess)
            return le;
    }
    const int64_t hist_len = (int64_t)(a.T - 1) * a.B;
    if (hist_len > 0)
    {
        hipLaunchKernelGGL((sub_carry_kernel<I16>), dim3(stream_generic_groups(hist_len, SUB_THREADS, a.grid_limit)), dim3(SUB_THREADS), 0,
                           a.stream, a.in, a.hist, a.hist_out, hist_len, a.F * a.B);
        return hipGetLastError();
    }
    return hipSuccess;
}

hipError_t launch_sub(const SubArgs &a)
{
    if (a.B < 1 || a.B > (int)SUB_MAX_BINS || a.T < 1 || a.T > (int)SUB_MAX_TAPS || a.R < 1 || a.R > (int)SUB_MAX_DECIMATION || a.F < 1 ||
        (uint64_t)a.F > SUB_MAX_FRAMES || a.call.n0 >= (uint32_t)a.R ||
        a.call.count != ((uint64_t)a.F > a.call.n0 ? ((uint64_t)a.F - a.call.n0 - 1) / (uint64_t)a.R + 1 : 0))
        return hipErrorInvalidValue;
    return a.in_i16 ? launch_t<true>(a) : launch_t<false>(a);
}

} // namespace if_fir
