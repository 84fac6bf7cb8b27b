// if_fir_subup.hip — per-bin interpolating FIR stage over frames for gfx950: every bin of a frame-major stream interpolated by
// R through its own FIR row and mixed up by its own NCO in one pass (docs/SPEC.md §16).
//
//   y_j[m R + p] = e^{+j theta_j (m R + p)} sum_{i<J} h_r[p + i R] x_j[m - i],   x_j[m] = in[m B + j],   J = ceil(T / R)
//
// fir_subup_kernel: LANES RUN ALONG BINS.  An item is one (bin j, phase p) over a run of SUBUP_Q consecutive input frames,
// numbered with the bin fastest, then the phase (subup_tiles, if_fir_subup_plan.h): lane t of a tile takes item tile * 256 + t,
// so a wave reads runs of consecutive elements of a frame and writes 64 consecutive elements of the output per step, whatever B
// is; only the call's last tile has idle lanes.  A lane keeps its J taps h_r[p + i R] and a window of the last J input values
// in registers: per step one load, J x 2 FMAs, one phasor, one store.  The window is a ring whose slot numbers are
// compile-time constants: the walk is unrolled in blocks of a multiple of JB steps (JB = the bucket of J: 1, 2, 4, 8, 16, 32), so
// nothing moves between registers; a block's loads are issued together before its first step (measured: 7-20 % faster than a
// load per step).  No LDS: the R lanes that share an input sit in other waves and meet in the caches.
// Items whose frames all lie inside the call take plain loads; the items at the ends of a call go through the bounds-checked
// stream_load (frames before the call from the history buffer, zeros before the stream) -- the same values, and the
// arithmetic does not know which loaded them.
// Arithmetic per output and component (SPEC §16): one chain from +0 over i = JB - 1 .. 0 (oldest frame first) of
// fma(h, x, acc), the taps at p + i R >= T being zeros of the table (they come first in the chain, where they leave +0); then the
// rotation by the phasor of the output's own absolute index, skipped for a bin whose word is 0.  The same instructions
// whatever the tile, the lane or the call, so a stream cut anywhere gives the same bits.  The kernel sees call-relative frames
// and the low 32 bits of the first output's absolute index, never the position.
// subup_carry_kernel: the last J - 1 frames of (history || call) go to the other ping-pong buffer as float32.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <mutex>

#include "if_fir_kernels.h"
#include "if_fir_stream_dev.h"
#include "if_fir_subup.h"

namespace if_fir
{

template <bool I16, bool CHECKED, int JB>
__device__ __forceinline__ void subup_item(const void *__restrict__ in, float2 *__restrict__ out, const float2 *__restrict__ hist,
                                           const float *__restrict__ tp, uint32_t word, int B, int J, int R, int rows, int64_t m0, int p,
                                           int j, uint32_t n0, int64_t hist_len, int64_t F)
{
    constexpr int BLOCK = JB < 8 ? 8 : JB; // steps unrolled together: a multiple of JB, so a frame's slot is a constant
    const int64_t N = F * B;
    float h[JB];
    stream_v2f win[JB];
#pragma unroll
    for (int i = 0; i < JB; i++)
        h[i] = i < J ? tp[(int64_t)(p + i * R) * rows] : 0.f;
    // the J - 1 frames before the run: frame m0 - d in slot (JB - d) mod JB
    win[0] = stream_v2f{0.f, 0.f};
#pragma unroll
    for (int d = 1; d < JB; d++)
    {
        win[JB - d] = stream_v2f{0.f, 0.f};
        if (d < J)
            win[JB - d] = CHECKED ? stream_load<I16>(in, hist, hist_len, N, (m0 - d) * B + j) : stream_sample<I16>(in, (m0 - d) * B + j);
    }
    for (int blk = 0; blk < SUBUP_Q / BLOCK; blk++)
    {
        const int64_t mb = m0 + blk * BLOCK;
        if (CHECKED && mb >= F)
            break;
        // the block's loads first, all in flight together
        stream_v2f next[BLOCK];
#pragma unroll
        for (int s = 0; s < BLOCK; s++)
            next[s] = CHECKED ? stream_load<I16>(in, hist, hist_len, N, (mb + s) * B + j) : stream_sample<I16>(in, (mb + s) * B + j);
#pragma unroll
        for (int s = 0; s < BLOCK; s++)
        {
            const int64_t m = mb + s;
            win[s % JB] = next[s];
            stream_v2f v = {0.f, 0.f};
#pragma unroll
            for (int i = JB - 1; i >= 0; i--)
            {
                const stream_v2f x = win[((s - i) % JB + JB) % JB];
                v.x = fmaf(h[i], x.x, v.x);
                v.y = fmaf(h[i], x.y, v.y);
            }
            const int64_t o = m * R + p;
            if (word)
            {
                // the phase of the output's own absolute index: (P n) mod 2^32, n = n0 + o
                const float2 w = nco_phasor(word * (n0 + (uint32_t)o));
                v = stream_v2f{fmaf(v.x, w.x, -(v.y * w.y)), fmaf(v.x, w.y, v.y * w.x)};
            }
            if (!CHECKED || m < F)
                out[o * B + j] = make_float2(v.x, v.y);
        }
    }
}

template <bool I16, int JB>
__global__ __launch_bounds__(SUBUP_THREADS) void fir_subup_kernel(const void *__restrict__ in, float2 *__restrict__ out,
                                                                  const float2 *__restrict__ hist, const float *__restrict__ taps,
                                                                  const uint32_t *__restrict__ words, int B, int J, int R, int rows,
                                                                  uint32_t n0, int64_t F, int64_t items, int64_t ntiles)
{
    const int64_t hist_len = (int64_t)(J - 1) * B;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x)
    {
        const int64_t item = tile * SUBUP_THREADS + threadIdx.x;
        if (item >= items)
            continue; // (no barrier in this kernel)
        uint64_t m0;
        uint32_t p, j;
        subup_item_place((uint64_t)item, (uint32_t)B, (uint32_t)R, &m0, &p, &j);
        const uint32_t word = words[j];
        const float *tp = taps + (rows == 1 ? 0 : (int)j);
        // every frame the run's outputs weigh, and the whole run, lies inside the call
        if ((int64_t)m0 - (J - 1) >= 0 && (int64_t)m0 + SUBUP_Q <= F)
            subup_item<I16, false, JB>(in, out, hist, tp, word, B, J, R, rows, (int64_t)m0, (int)p, (int)j, n0, hist_len, F);
        else
            subup_item<I16, true, JB>(in, out, hist, tp, word, B, J, R, rows, (int64_t)m0, (int)p, (int)j, n0, hist_len, F);
    }
}

template <bool I16>
__global__ __launch_bounds__(SUBUP_THREADS) void subup_carry_kernel(const void *__restrict__ in, const float2 *__restrict__ hist,
                                                                    float2 *__restrict__ hist_out, int64_t hist_len, int64_t N)
{
    // the last hist_len elements of (hist || call) (its own loop, as sub_carry_kernel's)
    for (int64_t i = (int64_t)blockIdx.x * SUBUP_THREADS + threadIdx.x; i < hist_len; i += (int64_t)gridDim.x * SUBUP_THREADS)
    {
        const stream_v2f v = stream_load<I16>(in, hist, hist_len, N, N - hist_len + i);
        hist_out[i] = make_float2(v.x, v.y);
    }
}

template <bool I16, int JB>
static hipError_t launch_stage(const SubUpArgs &a, int J, const SubUpTiles &t)
{
    int cus = 0;
    const hipError_t e = stream_kernel_setup<&fir_subup_kernel<I16, JB>>(a.device, 0, &cus);
    if (e != hipSuccess)
        return e;
    // a grid-stride loop over the tiles on as many workgroups as are resident at a time
    const unsigned groups = stream_persistent_groups(cus, subup_groups_per_cu(JB), (int64_t)t.tiles, a.grid_limit);
    hipLaunchKernelGGL((fir_subup_kernel<I16, JB>), dim3(groups), dim3(SUBUP_THREADS), 0, a.stream, a.in, a.out, a.hist, a.taps, a.words, a.B,
                       J, a.R, a.rows, a.call.n0, a.F, (int64_t)t.items, (int64_t)t.tiles);
    return hipGetLastError();
}

template <bool I16>
static hipError_t launch_t(const SubUpArgs &a)
{
    const int J = (int)subup_j((uint32_t)a.T, (uint32_t)a.R);
    const SubUpTiles t = subup_tiles((uint32_t)a.B, (uint32_t)a.R, (uint64_t)a.F);
    hipError_t e = hipErrorInvalidValue;
    switch (subup_bucket((uint32_t)J))
    {
    case 1: e = launch_stage<I16, 1>(a, J, t); break;
    case 2: e = launch_stage<I16, 2>(a, J, t); break;
    case 4: e = launch_stage<I16, 4>(a, J, t); break;
    case 8: e = launch_stage<I16, 8>(a, J, t); break;
    case 16: e = launch_stage<I16, 16>(a, J, t); break;
    case 32: e = launch_stage<I16, 32>(a, J, t); break;
    }
    if (e != hipSuccess)
        return e;
    const int64_t hist_len = (int64_t)(J - 1) * a.B;
    if (hist_len > 0)
    {
        hipLaunchKernelGGL((subup_carry_kernel<I16>), dim3(stream_generic_groups(hist_len, SUBUP_THREADS, a.grid_limit)), dim3(SUBUP_THREADS),
                           0, a.stream, a.in, a.hist, a.hist_out, hist_len, a.F * a.B);
        return hipGetLastError();
    }
    return hipSuccess;
}

hipError_t launch_subup(const SubUpArgs &a)
{
    if (a.B < 1 || a.B > (int)SUBUP_MAX_BINS || a.T < 1 || a.T > (int)SUBUP_MAX_TAPS || a.R < 1 || a.R > (int)SUBUP_MAX_INTERPOLATION ||
        subup_j((uint32_t)a.T, (uint32_t)a.R) > SUBUP_MAX_J || (a.rows != 1 && a.rows != a.B) || a.F < 1 ||
        (uint64_t)a.F > SUBUP_MAX_FRAMES || a.call.count != (uint64_t)a.F * (uint64_t)a.R)
        return hipErrorInvalidValue;
    return a.in_i16 ? launch_t<true>(a) : launch_t<false>(a);
}

} // namespace if_fir
