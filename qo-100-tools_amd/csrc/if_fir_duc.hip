// if_fir_duc.hip — real-output up-converter for gfx950: complex baseband to a real IF stream at L times the rate in one pass
// (docs/SPEC.md §11).
//
//   y[q L + p] = sum_j ( g_r[p + j L] x'_r[q - j] - g_i[p + j L] x'_i[q - j] ),   g[k] = h[k] e^{+j theta k},   x'[n] = x[n] e^{+j theta L n}
//
// fir_duc_kernel: a WORKGROUP owns tiles of Q consecutive input samples <-> the L Q outputs they produce (the shape comes from
// duc_shape, if_fir_duc_plan.h).  Per tile:
//   fill     the Q + KP - 1 samples of the window go through coalesced global loads into LDS as (re, im) pairs, int16 converted
//            and the sample ROTATED on the way (one nco_phasor per input sample, of the exact word of its absolute index).  A
//            window inside the call is filled with plain loads, DUC_FILL per lane in flight; the windows at the ends of a call go
//            through the bounds-checked stream_load (same values: the arithmetic does not know which filled its tile).
//   compute  a WAVE takes one phase p and a run of 256 consecutive q; lane t the DUC_R = 4 outputs q = 4 t .. 4 t + 3 of that
//            phase.  It slides a register window along x': one 16-byte LDS read (dense across the lanes) brings two samples, for
//            two taps x four outputs = 8 packed FMAs on (g_r x'_r, -g_i x'_i).  The taps are wave-uniform: read front to back
//            from the table of duc_build_table through the scalar cache.  The four results of a lane go to the staging area in
//            LDS, phase-major, as one 16-byte store.
//   store    the staging area is read in output order (index q L + p) and written to memory in dense runs: one float32 per
//            lane, or two int16 packed into an aligned dword per lane with single int16 stores where a pair is cut by the tile's
//            ends or by an odd element alignment of the output pointer.
// Arithmetic per output (SPEC §11): the row entries front to back (descending j: oldest sample first); segments from +0 that
// end after `top` entries and then after every 16th, joined by the compensated addition of two_sum_add; then the two halves
// are added -- the same instructions whatever the tile, the lane or the call, so a stream cut anywhere gives the same bits.
// The first workgroup writes the next call's history (unrotated) into the other ping-pong buffer before anything else.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <mutex>

#include "if_fir_duc.h"
#include "if_fir_kernels.h"
#include "if_fir_stream_dev.h"

namespace if_fir
{

typedef float duc_v4f __attribute__((ext_vector_type(4)));

constexpr int DUC_FILL = 4; // loads a lane has in flight while it fills an interior window

// x'[n] = x[n] e^{+j theta L n}: the phasor of the exact word (P L n) mod 2^32, n the sample's absolute index (j = its index in
// the call, negative in the history)
__device__ __forceinline__ float2 duc_rotate(stream_v2f v, uint32_t nco_on, uint32_t phi0, uint32_t delta, int64_t j)
{
    if (nco_on)
    {
        const float2 w = nco_phasor(phi0 + (uint32_t)j * delta);
        return make_float2(fmaf(v.x, w.x, -(v.y * w.y)), fmaf(v.x, w.y, v.y * w.x));
    }
    return make_float2(v.x, v.y);
}

// (single LDS reads, if_fir_stream_dev.h)
template <bool I16, bool O16>
__global__ __launch_bounds__(DUC_THREADS) IF_FIR_SINGLE_READS void fir_duc_kernel(const void *__restrict__ in, void *__restrict__ out,
                                                                const float2 *__restrict__ hist, float2 *__restrict__ hist_out,
                                                                const float2 *__restrict__ taps, int L, int K, int KP, int top, int Q,
                                                                int RS, int64_t N, int64_t count, int64_t ntiles, uint32_t nco_on,
                                                                uint32_t phi0, uint32_t delta, uint32_t magic)
{
    extern __shared__ __attribute__((aligned(16))) float duc_lds[];
    float *xs = duc_lds;                   // the window: Q + KP (re, im) pairs
    float *stage = duc_lds + 2 * (Q + KP); // the tile's outputs: L rows of RS floats
    const int tid = threadIdx.x;
    const int hist_len = K - 1;
    if (blockIdx.x == 0) // (its own loop: through a shared helper it compiles to other code, profiles/stream_plan_ab.txt)
        for (int i = tid; i < hist_len; i += DUC_THREADS)
        {
            const stream_v2f v = stream_load<I16>(in, hist, hist_len, N, N - hist_len + i);
            hist_out[i] = make_float2(v.x, v.y);
        }
    const int W = Q + KP - 1;
    const int tile_out = Q * L;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int items = L * (Q / DUC_RUN);

    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x)
    {
        __syncthreads(); // the previous tile's window and staging area have been read
        const int64_t jfirst = tile * Q - (KP - 1);
        if (jfirst >= 0 && jfirst + W <= N)
        {
            // the whole window lies inside the call: plain loads, several in flight per lane (a load behind a bounds check is
            // waited for before the next one is asked for)
            for (int w0 = tid; w0 < W; w0 += DUC_FILL * DUC_THREADS)
            {
                stream_v2f v[DUC_FILL];
#pragma unroll
                for (int u = 0; u < DUC_FILL; u++)
                {
                    // (past the last sample: the last one again, loaded and not stored)
                    const int w = w0 + u * DUC_THREADS < W ? w0 + u * DUC_THREADS : W - 1;
                    v[u] = stream_sample<I16>(in, jfirst + w);
                }
#pragma unroll
                for (int u = 0; u < DUC_FILL; u++)
                {
                    const int w = w0 + u * DUC_THREADS;
                    if (w < W)
                        *reinterpret_cast<float2 *>(xs + 2 * w) = duc_rotate(v[u], nco_on, phi0, delta, jfirst + w);
                }
            }
        }
        else
            for (int w = tid; w < W; w += DUC_THREADS)
                *reinterpret_cast<float2 *>(xs + 2 * w) =
                    duc_rotate(stream_load<I16>(in, hist, hist_len, N, jfirst + w), nco_on, phi0, delta, jfirst + w);
        __syncthreads();

        for (int it = wave; it < items; it += DUC_THREADS / 64)
        {
            const int qb = it / L, p = it - qb * L; // (wave-uniform)
            const int q0 = qb * DUC_RUN + DUC_R * lane;
            const duc_v4f *x = reinterpret_cast<const duc_v4f *>(xs + 2 * q0); // two samples per element
            const float2 *tp = taps + p * KP;
            stream_v2f acc[DUC_R], lost[DUC_R], seg[DUC_R];
#pragma unroll
            for (int i = 0; i < DUC_R; i++)
                acc[i] = lost[i] = seg[i] = stream_v2f{0.f, 0.f};
            duc_v4f a = x[0], b = x[1], c = x[2];
            float2 t0 = tp[0], t1 = tp[1];
            int join = top;
            for (int e = 0; e < KP; e += 2)
            {
                // the next step's samples and taps are requested ahead of this step's 8 FMAs (the last step asks for its own
                // again: nothing is read beyond the window)
                const int en = e + 2 < KP ? e + 2 : e;
                const duc_v4f cn = x[en / 2 + 2];
                const float2 n0 = tp[en], n1 = tp[en + 1];
                __builtin_amdgcn_sched_barrier(0); // (the scheduler would sink the requests down to their use)
                const stream_v2f win[5] = {{a.x, a.y}, {a.z, a.w}, {b.x, b.y}, {b.z, b.w}, {c.x, c.y}};
                const stream_v2f g0 = {t0.x, t0.y}, g1 = {t1.x, t1.y};
#pragma unroll
                for (int i = 0; i < DUC_R; i++)
                    seg[i] = __builtin_elementwise_fma(g0, win[i], seg[i]);
#pragma unroll
                for (int i = 0; i < DUC_R; i++)
                    seg[i] = __builtin_elementwise_fma(g1, win[i + 1], seg[i]);
                a = b;
                b = c;
                c = cn;
                t0 = n0;
                t1 = n1;
                if (e + 2 == join)
                {
#pragma unroll
                    for (int i = 0; i < DUC_R; i++)
                    {
                        two_sum_add(acc[i], lost[i], seg[i]);
                        seg[i] = stream_v2f{0.f, 0.f};
                    }
                    join += DUC_SEG;
                }
            }
            duc_v4f y;
#pragma unroll
            for (int i = 0; i < DUC_R; i++)
            {
                const stream_v2f v = acc[i] + lost[i];
                y[i] = v.x + v.y;
            }
            *reinterpret_cast<duc_v4f *>(stage + p * RS + q0) = y;
        }
        __syncthreads();

        // the tile's outputs in index order: n = q L + p lies at stage[p RS + q]
        const int64_t tb = tile * tile_out;
        const int valid = count - tb < tile_out ? (int)(count - tb) : tile_out; // >= 1
        if constexpr (!O16)
        {
            float *o = static_cast<float *>(out) + tb;
            for (int n = tid; n < valid; n += DUC_THREADS)
            {
                const int q = (int)(((uint64_t)n * magic) >> DUC_DIV_SHIFT), p = n - q * L;
                o[n] = stage[p * RS + q];
            }
        }
        else
        {
            // dword d of the tile holds its elements 2 d - odd and 2 d - odd + 1 (tb is even: the pointer's own element parity
            // decides which pairs share an aligned dword)
            short *o = static_cast<short *>(out) + tb;
            const int odd = (int)((reinterpret_cast<uintptr_t>(out) >> 1) & 1);
            for (int d = tid; 2 * d - odd < valid; d += DUC_THREADS)
            {
                const int e0 = 2 * d - odd, e1 = e0 + 1;
                const bool ok0 = e0 >= 0, ok1 = e1 < valid;
                const int n0 = ok0 ? e0 : e1, n1 = ok1 ? e1 : e0; // (both inside the tile)
                const int qa = (int)(((uint64_t)n0 * magic) >> DUC_DIV_SHIFT), qc = (int)(((uint64_t)n1 * magic) >> DUC_DIV_SHIFT);
                const int16_t s0 = duc_to_i16(stage[(n0 - qa * L) * RS + qa]), s1 = duc_to_i16(stage[(n1 - qc * L) * RS + qc]);
                if (ok0 && ok1)
                    *reinterpret_cast<uint32_t *>(o + e0) = (uint32_t)(uint16_t)s0 | ((uint32_t)(uint16_t)s1 << 16);
                else if (ok0)
                    o[e0] = s0;
                else
                    o[e1] = s1;
            }
        }
    }
}

template <bool I16, bool O16>
static hipError_t launch_t(const DucArgs &a)
{
    int cus = 0;
    const hipError_t e = stream_kernel_setup<&fir_duc_kernel<I16, O16>>(a.device, DUC_LDS_MAX, &cus);
    if (e != hipSuccess)
        return e;
    const DucShape s = duc_shape(a.T, a.L);
    const int64_t ntiles = (a.N + s.Q - 1) / s.Q;
    // a grid-stride loop over the tiles on as many workgroups as are resident at a time; at least one, which writes the history
    const unsigned groups = stream_persistent_groups(cus, duc_groups_per_cu(s, a.L), ntiles, a.grid_limit);
    const uint32_t delta = a.nco_word * (uint32_t)a.L;
    hipLaunchKernelGGL((fir_duc_kernel<I16, O16>), dim3(groups), dim3(DUC_THREADS), duc_lds_bytes(s, a.L), a.stream, a.in, a.out, a.hist,
                       a.hist_out, reinterpret_cast<const float2 *>(a.taps), a.L, s.K, s.KP, s.top, s.Q, s.RS, a.N, a.N * a.L, ntiles,
                       a.nco_word != 0 ? 1u : 0u, delta * a.nco_abs0, delta, duc_div_magic(a.L));
    return hipGetLastError();
}

hipError_t launch_duc(const DucArgs &a)
{
    if (a.T < 1 || a.T > DUC_MAX_TAPS || a.L < 1 || a.L > DUC_MAX_L || a.N < 1)
        return hipErrorInvalidValue;
    if (a.in_i16)
        return a.out_i16 ? launch_t<true, true>(a) : launch_t<true, false>(a);
    return a.out_i16 ? launch_t<false, true>(a) : launch_t<false, false>(a);
}

} // namespace if_fir
