// if_fir_ddc.hip — real-input down-converter for gfx950: real IF samples to decimated complex baseband in one pass
// (docs/SPEC.md §10).
//
//   y[m D] = e^{-j theta m D} sum_k g[k] r[m D - k],   g[k] = h[k] e^{+j theta k}   (the identity of SPEC §3.2 on x = (r, 0))
//
// fir_ddc_kernel: a WORKGROUP owns tiles of tile_out consecutive outputs <-> tile_out D inputs (+ K D - 1 inputs before them;
// the shape comes from ddc_shape, if_fir_ddc_plan.h).  Per tile: the real samples go through coalesced global loads into LDS
// (int16 converted on the way, samples before the call from the history buffer) DE-INTERLEAVED into D rows, window sample w in
// row w mod D, column w / D, four columns of a row per 16-byte LDS store.  Row R then holds, for the tile's output i, the
// samples of the taps rho = D - 1 - R, j = K - 1 .. 0 at the columns i .. i + K - 1: the kernel is D small FIRs of K taps over
// contiguous rows.  Lane t computes the DDC_R = 4 consecutive outputs 4 t .. 4 t + 3: it slides a register window along the row,
// one 16-byte LDS read (dense across the lanes: no bank conflict) per 4 taps = 16 packed FMAs on (re, im).  The taps are
// wave-uniform: read front to back from the table of ddc_build_table through the scalar cache.  A tile whose window lies
// inside the call is filled with plain loads, DDC_FILL items per lane in flight; the tiles at the ends of a call go through the
// bounds-checked stream_load_real (same values: the arithmetic does not know which filled its tile).
// Arithmetic per output (SPEC §10): rows R = 0 .. D - 1, in a row oldest sample first; segments of at most 16 taps from +0 (whole
// rows when K <= 16, else a row is cut), joined by the compensated addition of two_sum_add; then one rotation by the phasor of
// the output's own absolute index -- the same instructions whatever the tile, the lane or the call, so a stream cut anywhere
// gives the same bits.
// The first workgroup writes the next call's history into the other ping-pong buffer before anything else.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <mutex>
#include <type_traits>

#include "if_fir_ddc.h"
#include "if_fir_kernels.h"
#include "if_fir_stream_dev.h"

namespace if_fir
{

typedef float ddc_v4f __attribute__((ext_vector_type(4)));

// the K taps (a multiple of 4) of one row on the lane's DDC_R outputs: x = the lane's place in the row (16-byte aligned), tp =
// the row of the tap table.  CUT (a row of more than 16 taps): the segment is joined to the total and started again from +0
// after the tap `join` - 1 and then after every 16th, the last time after the row's last tap; otherwise the row adds to seg.
template <bool CUT>
__device__ __forceinline__ void ddc_row(const float *__restrict__ x, const float2 *__restrict__ tp, int K, int join, stream_v2f (&seg)[DDC_R],
                                        stream_v2f (&acc)[DDC_R], stream_v2f (&lost)[DDC_R])
{
    const int e0 = 0, e1 = K;
    ddc_v4f a = *reinterpret_cast<const ddc_v4f *>(x + e0), b = *reinterpret_cast<const ddc_v4f *>(x + e0 + 4);
    float2 t[4] = {tp[e0], tp[e0 + 1], tp[e0 + 2], tp[e0 + 3]};
    for (int e = e0; e < e1; e += 4)
    {
        // the next step's columns and taps are requested ahead of this step's 16 FMAs (the last step asks for its own again:
        // nothing is read beyond the row)
        const int en = e + 4 < e1 ? e + 4 : e;
        const ddc_v4f bn = *reinterpret_cast<const ddc_v4f *>(x + en + 4);
        const float2 tn[4] = {tp[en], tp[en + 1], tp[en + 2], tp[en + 3]};
        __builtin_amdgcn_sched_barrier(0); // (the scheduler would sink the requests down to their use)
        const float win[7] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z};
#pragma unroll
        for (int u = 0; u < 4; u++)
        {
            const stream_v2f g = {t[u].x, t[u].y};
#pragma unroll
            for (int i = 0; i < DDC_R; i++)
            {
                const stream_v2f s = {win[u + i], win[u + i]};
                seg[i] = __builtin_elementwise_fma(g, s, seg[i]);
            }
        }
        a = b;
        b = bn;
#pragma unroll
        for (int u = 0; u < 4; u++)
            t[u] = tn[u];
        if (CUT && e + 4 == join)
        {
#pragma unroll
            for (int i = 0; i < DDC_R; i++)
            {
                two_sum_add(acc[i], lost[i], seg[i]);
                seg[i] = stream_v2f{0.f, 0.f};
            }
            join += DDC_SEG;
        }
    }
}

constexpr int DDC_FILL = 4; // items (4 loads each) a lane has in flight while it fills an interior tile

// (single LDS reads, if_fir_stream_dev.h)
template <bool I16>
__global__ __launch_bounds__(DDC_THREADS) IF_FIR_SINGLE_READS void fir_ddc_kernel(const void *__restrict__ in, float2 *__restrict__ out,
                                                                const float *__restrict__ hist, float *__restrict__ hist_out,
                                                                const float2 *__restrict__ taps, int T, int D, int K, int G, int RS,
                                                                int tile_out, int n0, int64_t N, int64_t count, int64_t ntiles,
                                                                uint32_t nco_on, uint32_t phi0, uint32_t delta)
{
    using in_t = typename std::conditional<I16, short, float>::type;
    extern __shared__ __attribute__((aligned(16))) float ddc_xs[];
    float *xs = ddc_xs;
    const int tid = threadIdx.x;
    const int hist_len = T - 1;
    if (blockIdx.x == 0) // (its own loop: through a shared helper it compiles to other code, profiles/stream_plan_ab.txt)
        for (int i = tid; i < hist_len; i += DDC_THREADS)
            hist_out[i] = stream_load_real<I16>(in, hist, hist_len, N, N - hist_len + i);
    if ((int64_t)blockIdx.x >= ntiles)
        return; // (uniform per workgroup: a call without outputs only moves the history)
    const int quads = (tile_out + K) / 4, items = quads * D;
    const int64_t tile_in = (int64_t)tile_out * D;
    const bool mine = DDC_R * tid < tile_out;
    const float *xl = xs + DDC_R * tid;
    const int top = stream_top_segment(K); // (a long row's first segment: 4, 8, 12 or 16 taps)

    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x)
    {
        __syncthreads(); // the previous tile has been read
        const int64_t wfirst = (int64_t)n0 + tile * tile_in - ((int64_t)K * D - 1);
        if (wfirst >= 0 && wfirst + (int64_t)(tile_out + K) * D <= N)
        {
            // the whole window lies inside the call: plain loads, several items' worth in flight per lane (a load behind a
            // bounds check is waited for before the next one is asked for)
            const in_t *src = static_cast<const in_t *>(in) + wfirst;
            for (int q0 = tid; q0 < items; q0 += DDC_FILL * DDC_THREADS)
            {
                ddc_v4f v[DDC_FILL];
                int to[DDC_FILL];
#pragma unroll
                for (int u = 0; u < DDC_FILL; u++)
                {
                    // (past the last item: the last item again, loaded and not stored)
                    const int q = q0 + u * DDC_THREADS < items ? q0 + u * DDC_THREADS : items - 1;
                    const int cq = q / D, row = q - cq * D, at = 4 * cq * D + row;
                    v[u] = ddc_v4f{stream_sample_real<I16>(src, at), stream_sample_real<I16>(src, at + D), stream_sample_real<I16>(src, at + 2 * D),
                                   stream_sample_real<I16>(src, at + 3 * D)};
                    to[u] = row * RS + 4 * cq;
                }
#pragma unroll
                for (int u = 0; u < DDC_FILL; u++)
                    if (q0 + u * DDC_THREADS < items)
                        *reinterpret_cast<ddc_v4f *>(xs + to[u]) = v[u];
            }
        }
        else
            for (int q = tid; q < items; q += DDC_THREADS)
            {
                const int cq = q / D, row = q - cq * D;
                const int64_t p = wfirst + (int64_t)(4 * cq) * D + row;
                ddc_v4f v;
                v.x = stream_load_real<I16>(in, hist, hist_len, N, p);
                v.y = stream_load_real<I16>(in, hist, hist_len, N, p + D);
                v.z = stream_load_real<I16>(in, hist, hist_len, N, p + 2 * D);
                v.w = stream_load_real<I16>(in, hist, hist_len, N, p + 3 * D);
                *reinterpret_cast<ddc_v4f *>(xs + row * RS + 4 * cq) = v;
            }
        __syncthreads();
        if (!mine)
            continue; // (the barriers are at the head of the loop body: every lane reaches them)

        stream_v2f acc[DDC_R], lost[DDC_R], seg[DDC_R];
#pragma unroll
        for (int i = 0; i < DDC_R; i++)
            acc[i] = lost[i] = stream_v2f{0.f, 0.f};
        if (K <= DDC_SEG)
        {
            for (int r0 = 0; r0 < D; r0 += G)
            {
#pragma unroll
                for (int i = 0; i < DDC_R; i++)
                    seg[i] = stream_v2f{0.f, 0.f};
                const int r1 = r0 + G < D ? r0 + G : D;
                for (int r = r0; r < r1; r++)
                    ddc_row<false>(xl + r * RS, taps + r * K, K, 0, seg, acc, lost);
#pragma unroll
                for (int i = 0; i < DDC_R; i++)
                    two_sum_add(acc[i], lost[i], seg[i]);
            }
        }
        else
        {
#pragma unroll
            for (int i = 0; i < DDC_R; i++)
                seg[i] = stream_v2f{0.f, 0.f};
            for (int r = 0; r < D; r++) // (a row ends on a join: seg is +0 again for the next one)
                ddc_row<true>(xl + r * RS, taps + r * K, K, top, seg, acc, lost);
        }
        const int64_t obase = tile * tile_out + DDC_R * tid;
#pragma unroll
        for (int i = 0; i < DDC_R; i++)
        {
            const int64_t o = obase + i;
            stream_v2f v = acc[i] + lost[i];
            if (nco_on)
            {
                // the phase of the output's own absolute index: -(P a) mod 2^32, a = abs0 + o D
                const float2 w = nco_phasor(phi0 + (uint32_t)o * delta);
                v = stream_v2f{fmaf(v.x, w.x, -v.y * w.y), fmaf(v.x, w.y, v.y * w.x)};
            }
            if (o < count)
                out[o] = make_float2(v.x, v.y);
        }
    }
}

template <bool I16>
static hipError_t launch_t(const DdcArgs &a)
{
    int cus = 0;
    const hipError_t e = stream_kernel_setup<&fir_ddc_kernel<I16>>(a.device, DDC_LDS_MAX, &cus);
    if (e != hipSuccess)
        return e;
    const DdcShape s = ddc_shape(a.T, a.D);
    const int64_t ntiles = (a.count + s.tile_out - 1) / s.tile_out;
    // a grid-stride loop over the tiles on as many workgroups as are resident at a time (2 per CU with a 64 KB window, up to
    // 8 with small ones); at least one, which writes the history
    const unsigned groups = stream_persistent_groups(cus, ddc_groups_per_cu(s, a.D), ntiles, a.grid_limit);
    hipLaunchKernelGGL((fir_ddc_kernel<I16>), dim3(groups), dim3(DDC_THREADS), ddc_lds_bytes(s, a.D), a.stream, a.in,
                       static_cast<float2 *>(a.out), a.hist, a.hist_out, reinterpret_cast<const float2 *>(a.taps), a.T, a.D, s.K, s.G, s.RS,
                       s.tile_out, a.n0, a.N, a.count, ntiles, a.nco_word != 0 ? 1u : 0u, 0u - a.nco_word * a.nco_abs0,
                       0u - a.nco_word * (uint32_t)a.D);
    return hipGetLastError();
}

hipError_t launch_ddc(const DdcArgs &a)
{
    if (a.T < 1 || a.T > DDC_MAX_TAPS || a.D < 1 || a.D > DDC_MAX_D || a.N < 1 || a.count < 0 || a.n0 < 0 || a.n0 >= a.D)
        return hipErrorInvalidValue;
    return a.in_i16 ? launch_t<true>(a) : launch_t<false>(a);
}

} // namespace if_fir
