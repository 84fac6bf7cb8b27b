// if_fir_combiner.hip — channel combiner for gfx950 (docs/SPEC.md §9): C baseband streams, each interpolated
// by L with one prototype filter and mixed up to its own centre, summed into one stream in one pass.
//
//   u_c[n] = x_c[n/L] (n mod L == 0, else 0),   y[n] = sum_c exp(+j 2 pi P_c n / 2^32) sum_k h[k] u_c[n-k]
//
// fir_combiner_kernel (overlap-save, L in {4, ..., 64}, T <= 3073): the interpolator's block geometry (if_fir_interp.hip: one
// WORKGROUP = one block of 4096 output-rate points, overlap OVL = 64 ROWS, small form).  With P = G 2^20 + r (G = the nearest
// point of the 1/4096 grid, |r| <= 2^19) and theta_x = 2 pi x / 2^32
//   exp(j theta_P n) sum_k h[k] u[n-k] = exp(j 2 pi G n / 4096) sum_k (h[k] exp(j theta_r k)) (u[n-k] exp(j theta_r (n-k)))
// so per block and channel: load the 4096/L input samples rotated by the residual r at their absolute output index (and by the
// block's scalar exp(j 2 pi G n0 / 4096), n0 = the block's first point: everything after is linear), the 4096/L-point forward
// transform, times the table of the prototype rotated by r read modulo 4096/L, moved by G bins, ADDED to the sums a thread
// keeps in registers for its 16 bins.  After the last channel: one 4096-point inverse and one store of positions OVL..4095.
// fir_combiner_generic_kernel: one output per thread, all the taps of its phase for every channel, channels in ascending
// order; any L, T, C (the slow cross-check).
//
// Build: compiled once per overlap length (-DIF_FIR_COMBINER_ROWS=4|8|16|32|48, the overlap-save instantiations and their
// launcher) and once without (host tables, routing, the generic kernel), like the interpolator.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>
#include <vector>

#include "if_fir_combiner.h"
#include "if_fir_interp_dev.h"
#include "if_fir_kernels.h"

namespace if_fir
{

// the next call's history of every channel = the last hist_len samples of (history || input), converted to float32; written by
// workgroup 0 into the other ping-pong buffer (everything it reads is read-only during the launch)
template <bool I16>
__device__ __forceinline__ void cb_write_history(const CombinerChans &ch, int C, const float2 *__restrict__ hist,
                                                 float2 *__restrict__ hist_out, int hist_len, int64_t N)
{
    if (blockIdx.x != 0 || !hist_out)
        return;
    for (int c = 0; c < C; c++)
        ip_history<I16>(ch.in[c], hist + c * hist_len, hist_out + c * hist_len, hist_len, N);
}

#if !defined(IF_FIR_COMBINER_ROWS) // ================= host side + the generic kernel =================

bool combiner_fft_supported(int T, int L)
{
    return L >= 4 && interp_fft_supported(T, L);
}

void combiner_build_table(const float *taps, int T, int ctaps, int32_t r, float2 *H)
{
    if (r == 0)
    {
        // a channel on the 1/4096 grid: the interpolator's H
        std::vector<float2> tw(INTERP_N);
        interp_build_tables(taps, T, ctaps, H, tw.data());
        return;
    }
    static_assert(COMBINER_TABLE_N == INTERP_N, "one block size");
    combiner_residual_table(taps, T, ctaps, r, reinterpret_cast<float *>(H));
}

hipError_t launch_combiner_fft(const CombinerArgs &a)
{
    if (!combiner_fft_supported(a.T, a.L) || !a.H || !a.tw || a.C < 1 || a.C > COMBINER_MAX_CHANNELS)
        return hipErrorInvalidConfiguration;
    switch (interp_overlap_rows(a.T))
    {
    case 4: return launch_combiner_fft_rows<4>(a);
    case 8: return launch_combiner_fft_rows<8>(a);
    case 16: return launch_combiner_fft_rows<16>(a);
    case 32: return launch_combiner_fft_rows<32>(a);
    default: return launch_combiner_fft_rows<48>(a);
    }
}

template <bool I16, bool CT>
__global__ __launch_bounds__(INTERP_THREADS) void fir_combiner_generic_kernel(const CombinerChans ch, int C, float2 *__restrict__ out,
                                                                             const float2 *__restrict__ hist, float2 *__restrict__ hist_out,
                                                                             int hist_len, const float *__restrict__ taps, int T, int L,
                                                                             int64_t N, int64_t M, uint32_t first_out)
{
    cb_write_history<I16>(ch, C, hist, hist_out, hist_len, N);
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < M; i += stride)
    {
        // per channel as fir_interp_generic_kernel; the channels are added the same way (two-sum), in ascending order
        const uint32_t n32 = first_out + (uint32_t)i;
        float yr = 0.f, yi = 0.f, er = 0.f, ei = 0.f;
        for (int c = 0; c < C; c++)
        {
            float2 y = ip_phase_sum<I16, CT>(ch.in[c], hist + c * hist_len, hist_len, taps, T, L, N, i);
            const uint32_t word = ((uint32_t)ch.G[c] << 20) + ch.rword[c];
            if (word)
                y = ip_cmul(y, nco_phasor(word * n32));
            two_sum_add(yr, er, y.x);
            two_sum_add(yi, ei, y.y);
        }
        out[i] = make_float2(yr + er, yi + ei);
    }
}

template <bool I16, bool CT>
static hipError_t launch_generic_t(const CombinerArgs &a)
{
    const unsigned groups = stream_generic_groups(a.M, INTERP_THREADS, a.grid_limit);
    hipLaunchKernelGGL((fir_combiner_generic_kernel<I16, CT>), dim3(groups), dim3(INTERP_THREADS), 0, a.stream, a.ch, a.C,
                       static_cast<float2 *>(a.out), a.hist, a.hist_out, a.hist_len, a.taps, a.T, a.L, a.N, a.M, a.first_out);
    return hipGetLastError();
}

hipError_t launch_combiner_generic(const CombinerArgs &a)
{
    if (a.C < 1 || a.C > COMBINER_MAX_CHANNELS || !a.taps)
        return hipErrorInvalidConfiguration;
    if (a.in_i16)
        return a.ctaps ? launch_generic_t<true, true>(a) : launch_generic_t<true, false>(a);
    return a.ctaps ? launch_generic_t<false, true>(a) : launch_generic_t<false, false>(a);
}

#else // ================= overlap-save kernel: one unit per overlap length =================

// (single ds_read_b64 LDS reads, like the interpolator's units)
template <int OVL_ROWS, bool I16>
__global__ __launch_bounds__(INTERP_THREADS, 2) IF_FIR_SINGLE_READS void fir_combiner_kernel(
    const CombinerChans ch, int C, float2 *__restrict__ out, const float2 *__restrict__ hist, float2 *__restrict__ hist_out, int hist_len,
    const float2 *__restrict__ H, const float2 *__restrict__ tw, int L, int64_t N, int64_t M, int64_t nblocks, uint32_t first_out)
{
    constexpr int OVL = 64 * OVL_ROWS;
    constexpr int A = INTERP_N - OVL;                 // kept outputs per block
    constexpr int Q = INTERP_N / 4 / INTERP_THREADS;  // a thread's bins: k = t + q 256 + r 1024, the inputs of its first inverse butterflies
    __shared__ float2 buf[INTERP_N];
    cb_write_history<I16>(ch, C, hist, hist_out, hist_len, N);
    const int nf = INTERP_N / L; // forward transform size
    const int a_in = A / L;      // input samples per block advance
    const int ovl_in = OVL / L;
    auto lds = [&](int i) -> float2 { return buf[i]; };
    auto to_lds = [&](int i, float2 v) { buf[i] = v; };
    for (int64_t b = blockIdx.x; b < nblocks; b += gridDim.x)
    {
        const int64_t j0 = b * a_in - ovl_in;              // input index of the block's first point
        const int64_t o0 = b * A - OVL;                    // output index of the block's first point
        const uint32_t n0 = first_out + (uint32_t)o0;      // its absolute output index mod 2^32
        float2 acc[Q][4];
#pragma unroll
        for (int q = 0; q < Q; q++)
#pragma unroll
            for (int r = 0; r < 4; r++)
                acc[q][r] = make_float2(0.f, 0.f);
#pragma unroll 1
        for (int c = 0; c < C; c++)
        {
            const void *in = ch.in[c];
            const float2 *hc = hist + c * hist_len;
            const uint32_t rw = ch.rword[c];
            const int G = ch.G[c];
            const float2 *Hc = H + (size_t)ch.table[c] * INTERP_N;
            // ---- the block's input into LDS, rotated by exp(j 2 pi G n0 / 4096) exp(j theta_r n), then the forward transform ----
            float2 s = tw[(unsigned)(G * (int)(n0 & (INTERP_N - 1))) & (INTERP_N - 1)];
            s.y = -s.y; // the table holds exp(-j ...)
            for (int p = threadIdx.x; p < nf; p += INTERP_THREADS)
            {
                const float2 x = ip_load<I16>(in, hc, hist_len, N, j0 + p);
                const float2 w = rw ? ip_cmul(s, nco_phasor(rw * (n0 + (uint32_t)(p * L)))) : s;
                buf[p] = ip_cmul(x, w);
            }
            __syncthreads();
            ip_forward(nf, tw, lds, to_lds);
            // ---- Z_c = H_r X_c (X_c read modulo nf) moved by G bins, added to the sums; 1/4096 is in H_r ----
#pragma unroll
            for (int q = 0; q < Q; q++)
#pragma unroll
                for (int r = 0; r < 4; r++)
                {
                    const int k = ((int)threadIdx.x + q * INTERP_THREADS + r * (INTERP_N / 4) - G) & (INTERP_N - 1);
                    const float2 z = ip_cmul(Hc[(unsigned)k], buf[k & (nf - 1)]);
                    acc[q][r].x += z.x;
                    acc[q][r].y += z.y;
                }
            __syncthreads(); // the next channel's input overwrites buf
        }
        // ---- the first inverse pass (ns = 1: no twiddles) from the registers: input j + r 1024 -> position 4 j + r ----
#pragma unroll
        for (int q = 0; q < Q; q++)
        {
            const int j = (int)threadIdx.x + q * INTERP_THREADS;
            ip_bfly<4, true>(acc[q]);
#pragma unroll
            for (int r = 0; r < 4; r++)
                buf[4 * j + r] = acc[q][r];
        }
        __syncthreads();
        ip_inverse_mid(tw, lds, to_lds);
        // ---- last inverse pass: positions OVL..4095 straight to the outputs; beyond M dropped ----
        float2 *ob = out + o0;                                        // (wave-uniform base: 32-bit offsets below)
        const int pend = M - o0 < INTERP_N ? (int)(M - o0) : INTERP_N; // positions past the last output are dropped
        auto store = [&](int p, float2 v) {
            if (p >= OVL && p < pend)
                ob[(unsigned)p] = v;
        };
        ip_pass<4, true>(INTERP_N, INTERP_N / 4, tw, lds, store);
    }
}

template <int ROWS>
hipError_t launch_combiner_fft_rows(const CombinerArgs &a)
{
    int64_t nblocks;
    unsigned groups;
    const hipError_t e = ip_fft_grid(a.device, a.M, INTERP_N - 64 * ROWS, a.grid_limit, &nblocks, &groups);
    if (e != hipSuccess)
        return e;
    if (a.in_i16)
        hipLaunchKernelGGL((fir_combiner_kernel<ROWS, true>), dim3(groups), dim3(INTERP_THREADS), 0, a.stream, a.ch, a.C,
                           static_cast<float2 *>(a.out), a.hist, a.hist_out, a.hist_len, a.H, a.tw, a.L, a.N, a.M, nblocks, a.first_out);
    else
        hipLaunchKernelGGL((fir_combiner_kernel<ROWS, false>), dim3(groups), dim3(INTERP_THREADS), 0, a.stream, a.ch, a.C,
                           static_cast<float2 *>(a.out), a.hist, a.hist_out, a.hist_len, a.H, a.tw, a.L, a.N, a.M, nblocks, a.first_out);
    return hipGetLastError();
}

template hipError_t launch_combiner_fft_rows<IF_FIR_COMBINER_ROWS>(const CombinerArgs &a);

#endif // IF_FIR_COMBINER_ROWS

} // namespace if_fir
