// if_fir_interp.hip — interpolate-by-L FIR with a fused NCO up-mix for gfx950 (docs/SPEC.md §6).
//
//   u[n] = x[n/L] (n mod L == 0, else 0),   y[n] = sum_k h[k] u[n-k],   y'[n] = exp(+j 2 pi P n / 2^32) y[n]
//
// fir_interp_kernel (overlap-save, L | 64, T <= 3073): one WORKGROUP = one block of 4096 output-rate points in LDS.  The
// block starts OVL = 64 ROWS outputs before the first output it keeps and advances A = 4096 - OVL outputs = A/L inputs;
// L divides 64, so every block starts on an input sample.
//   small form (L >= 4)  load the block's 4096/L input samples, 4096/L-point forward transform; the transform of the
//                        zero-stuffed block is that one repeated L times, so the multiply by H reads it modulo 4096/L
//   full form (any L)    load the zero-stuffed block, 4096-point forward transform (the small form's cross-check)
// then Z = H X (fused into the first inverse pass), the 4096-point inverse, and the store of positions OVL..4095 fused
// into the last inverse pass (rotated by the NCO).  Transforms: radix-4 Stockham passes (one radix-2 pass first when the
// size is an odd power of 2) with the twiddles W4096^i from a table; index algebra in tools/fft_model.py (interp_block).
// fir_interp_generic_kernel: one output per thread, all the taps of its phase; any L, any T (the slow cross-check).
//
// Build: compiled once per overlap length (-DIF_FIR_INTERP_ROWS=4|8|16|32|48, the overlap-save instantiations and their
// launcher) and once without (host tables, routing, the generic kernel).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>

#include "if_fir_interp.h"
#include "if_fir_interp_dev.h"
#include "if_fir_kernels.h"

namespace if_fir
{

// the next call's history = the last hist_len samples of (history || input), converted to float32; written by workgroup 0
// into the other ping-pong buffer (everything it reads is read-only during the launch)
template <bool I16>
__device__ __forceinline__ void ip_write_history(const void *__restrict__ in, const float2 *__restrict__ hist, float2 *__restrict__ hist_out,
                                                 int hist_len, int64_t N)
{
    if (blockIdx.x == 0 && hist_out)
        ip_history<I16>(in, hist, hist_out, hist_len, N);
}

#if !defined(IF_FIR_INTERP_ROWS) // ================= host side + the generic kernel =================

bool interp_fft_supported(int T, int L)
{
    return T >= 1 && T <= INTERP_FFT_MAX_TAPS && L >= 1 && L <= INTERP_MAX_L && (64 % L) == 0;
}

int interp_overlap_rows(int T)
{
    const int rows[] = {4, 8, 16, 32, 48};
    for (int r : rows)
        if (64 * r >= T - 1)
            return r;
    return 48;
}

int interp_hist_len(int T, int L)
{
    // the overlap-save kernel reads OVL / L samples before a block; the generic kernel ceil((T - 1) / L): one length serves both
    const int ovl = T <= INTERP_FFT_MAX_TAPS ? 64 * interp_overlap_rows(T) : T - 1;
    return (ovl + L - 1) / L;
}

void interp_build_tables(const float *taps, int T, int ctaps, float2 *H, float2 *tw)
{
    double c[INTERP_N], s[INTERP_N];
    for (int i = 0; i < INTERP_N; i++)
    {
        c[i] = cos(2.0 * M_PI * i / INTERP_N);
        s[i] = -sin(2.0 * M_PI * i / INTERP_N);
        tw[i] = make_float2((float)c[i], (float)s[i]);
    }
    for (int k = 0; k < INTERP_N; k++)
    {
        double re = 0.0, im = 0.0;
        for (int t = 0; t < T; t++)
        {
            const double hr = ctaps ? taps[2 * t] : taps[t], hi = ctaps ? taps[2 * t + 1] : 0.0;
            const int e = (int)(((int64_t)k * t) & (INTERP_N - 1));
            re += hr * c[e] - hi * s[e];
            im += hr * s[e] + hi * c[e];
        }
        H[k] = make_float2((float)(re / INTERP_N), (float)(im / INTERP_N));
    }
}

hipError_t launch_interp_fft(const InterpArgs &a)
{
    if (!interp_fft_supported(a.T, a.L) || !a.H || !a.tw)
        return hipErrorInvalidConfiguration;
    switch (interp_overlap_rows(a.T))
    {
    case 4: return launch_interp_fft_rows<4>(a);
    case 8: return launch_interp_fft_rows<8>(a);
    case 16: return launch_interp_fft_rows<16>(a);
    case 32: return launch_interp_fft_rows<32>(a);
    default: return launch_interp_fft_rows<48>(a);
    }
}

template <bool I16, bool CT, bool NCO>
__global__ __launch_bounds__(INTERP_THREADS) void fir_interp_generic_kernel(const void *__restrict__ in, float2 *__restrict__ out,
                                                                           const float2 *__restrict__ hist, float2 *__restrict__ hist_out,
                                                                           int hist_len, const float *__restrict__ taps, int T, int L,
                                                                           int64_t N, int64_t M, uint32_t nco_word, uint32_t nco_phi0)
{
    ip_write_history<I16>(in, hist, hist_out, hist_len, N);
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < M; i += stride)
    {
        float2 y = ip_phase_sum<I16, CT>(in, hist, hist_len, taps, T, L, N, i);
        if constexpr (NCO)
            y = ip_cmul(y, nco_phasor(nco_phi0 + nco_word * (uint32_t)i));
        out[i] = y;
    }
}

template <bool I16, bool CT, bool NCO>
static hipError_t launch_generic_t(const InterpArgs &a)
{
    const unsigned groups = stream_generic_groups(a.M, INTERP_THREADS, a.grid_limit);
    hipLaunchKernelGGL((fir_interp_generic_kernel<I16, CT, NCO>), dim3(groups), dim3(INTERP_THREADS), 0, a.stream, a.in,
                       static_cast<float2 *>(a.out), a.hist, a.hist_out, a.hist_len, a.taps, a.T, a.L, a.N, a.M, a.nco_word,
                       a.nco_phi0);
    return hipGetLastError();
}

hipError_t launch_interp_generic(const InterpArgs &a)
{
    const bool nco = a.nco_word != 0;
    if (a.in_i16)
    {
        if (a.ctaps)
            return nco ? launch_generic_t<true, true, true>(a) : launch_generic_t<true, true, false>(a);
        return nco ? launch_generic_t<true, false, true>(a) : launch_generic_t<true, false, false>(a);
    }
    if (a.ctaps)
        return nco ? launch_generic_t<false, true, true>(a) : launch_generic_t<false, true, false>(a);
    return nco ? launch_generic_t<false, false, true>(a) : launch_generic_t<false, false, false>(a);
}

#else // ================= overlap-save kernel: one unit per overlap length =================

// (single ds_read_b64 LDS reads, like the decimator's overlap-save units)
template <int OVL_ROWS, bool I16, bool NCO, bool SMALL>
__global__ __launch_bounds__(INTERP_THREADS, 2) IF_FIR_SINGLE_READS void fir_interp_kernel(
    const void *__restrict__ in, float2 *__restrict__ out, const float2 *__restrict__ hist, float2 *__restrict__ hist_out, int hist_len,
    const float2 *__restrict__ H, const float2 *__restrict__ tw, int L, int64_t N, int64_t M, int64_t nblocks, uint32_t nco_word,
    uint32_t nco_phi0)
{
    constexpr int OVL = 64 * OVL_ROWS;
    constexpr int A = INTERP_N - OVL; // kept outputs per block
    __shared__ float2 buf[INTERP_N];
    ip_write_history<I16>(in, hist, hist_out, hist_len, N);
    const int nf = SMALL ? INTERP_N / L : INTERP_N; // forward transform size
    const int a_in = A / L;                          // input samples per block advance
    const int ovl_in = OVL / L;
    auto lds = [&](int i) -> float2 { return buf[i]; };
    auto to_lds = [&](int i, float2 v) { buf[i] = v; };
    for (int64_t b = blockIdx.x; b < nblocks; b += gridDim.x)
    {
        const int64_t j0 = b * a_in - ovl_in; // input index of the block's first point
        const int64_t o0 = b * A - OVL;       // output index of the block's first point
        // ---- the block's input into LDS (the full form zero-stuffed), then the forward transform ----
        for (int p = threadIdx.x; p < nf; p += INTERP_THREADS)
        {
            if (SMALL)
                buf[p] = ip_load<I16>(in, hist, hist_len, N, j0 + p);
            else
                buf[p] = (p & (L - 1)) == 0 ? ip_load<I16>(in, hist, hist_len, N, j0 + p / L) : make_float2(0.f, 0.f);
        }
        __syncthreads();
        // (ip_forward of if_fir_interp_dev.h written out: through the function the small form's kernels compile differently and
        // measured 0.4 - 1.2 % slower at L = 4, 8, 16 -- profiles/r11_stream_dev_ab.txt)
        int ns = 1;
        if (nf & 0x2aaa) // log2(nf) odd: one radix-2 pass first
        {
            ip_pass<2, false>(nf, ns, tw, lds, to_lds);
            ns = 2;
        }
#pragma unroll 1
        for (; ns < nf; ns *= 4)
            ip_pass<4, false>(nf, ns, tw, lds, to_lds);
        // ---- Z = H X (X read modulo nf), fused into the first inverse pass; 1/4096 is in H ----
        auto zsrc = [&](int k) -> float2 { return ip_cmul(H[(unsigned)k], buf[k & (nf - 1)]); };
        ip_pass<4, true>(INTERP_N, 1, tw, zsrc, to_lds);
        ip_inverse_mid(tw, lds, to_lds);
        // ---- last inverse pass: positions OVL..4095 straight to the outputs (rotated by the NCO); beyond M dropped ----
        float2 *ob = out + o0;                                  // (wave-uniform base: 32-bit offsets below)
        const int pend = M - o0 < INTERP_N ? (int)(M - o0) : INTERP_N; // positions past the last output are dropped
        const uint32_t phb = nco_phi0 + nco_word * (uint32_t)o0;
        auto store = [&](int p, float2 v) {
            if (p >= OVL && p < pend)
            {
                if constexpr (NCO)
                    v = ip_cmul(v, nco_phasor(phb + nco_word * (uint32_t)p));
                ob[(unsigned)p] = v;
            }
        };
        ip_pass<4, true>(INTERP_N, INTERP_N / 4, tw, lds, store);
    }
}

template <int ROWS, bool I16, bool NCO, bool SMALL>
static hipError_t launch_t(const InterpArgs &a, int64_t nblocks, unsigned groups)
{
    hipLaunchKernelGGL((fir_interp_kernel<ROWS, I16, NCO, SMALL>), dim3(groups), dim3(INTERP_THREADS), 0, a.stream, a.in,
                       static_cast<float2 *>(a.out), a.hist, a.hist_out, a.hist_len, a.H, a.tw, a.L, a.N, a.M, nblocks, a.nco_word,
                       a.nco_phi0);
    return hipGetLastError();
}

template <int ROWS>
hipError_t launch_interp_fft_rows(const InterpArgs &a)
{
    int64_t nblocks;
    unsigned g;
    const hipError_t e = ip_fft_grid(a.device, a.M, INTERP_N - 64 * ROWS, a.grid_limit, &nblocks, &g);
    if (e != hipSuccess)
        return e;
    const bool small = !a.full && a.L >= 4;
    const bool nco = a.nco_word != 0;
#define IP_LAUNCH(I16, NCO)                                                                                              \
    return small ? launch_t<ROWS, I16, NCO, true>(a, nblocks, g) : launch_t<ROWS, I16, NCO, false>(a, nblocks, g)
    if (a.in_i16)
    {
        if (nco)
            IP_LAUNCH(true, true);
        IP_LAUNCH(true, false);
    }
    if (nco)
        IP_LAUNCH(false, true);
    IP_LAUNCH(false, false);
#undef IP_LAUNCH
}

template hipError_t launch_interp_fft_rows<IF_FIR_INTERP_ROWS>(const InterpArgs &a);

#endif // IF_FIR_INTERP_ROWS

} // namespace if_fir
