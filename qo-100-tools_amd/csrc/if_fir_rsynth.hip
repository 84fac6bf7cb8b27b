// if_fir_rsynth.hip — real-output polyphase synthesis bank: the M/2 + 1 distinct channels of a grid to one REAL stream in one
// pass, for gfx950 (docs/SPEC.md §18).
//
//   y[n] = sum_{j<J} h[t_j] v_{m_j}[n mod M],   m_j = floor(n / L) - j,  t_j = (n mod L) + j L,  terms with t_j >= T skipped
//   v_m[s] = Re X_0 + (-1)^s Re X_H + 2 sum_{0<k<H} Re( X_k e^{+j 2 pi k s / M} ),   H = M / 2:  REAL, so z[n] = v[2n] + j v[2n+1]
//   is the inverse H-point transform of Z_k = (X_k + conj X_{H-k}) + j W^k (X_k - conj X_{H-k}), W = e^{+j 2 pi / M}
//
// A call is cut into chunks of a device workspace (if_fir_synth_plan.h's chunking, rows of M floats); per chunk, on the
// context's stream:
// rsynth_transform_kernel<M, I16>: a workgroup takes B = rsynth_batch(M) consecutive frames of (history || call) at a time
// (B H >= 1024 points).  Lane item (frame, k), k = 0 .. H/2, loads channels k and H - k of its frame (coalesced global loads
// along the span, the second running backwards; int16 converted on the way, frames before the call from the carried history,
// channels outside the span +0), takes W^k from the L2-resident table (coalesced along k, the same H/2 + 1 entries for every
// frame) and writes Z_k and Z_{H-k} to LDS slots k and H - k, both runs of consecutive 8-byte slots: rpfb's untangling pass in
// reverse.
// Then the in-place FORWARD transform of if_fir_lds_fft_dev.h over all B blocks of H points at once, and z[n] leaves for the
// workspace from place psd_bin_position((H - n) mod H, H), coalesced along n: float2 n of a row is (v[2n], v[2n+1]).
// rsynth_emit_kernel<O16>: one real output per lane, coalesced along n: the chain acc = fma(h[t_j], v_{m_j}[n mod M], acc),
// j = 0 .. J-1 (newest frame first), from the workspace and the tap table; stored as float32 or as SPEC §11's int16.
// rsynth_carry_kernel (once per call): the last J - 1 input frames of (history || call) go to the other ping-pong buffer as float32.
// Every frame is transformed on its own, and an output's arithmetic depends on its J frames, the taps and n mod M only -- not on
// the call, the chunk, the batch or the workgroup -- so a stream cut anywhere gives the same bits.  The kernels see
// call-relative positions and (c L) mod M, never c.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "if_fir_duc_plan.h" // duc_to_i16: SPEC §11's int16 rule
#include "if_fir_kernels.h"
#include "if_fir_lds_fft_dev.h"
#include "if_fir_rsynth.h"
#include "if_fir_stream_dev.h"

namespace if_fir
{

// rows [0, rows) of `work` receive the transforms of the call's frames frame0 .. frame0 + rows - 1 (frame0 may be negative)
template <int M, bool I16>
__global__ __launch_bounds__(RSYNTH_THREADS) IF_FIR_SINGLE_READS void rsynth_transform_kernel(
    const void *__restrict__ in, const float2 *__restrict__ hist, const float2 *__restrict__ twiddle, const uint16_t *__restrict__ place,
    const float2 *__restrict__ pretangle, float *__restrict__ work, int first_bin, int bins, int64_t hist_len, int64_t n, int64_t frame0,
    int64_t rows, int64_t batches)
{
    constexpr int H = M / 2, B = (int)rsynth_batch(M), TOTAL = B * H, P = (int)rsynth_pair_items(M);
    extern __shared__ __attribute__((aligned(16))) char smem[];
    stream_v2f *x = reinterpret_cast<stream_v2f *>(smem);
    stream_v2f *tw = x + TOTAL;
    uint16_t *where = reinterpret_cast<uint16_t *>(tw + H);
    const int tid = threadIdx.x;
    for (int e = tid; e < H; e += RSYNTH_THREADS)
    {
        const float2 t = twiddle[e];
        tw[e] = stream_v2f{t.x, t.y};
        where[e] = place[e];
    }

    for (int64_t g = blockIdx.x; g < batches; g += gridDim.x)
    {
        const int64_t r0 = g * B;
        __syncthreads(); // the previous batch has been stored (and, the first time, the tables are staged)
        for (int e = tid; e < B * P; e += RSYNTH_THREADS)
        {
            const int fb = B == 1 ? 0 : e / P, k = e - fb * P;
            // channels k and H - k of the frame: elements k - first_bin and H - k - first_bin of the span, where it holds them
            const int ja = k - first_bin, jb = H - k - first_bin;
            stream_v2f a = {0.f, 0.f}, b = {0.f, 0.f};
            if (r0 + fb < rows)
            {
                const int64_t base = (frame0 + r0 + fb) * bins;
                if (ja >= 0 && ja < bins)
                    a = stream_load<I16>(in, hist, hist_len, n, base + ja);
                if (jb >= 0 && jb < bins)
                    b = stream_load<I16>(in, hist, hist_len, n, base + jb);
            }
            if (k == 0) // channels 0 and H count by their real parts alone
                a.y = b.y = 0.f;
            const float2 wk = pretangle[k];
            const stream_v2f w = {wk.x, wk.y};
            stream_v2f *z = x + fb * H;
            {
                const stream_v2f ev = {a.x + b.x, a.y - b.y}, d = {a.x - b.x, a.y + b.y};
                const stream_v2f p = lds_fft_cmul(d, w);
                z[k] = stream_v2f{ev.x - p.y, ev.y + p.x};
            }
            if (k != 0 && 2 * k != H)
            {
                // Z_{H-k}: the roles of the two channels swapped, W^{H-k} = -conj W^k
                const stream_v2f ev = {b.x + a.x, b.y - a.y}, d = {b.x - a.x, b.y + a.y};
                const stream_v2f p = lds_fft_cmul(d, stream_v2f{-w.x, w.y});
                z[H - k] = stream_v2f{ev.x - p.y, ev.y + p.x};
            }
        }
        __syncthreads();
        lds_fft_passes<TOTAL, H, H, RSYNTH_THREADS>(x, tw, tid);
        const int nb = rows - r0 < B ? (int)(rows - r0) : B;
        float2 *dst = reinterpret_cast<float2 *>(work + (size_t)r0 * M);
        for (int e = tid; e < nb * H; e += RSYNTH_THREADS)
        {
            const int fb = B == 1 ? 0 : e / H;
            const stream_v2f v = x[fb * H + where[e - fb * H]];
            dst[e] = make_float2(v.x, v.y);
        }
    }
}

// output i of the chunk, i < count = frames L: frame f = i / L of the chunk has its transform in row f + J - 1 of `work`
template <bool O16>
__global__ __launch_bounds__(RSYNTH_THREADS) void rsynth_emit_kernel(const float *__restrict__ work, const float *__restrict__ taps,
                                                                      void *__restrict__ out, int M, int T, int J, int L, uint32_t smod,
                                                                      uint32_t count)
{
    for (uint32_t i = blockIdx.x * RSYNTH_THREADS + threadIdx.x; i < count; i += gridDim.x * RSYNTH_THREADS)
    {
        const uint32_t f = i / (uint32_t)L, p = i - f * (uint32_t)L;
        const uint32_t s = (smod + i) & (uint32_t)(M - 1);
        const float *v = work + (size_t)(f + J - 1) * M + s;
        float acc = 0.f;
#pragma unroll 4
        for (int j = 0; j < J; j++)
        {
            const int t = (int)p + j * L;
            if (t < T)
                acc = fmaf(taps[t], v[-(ptrdiff_t)j * M], acc);
        }
        if constexpr (O16)
            static_cast<int16_t *>(out)[i] = duc_to_i16(acc);
        else
            static_cast<float *>(out)[i] = acc;
    }
}

template <bool I16>
__global__ __launch_bounds__(RSYNTH_THREADS) void rsynth_carry_kernel(const void *__restrict__ in, const float2 *__restrict__ hist,
                                                                      float2 *__restrict__ hist_out, int64_t hist_len, int64_t n)
{
    // the last hist_len elements of (hist || call)
    for (int64_t i = (int64_t)blockIdx.x * RSYNTH_THREADS + threadIdx.x; i < hist_len; i += (int64_t)gridDim.x * RSYNTH_THREADS)
    {
        const stream_v2f v = stream_load<I16>(in, hist, hist_len, n, n - hist_len + i);
        hist_out[i] = make_float2(v.x, v.y);
    }
}

template <int M, bool I16, bool O16>
static hipError_t launch_chunks(const RsynthArgs &a)
{
    int cus = 0;
    constexpr int lds = (int)rsynth_lds_bytes(M), B = (int)rsynth_batch(M);
    const hipError_t e = stream_kernel_setup<&rsynth_transform_kernel<M, I16>>(a.device, lds, &cus);
    if (e != hipSuccess)
        return e;
    const int64_t hist_len = (int64_t)(a.J - 1) * a.bins, n = a.frames * a.bins;
    const uint64_t per_chunk = synth_even_chunk_frames((uint64_t)a.frames, synth_chunk_frames(a.work_frames, (uint32_t)a.J)),
                   chunks = synth_chunks((uint64_t)a.frames, per_chunk);
    for (uint64_t i = 0; i < chunks; i++)
    {
        const SynthChunk ch = synth_chunk(i, (uint64_t)a.frames, per_chunk, (uint32_t)M, (uint32_t)a.L, a.call.smod);
        const int64_t rows = (int64_t)ch.frames + a.J - 1, batches = (rows + B - 1) / B;
        const unsigned groups = stream_persistent_groups(cus, rsynth_groups_per_cu(M), batches, a.grid_limit);
        hipLaunchKernelGGL((rsynth_transform_kernel<M, I16>), dim3(groups), dim3(RSYNTH_THREADS), lds, a.stream, a.in, a.hist, a.twiddle,
                           a.place, a.pretangle, a.work, a.first_bin, a.bins, hist_len, n, (int64_t)ch.first - (a.J - 1), rows, batches);
        hipError_t le = hipGetLastError();
        if (le != hipSuccess)
            return le;
        const uint32_t count = (uint32_t)(ch.frames * (uint64_t)a.L);
        const size_t first_out = (size_t)ch.first * (size_t)a.L;
        void *out = O16 ? (void *)(static_cast<int16_t *>(a.out) + first_out) : (void *)(static_cast<float *>(a.out) + first_out);
        hipLaunchKernelGGL((rsynth_emit_kernel<O16>), dim3(stream_generic_groups(count, RSYNTH_THREADS, a.grid_limit)),
                           dim3(RSYNTH_THREADS), 0, a.stream, a.work, a.taps, out, M, a.T, a.J, a.L, ch.smod, count);
        le = hipGetLastError();
        if (le != hipSuccess)
            return le;
    }
    if (hist_len > 0)
    {
        hipLaunchKernelGGL((rsynth_carry_kernel<I16>), dim3(stream_generic_groups(hist_len, RSYNTH_THREADS, a.grid_limit)),
                           dim3(RSYNTH_THREADS), 0, a.stream, a.in, a.hist, a.hist_out, hist_len, n);
        return hipGetLastError();
    }
    return hipSuccess;
}

template <bool I16, bool O16>
static hipError_t launch_t(const RsynthArgs &a)
{
    switch (a.M)
    {
    case 128: return launch_chunks<128, I16, O16>(a);
    case 256: return launch_chunks<256, I16, O16>(a);
    case 512: return launch_chunks<512, I16, O16>(a);
    case 1024: return launch_chunks<1024, I16, O16>(a);
    case 2048: return launch_chunks<2048, I16, O16>(a);
    case 4096: return launch_chunks<4096, I16, O16>(a);
    case 8192: return launch_chunks<8192, I16, O16>(a);
    default: return hipErrorInvalidValue;
    }
}

hipError_t launch_rsynth(const RsynthArgs &a)
{
    if (a.M < 1 || a.T < 1 || a.L < 1 || !rsynth_config_ok((uint32_t)a.M, (uint32_t)a.T, (uint32_t)a.L) ||
        a.J != (int)synth_terms((uint32_t)a.T, (uint32_t)a.L) || a.first_bin < 0 || a.bins < 1 ||
        !rsynth_span_ok((uint32_t)a.first_bin, (uint32_t)a.bins, (uint32_t)a.M) || a.frames < 1 || (uint64_t)a.frames > RSYNTH_MAX_CALL ||
        a.work_frames < (uint64_t)a.J || a.work_frames * (uint64_t)a.M * 4 > RSYNTH_WORKSPACE_MAX || a.call.smod >= (uint32_t)a.M ||
        a.call.outputs != (uint64_t)a.frames * (uint64_t)a.L || a.call.carry != (uint32_t)a.J - 1)
        return hipErrorInvalidValue;
    if (a.in_i16)
        return a.out_i16 ? launch_t<true, true>(a) : launch_t<true, false>(a);
    return a.out_i16 ? launch_t<false, true>(a) : launch_t<false, false>(a);
}

} // namespace if_fir
