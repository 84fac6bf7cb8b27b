// if_fir_synth.hip — polyphase synthesis bank (weighted overlap-add synthesis): M channel streams on a uniform grid to one IQ
// stream in one pass, for gfx950 (docs/SPEC.md §14).
//
//   y[n] = sum_{j<J} h[t_j] v_{m_j}[n mod M],   m_j = floor(n / L) - j,  t_j = (n mod L) + j L,  terms with t_j >= T skipped
//   v_m[s] = sum_k X_k[m] e^{+j 2 pi k s / M} = F_m[(M - s) mod M],  F_m the forward M-point transform of frame m
//
// Two routes, the same bits (synth_route, if_fir_synth_plan.h).  Where two workgroups of it fit a CU's LDS, one kernel:
// synth_ring_kernel<M, I16> (below, at its definition).  Elsewhere a call is cut into chunks of a device workspace; per chunk,
// on the context's stream:
// synth_transform_kernel<M, I16>: a workgroup takes B = synth_batch(M) consecutive frames of (history || call) at a time
// (B M >= 1024 points, so every lane has a butterfly in every pass).  Channel k of a frame goes to LDS slot k (coalesced global
// loads along the span, int16 converted on the way, frames before the call from the carried history, channels outside the span
// +0), then the in-place transform of if_fir_lds_fft_dev.h over all B blocks at once, and slot s of v leaves for the workspace
// from place psd_bin_position((M - s) mod M, M), coalesced along s.
// synth_emit_kernel: one output per lane, coalesced along n: the chain acc = fma(h[t_j], v_{m_j}[n mod M], acc), j = 0 .. J-1
// (newest frame first), from the workspace and the tap table.
// synth_carry_kernel (once per call): the last J - 1 input frames of (history || call) go to the other ping-pong buffer as float32.
// An output's arithmetic depends on its J frames, the taps and n mod M only -- not on the call, the chunk, the batch or the
// workgroup -- so a stream cut anywhere gives the same bits.  The kernels see call-relative positions and (c L) mod M, never c.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <mutex>

#include "if_fir_kernels.h"
#include "if_fir_lds_fft_dev.h"
#include "if_fir_stream_dev.h"
#include "if_fir_synth.h"

namespace if_fir
{

// rows [0, rows) of `work` receive the transforms of the call's frames frame0 .. frame0 + rows - 1 (frame0 may be negative)
template <int M, bool I16>
__global__ __launch_bounds__(SYNTH_THREADS) IF_FIR_SINGLE_READS void synth_transform_kernel(
    const void *__restrict__ in, const float2 *__restrict__ hist, const float2 *__restrict__ twiddle, const uint16_t *__restrict__ place,
    float2 *__restrict__ work, int first_bin, int bins, int64_t hist_len, int64_t n, int64_t frame0, int64_t rows, int64_t batches)
{
    constexpr int B = (int)synth_batch(M), TOTAL = B * M;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    stream_v2f *x = reinterpret_cast<stream_v2f *>(smem);
    stream_v2f *tw = x + TOTAL;
    uint16_t *where = reinterpret_cast<uint16_t *>(tw + M);
    const int tid = threadIdx.x;
    for (int e = tid; e < M; e += SYNTH_THREADS)
    {
        const float2 t = twiddle[e];
        tw[e] = stream_v2f{t.x, t.y};
        where[e] = place[e];
    }

    for (int64_t g = blockIdx.x; g < batches; g += gridDim.x)
    {
        const int64_t r0 = g * B;
        __syncthreads(); // the previous batch has been stored (and, the first time, the twiddles are staged)
        for (int e = tid; e < TOTAL; e += SYNTH_THREADS)
        {
            const int fb = B == 1 ? 0 : e / M, k = e - fb * M;
            const int j = (int)synth_channel_index(first_bin, (uint32_t)k, M); // the element of channel k in a frame of the span
            stream_v2f v = {0.f, 0.f};
            if (j < bins && r0 + fb < rows)
                v = stream_load<I16>(in, hist, hist_len, n, (frame0 + r0 + fb) * bins + j);
            x[e] = v;
        }
        __syncthreads();
        lds_fft_passes<TOTAL, M, M, SYNTH_THREADS>(x, tw, tid);
        const int nb = rows - r0 < B ? (int)(rows - r0) : B;
        float2 *dst = work + (size_t)r0 * M;
        for (int e = tid; e < nb * M; e += SYNTH_THREADS)
        {
            const int fb = B == 1 ? 0 : e / M;
            const stream_v2f v = x[fb * M + where[e - fb * M]];
            dst[e] = make_float2(v.x, v.y);
        }
    }
}

// output i of the chunk, i < count = frames L: frame f = i / L of the chunk has its transform in row f + J - 1 of `work`
__global__ __launch_bounds__(SYNTH_THREADS) void synth_emit_kernel(const float2 *__restrict__ work, const float *__restrict__ taps,
                                                                    float2 *__restrict__ out, int M, int T, int J, int L, uint32_t smod,
                                                                    uint32_t count)
{
    for (uint32_t i = blockIdx.x * SYNTH_THREADS + threadIdx.x; i < count; i += gridDim.x * SYNTH_THREADS)
    {
        const uint32_t f = i / (uint32_t)L, p = i - f * (uint32_t)L;
        const uint32_t s = (smod + i) & (uint32_t)(M - 1);
        const float2 *v = work + (size_t)(f + J - 1) * M + s;
        float ax = 0.f, ay = 0.f;
#pragma unroll 4
        for (int j = 0; j < J; j++)
        {
            const int t = (int)p + j * L;
            if (t < T)
            {
                const float h = taps[t];
                const float2 w = v[-(ptrdiff_t)j * M];
                ax = fmaf(h, w.x, ax);
                ay = fmaf(h, w.y, ay);
            }
        }
        out[i] = make_float2(ax, ay);
    }
}

// The one-kernel route.  A workgroup owns RUNS of run_len consecutive batches of the call's frames (batch q = frames q B ..
// q B + B - 1) and keeps the transforms of the last NB = ceil((J-1)/B) + 1 batches in an LDS ring, slot by slot in NATURAL slot
// order.  Per batch: load into the oldest ring slot, transform in place, bring the block from the transform's places to natural
// order through registers (the one gather from digit-reversed places; the J reads of an output then go to consecutive
// addresses for consecutive lanes), emit the batch's B L outputs with synth_emit_kernel's chain.  A run starts by filling the
// ring with the NB - 1 batches before it, from the call or the history: that warm-up is the route's only extra work.
template <int M, bool I16>
__global__ __launch_bounds__(SYNTH_THREADS) IF_FIR_SINGLE_READS void synth_ring_kernel(
    const void *__restrict__ in, const float2 *__restrict__ hist, const float *__restrict__ taps, const float2 *__restrict__ twiddle,
    const uint16_t *__restrict__ place, float2 *__restrict__ out, int T, int J, int L, int first_bin, int bins, int64_t hist_len, int64_t n,
    int64_t frames, int64_t batches, int64_t run_len, int NB, uint32_t smod)
{
    constexpr int B = (int)synth_batch(M), TOTAL = B * M, R = TOTAL / SYNTH_THREADS;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    stream_v2f *ring = reinterpret_cast<stream_v2f *>(smem);
    stream_v2f *tw = ring + (size_t)NB * TOTAL;
    uint16_t *where = reinterpret_cast<uint16_t *>(tw + M);
    const int tid = threadIdx.x;
    for (int e = tid; e < M; e += SYNTH_THREADS)
    {
        const float2 t = twiddle[e];
        tw[e] = stream_v2f{t.x, t.y};
        where[e] = place[e];
    }

    for (int64_t q0 = (int64_t)blockIdx.x * run_len; q0 < batches; q0 += (int64_t)gridDim.x * run_len)
    {
        const int64_t q1 = batches - q0 < run_len ? batches : q0 + run_len;
        int cur = 0;
        for (int64_t q = q0 - (NB - 1); q < q1; q++)
        {
            stream_v2f *x = ring + cur * TOTAL;
            __syncthreads(); // the batch before has been emitted: its oldest slot is free (the first time: the twiddles are staged)
            for (int e = tid; e < TOTAL; e += SYNTH_THREADS)
            {
                const int fb = B == 1 ? 0 : e / M, k = e - fb * M;
                const int j = (int)synth_channel_index(first_bin, (uint32_t)k, M);
                stream_v2f v = {0.f, 0.f};
                if (j < bins)
                    v = stream_load<I16>(in, hist, hist_len, n, (q * B + fb) * bins + j); // before the history and past the call: 0
                x[e] = v;
            }
            __syncthreads();
            lds_fft_passes<TOTAL, M, M, SYNTH_THREADS>(x, tw, tid);
            stream_v2f keep[R];
#pragma unroll
            for (int i = 0; i < R; i++)
            {
                const int e = tid + i * SYNTH_THREADS, fb = B == 1 ? 0 : e / M;
                keep[i] = x[fb * M + where[e - fb * M]];
            }
            __syncthreads();
#pragma unroll
            for (int i = 0; i < R; i++)
                x[tid + i * SYNTH_THREADS] = keep[i];
            __syncthreads();
            if (q >= q0)
            {
                const int64_t f0 = q * B;
                const int nb = frames - f0 < B ? (int)(frames - f0) : B;
                const uint32_t s0 = smod + (uint32_t)((uint64_t)f0 * (uint64_t)L); // modulo 2^32, which M divides
                float2 *dst = out + (size_t)f0 * (size_t)L;
                for (int i = tid; i < nb * L; i += SYNTH_THREADS)
                {
                    const int fbi = i / L, p = i - fbi * L;
                    const int s = (int)((s0 + (uint32_t)i) & (uint32_t)(M - 1));
                    float ax = 0.f, ay = 0.f;
#pragma unroll 4
                    for (int j = 0; j < J; j++)
                    {
                        const int t = p + j * L;
                        if (t < T)
                        {
                            // frame fbi - j of this batch, or of the batch `back` batches ago
                            const int back = j > fbi ? (j - fbi + B - 1) / B : 0;
                            const int slot = cur - back < 0 ? cur - back + NB : cur - back;
                            const int fb = (fbi - j) & (B - 1);
                            const float h = taps[t];
                            const stream_v2f w = ring[slot * TOTAL + fb * M + s];
                            ax = fmaf(h, w.x, ax);
                            ay = fmaf(h, w.y, ay);
                        }
                    }
                    dst[i] = make_float2(ax, ay);
                }
            }
            cur = cur + 1 == NB ? 0 : cur + 1;
        }
    }
}

template <bool I16>
__global__ __launch_bounds__(SYNTH_THREADS) void synth_carry_kernel(const void *__restrict__ in, const float2 *__restrict__ hist,
                                                                    float2 *__restrict__ hist_out, int64_t hist_len, int64_t n)
{
    // the last hist_len elements of (hist || call) (its own loop: through a shared helper it compiles to other code, profiles/stream_plan_ab.txt)
    for (int64_t i = (int64_t)blockIdx.x * SYNTH_THREADS + threadIdx.x; i < hist_len; i += (int64_t)gridDim.x * SYNTH_THREADS)
    {
        const stream_v2f v = stream_load<I16>(in, hist, hist_len, n, n - hist_len + i);
        hist_out[i] = make_float2(v.x, v.y);
    }
}

template <int M, bool I16>
static hipError_t launch_chunks(const SynthArgs &a)
{
    int cus = 0;
    constexpr int lds = (int)synth_lds_bytes(M), B = (int)synth_batch(M);
    const hipError_t e = stream_kernel_setup<&synth_transform_kernel<M, I16>>(a.device, lds, &cus);
    if (e != hipSuccess)
        return e;
    const int64_t hist_len = (int64_t)(a.J - 1) * a.bins, n = a.frames * a.bins;
    if (a.route == SYNTH_ROUTE_LDS)
    {
        const int ring_lds = (int)synth_lds_route_bytes(M, (uint32_t)a.J), NB = (a.J - 1 + B - 1) / B + 1;
        const hipError_t re = stream_kernel_setup<&synth_ring_kernel<M, I16>>(a.device, SYNTH_LDS_PER_CU / 2, nullptr);
        if (re != hipSuccess)
            return re;
        const int64_t ring_batches = (a.frames + B - 1) / B;
        const unsigned most = stream_persistent_groups(cus, synth_lds_route_groups_per_cu(M, (uint32_t)a.J), ring_batches, a.grid_limit);
        const int64_t run_len = (int64_t)synth_run_batches((uint64_t)ring_batches, most);
        const unsigned groups = (unsigned)((ring_batches + run_len - 1) / run_len);
        hipLaunchKernelGGL((synth_ring_kernel<M, I16>), dim3(groups), dim3(SYNTH_THREADS), ring_lds, a.stream, a.in, a.hist, a.taps, a.twiddle,
                           a.place, a.out, a.T, a.J, a.L, a.first_bin, a.bins, hist_len, n, a.frames, ring_batches, run_len, NB, a.call.smod);
        const hipError_t le = hipGetLastError();
        if (le != hipSuccess)
            return le;
    }
    else
    {
        const uint64_t per_chunk = synth_even_chunk_frames((uint64_t)a.frames, synth_chunk_frames(a.work_frames, (uint32_t)a.J)),
                       chunks = synth_chunks((uint64_t)a.frames, per_chunk);
        for (uint64_t i = 0; i < chunks; i++)
        {
            const SynthChunk ch = synth_chunk(i, (uint64_t)a.frames, per_chunk, (uint32_t)M, (uint32_t)a.L, a.call.smod);
            const int64_t rows = (int64_t)ch.frames + a.J - 1, batches = (rows + B - 1) / B;
            const unsigned groups = stream_persistent_groups(cus, synth_groups_per_cu(M), batches, a.grid_limit);
            hipLaunchKernelGGL((synth_transform_kernel<M, I16>), dim3(groups), dim3(SYNTH_THREADS), lds, a.stream, a.in, a.hist, a.twiddle,
                               a.place, a.work, a.first_bin, a.bins, hist_len, n, (int64_t)ch.first - (a.J - 1), rows, batches);
            hipError_t le = hipGetLastError();
            if (le != hipSuccess)
                return le;
            const uint32_t count = (uint32_t)(ch.frames * (uint64_t)a.L);
            hipLaunchKernelGGL(synth_emit_kernel, dim3(stream_generic_groups(count, SYNTH_THREADS, a.grid_limit)), dim3(SYNTH_THREADS), 0,
                               a.stream, a.work, a.taps, a.out + (size_t)ch.first * (size_t)a.L, M, a.T, a.J, a.L, ch.smod, count);
            le = hipGetLastError();
            if (le != hipSuccess)
                return le;
        }
    }
    if (hist_len > 0)
    {
        hipLaunchKernelGGL((synth_carry_kernel<I16>), dim3(stream_generic_groups(hist_len, SYNTH_THREADS, a.grid_limit)), dim3(SYNTH_THREADS), 0,
                           a.stream, a.in, a.hist, a.hist_out, hist_len, n);
        return hipGetLastError();
    }
    return hipSuccess;
}

template <bool I16>
static hipError_t launch_t(const SynthArgs &a)
{
    switch (a.M)
    {
    case 64: return launch_chunks<64, I16>(a);
    case 128: return launch_chunks<128, I16>(a);
    case 256: return launch_chunks<256, I16>(a);
    case 512: return launch_chunks<512, I16>(a);
    case 1024: return launch_chunks<1024, I16>(a);
    case 2048: return launch_chunks<2048, I16>(a);
    case 4096: return launch_chunks<4096, I16>(a);
    default: return hipErrorInvalidValue;
    }
}

hipError_t launch_synth(const SynthArgs &a)
{
    if (a.M < 1 || a.T < 1 || a.L < 1 || !synth_config_ok((uint32_t)a.M, (uint32_t)a.T, (uint32_t)a.L) ||
        a.J != (int)synth_terms((uint32_t)a.T, (uint32_t)a.L) || a.bins < 1 || a.bins > a.M || a.first_bin < -a.M / 2 || a.first_bin >= a.M ||
        a.frames < 1 || (uint64_t)a.frames > SYNTH_MAX_CALL || a.work_frames < (uint64_t)a.J ||
        a.work_frames * (uint64_t)a.M * 8 > SYNTH_WORKSPACE_MAX || a.call.smod >= (uint32_t)a.M ||
        a.call.outputs != (uint64_t)a.frames * (uint64_t)a.L || a.call.carry != (uint32_t)a.J - 1 ||
        (a.route != SYNTH_ROUTE_WORKSPACE && (a.route != SYNTH_ROUTE_LDS || !synth_lds_route_fits((uint32_t)a.M, (uint32_t)a.J))))
        return hipErrorInvalidValue;
    return a.in_i16 ? launch_t<true>(a) : launch_t<false>(a);
}

} // namespace if_fir
