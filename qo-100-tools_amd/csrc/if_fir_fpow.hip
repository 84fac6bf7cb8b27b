// if_fir_fpow.hip — frame power stage for gfx950: frames in the polyphase banks' layout in, K-frame averages of |.|^2 per bin out
// as the WB detector's spectrum codes and, optionally, float32 powers (docs/SPEC.md §19).
//
//   p(a, i) = fma(re, re, im im);   e_a[j] = sum of G adjacent p from +0 in element order;   a frame's e_a in chunks of 8 from +0
//   in frame order;   acc[j] = the chunk sums from +0 in chunk order;   P[f][j] = acc[j] * float32(1 / (K G fNorm))
//
// fpow_chunk_kernel<I16, G1>: LANES RUN ALONG OUTPUT BINS.  An item is one chunk of a call (fpow_chunk_entry, if_fir_fpow_plan.h)
// and one lane's bins of it, numbered with the bin fastest, so a wave reads one contiguous run of a frame per row whatever B is.
// G = 1 (G1): a lane owns the output bins of one 16-byte load, two complex64 or four int16 pairs; where the row's address is not
// 16-byte aligned (an odd B on every other row, an odd first element, an element-aligned base) or the lane's bins run past Bo,
// it loads them one element at a time: the same values, and the arithmetic does not know which loaded them.  A whole chunk
// whose rows all lie on the 16-byte grid issues its eight loads together.  G > 1: a lane owns
// one output bin and walks its G elements in order, one at a time up to a 16-byte boundary, 16 bytes at a time from there, one
// at a time for what is left.  The call's first chunk starts from the carried partial sum, every other from +0; every chunk sum,
// finished or not, goes to the workspace.  No LDS, no scratch.
// fpow_frame_kernel: one thread per (output frame, bin) adds the finished chunk sums in chunk order onto the carried accumulator;
// a completed frame is scaled once and mapped to its code in float64 (§8's mapping, restated here: psd_frame_kernel keeps its
// own), an open one stores its accumulator and the open chunk's partial sum for the next call.
// Every sum is made by the same operations in the same order whatever the call, so a stream cut anywhere gives the same bits;
// the operations the definition spells out are explicit intrinsics, which no contraction setting changes.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <mutex>

#include "if_fir_fpow.h"
#include "if_fir_kernels.h"
#include "if_fir_stream_dev.h"

namespace if_fir
{

typedef float fpow_v4f __attribute__((ext_vector_type(4)));
typedef int fpow_v4i __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float fpow_p(float re, float im)
{
    return __fmaf_rn(re, re, __fmul_rn(im, im));
}

// element e of the call's input, element-aligned
template <bool I16>
__device__ __forceinline__ float fpow_element(const void *__restrict__ in, int64_t e)
{
    const stream_v2f v = stream_sample<I16>(in, e);
    return fpow_p(v.x, v.y);
}

// is element e at a 16-byte boundary?
template <bool I16>
__device__ __forceinline__ bool fpow_aligned(const void *__restrict__ in, int64_t e)
{
    return (((uintptr_t)in + (uint64_t)e * (I16 ? 4 : 8)) & 15) == 0;
}

// the elements e .. e + V - 1 in one 16-byte load (e at a 16-byte boundary, all of them inside the call)
template <bool I16>
__device__ __forceinline__ void fpow_vector(const void *__restrict__ in, int64_t e, float (&p)[I16 ? 4 : 2])
{
    if constexpr (I16)
    {
        const fpow_v4i w = *reinterpret_cast<const fpow_v4i *>(static_cast<const int *>(in) + e);
#pragma unroll
        for (int i = 0; i < 4; i++)
            p[i] = fpow_p((float)(short)(w[i] & 0xffff) * (1.0f / 32768.0f), (float)(w[i] >> 16) * (1.0f / 32768.0f));
    }
    else
    {
        const fpow_v4f v = *reinterpret_cast<const fpow_v4f *>(static_cast<const float2 *>(in) + e);
        p[0] = fpow_p(v.x, v.y);
        p[1] = fpow_p(v.z, v.w);
    }
}

// one row (input frame) of a lane's bins onto its sums.  e = the lane's first element of the row; G1: `live` of the lane's V
// bins exist (V: all of them)
template <bool I16, bool G1>
__device__ __forceinline__ void fpow_row(const void *__restrict__ in, int64_t e, int G, int live, float (&sum)[G1 ? (I16 ? 4 : 2) : 1])
{
    constexpr int V = I16 ? 4 : 2;
    float p[V];
    if constexpr (G1)
    {
        if (live == V && fpow_aligned<I16>(in, e))
        {
            fpow_vector<I16>(in, e, p);
#pragma unroll
            for (int i = 0; i < V; i++)
                sum[i] = __fadd_rn(sum[i], __fadd_rn(0.f, p[i]));
        }
        else
        {
#pragma unroll
            for (int i = 0; i < V; i++)
                if (i < live)
                    sum[i] = __fadd_rn(sum[i], __fadd_rn(0.f, fpow_element<I16>(in, e + i)));
        }
    }
    else
    {
        float ea = 0.f;
        int g = 0;
        for (; g < G && !fpow_aligned<I16>(in, e + g); g++)
            ea = __fadd_rn(ea, fpow_element<I16>(in, e + g));
#pragma unroll 4
        for (; g + V <= G; g += V)
        {
            fpow_vector<I16>(in, e + g, p);
#pragma unroll
            for (int i = 0; i < V; i++)
                ea = __fadd_rn(ea, p[i]);
        }
        for (; g < G; g++)
            ea = __fadd_rn(ea, fpow_element<I16>(in, e + g));
        sum[0] = __fadd_rn(sum[0], ea);
    }
}

template <bool I16, bool G1>
__global__ __launch_bounds__(FPOW_THREADS) void fpow_chunk_kernel(const void *__restrict__ in, const float *__restrict__ partial,
                                                                  float *__restrict__ work, int B, int first, int G, int Bo, int K,
                                                                  uint32_t chunk0, uint32_t skip, uint32_t chunks, int64_t F, int slots)
{
    constexpr int OB = G1 ? (I16 ? 4 : 2) : 1; // output bins of one lane
    const int64_t items = (int64_t)chunks * slots;
    const bool rows_on_grid = ((int64_t)B * (I16 ? 4 : 8)) % 16 == 0;
    for (int64_t item = (int64_t)blockIdx.x * FPOW_THREADS + threadIdx.x; item < items; item += (int64_t)gridDim.x * FPOW_THREADS)
    {
        const uint32_t q = (uint32_t)(item / slots);
        const int j0 = (int)(item - (int64_t)q * slots) * OB;
        const int live = Bo - j0 < OB ? Bo - j0 : OB;
        uint64_t row0;
        uint32_t count;
        bool from_partial;
        fpow_chunk_entry(chunk0, skip, q, (uint32_t)K, (uint64_t)F, &row0, &count, &from_partial);
        float sum[OB];
#pragma unroll
        for (int i = 0; i < OB; i++)
            sum[i] = (from_partial && i < live) ? partial[j0 + i] : 0.f;
        const int64_t e0 = (int64_t)row0 * B + first + (int64_t)j0 * G;
        bool summed = false;
        if constexpr (G1)
        {
            // a whole chunk whose rows all start on the 16-byte grid (the row pitch is a multiple of 16 bytes): its eight loads
            // are issued together, then summed in row order -- the same operations as fpow_row's
            if (count == (uint32_t)FPOW_CHUNK && live == OB && rows_on_grid && fpow_aligned<I16>(in, e0))
            {
                float p[FPOW_CHUNK][OB];
#pragma unroll
                for (int u = 0; u < FPOW_CHUNK; u++)
                    fpow_vector<I16>(in, e0 + (int64_t)u * B, p[u]);
#pragma unroll
                for (int u = 0; u < FPOW_CHUNK; u++)
#pragma unroll
                    for (int i = 0; i < OB; i++)
                        sum[i] = __fadd_rn(sum[i], __fadd_rn(0.f, p[u][i]));
                summed = true;
            }
        }
        if (!summed)
            for (uint32_t u = 0; u < count; u++)
                fpow_row<I16, G1>(in, e0 + (int64_t)u * B, G, live, sum);
        float *dst = work + (int64_t)q * Bo + j0;
#pragma unroll
        for (int i = 0; i < OB; i++)
            if (i < live)
                dst[i] = sum[i];
    }
}

// thread (output frame t of the call, bin b): the frame's finished chunks of this call in chunk order onto the accumulator
__global__ __launch_bounds__(FPOW_THREADS) void fpow_frame_kernel(const float *__restrict__ work, const float *__restrict__ state,
                                                                  float *__restrict__ state_out, uint16_t *__restrict__ codes,
                                                                  float *__restrict__ power, int Bo, int K, uint32_t chunk0, uint64_t done,
                                                                  uint64_t chunks, uint32_t touched, float scale, double ref_power)
{
    const int64_t n = (int64_t)touched * Bo;
    for (int64_t idx = (int64_t)blockIdx.x * FPOW_THREADS + threadIdx.x; idx < n; idx += (int64_t)gridDim.x * FPOW_THREADS)
    {
        const uint32_t t = (uint32_t)(idx / Bo), b = (uint32_t)(idx - (int64_t)t * Bo);
        uint64_t lo, hi;
        bool complete;
        fpow_frame_entry(chunk0, done, t, (uint32_t)K, &lo, &hi, &complete);
        float a = (t == 0 && chunk0 > 0) ? state[b] : 0.f;
        for (uint64_t c = lo; c < hi; c++)
            a = __fadd_rn(a, work[c * Bo + b]);
        if (!complete)
        {
            // the open frame: its accumulator and, when the call ends inside a chunk, that chunk's partial sum
            state_out[b] = a;
            if (done < chunks)
                state_out[Bo + b] = work[done * Bo + b];
            continue;
        }
        const float p = __fmul_rn(a, scale);
        if (power)
            power[(size_t)t * Bo + b] = p;
        // SPEC §8's mapping (the detector's scale, wb_detect.hip): -3.35 dB .. 16.7 dB over 65535 codes
        const double slope = (16.7 - (-3.35)) / 65535;
        const double db = 10.0 * log10((double)p / ref_power); // p = 0: -inf, code 0
        double code = rint((db - (-3.35)) / slope);
        code = code > 0.0 ? code : 0.0; // (also takes -inf, and a NaN were there one)
        code = code < 65535.0 ? code : 65535.0;
        codes[(size_t)t * Bo + b] = (uint16_t)code;
    }
}

template <bool I16, bool G1>
static hipError_t launch_t(const FpowArgs &a)
{
    int cus = 0;
    const hipError_t e = stream_kernel_setup<&fpow_chunk_kernel<I16, G1>>(a.device, 0, &cus);
    if (e != hipSuccess)
        return e;
    constexpr int OB = G1 ? (I16 ? 4 : 2) : 1;
    const int slots = (a.Bo + OB - 1) / OB;
    const int64_t items = (int64_t)a.plan.chunks * slots;
    // a grid-stride loop over the items on as many workgroups as are resident at a time
    const unsigned groups = stream_persistent_groups(cus, FPOW_GROUPS_PER_CU, (items + FPOW_THREADS - 1) / FPOW_THREADS, a.grid_limit);
    hipLaunchKernelGGL((fpow_chunk_kernel<I16, G1>), dim3(groups), dim3(FPOW_THREADS), 0, a.stream, a.in, a.state + a.Bo, a.work, a.B,
                       a.first, a.G, a.Bo, a.K, a.plan.chunk0, a.plan.skip, (uint32_t)a.plan.chunks, a.F, slots);
    hipError_t le = hipGetLastError();
    if (le != hipSuccess)
        return le;
    const int64_t threads = (int64_t)a.plan.touched * a.Bo;
    hipLaunchKernelGGL(fpow_frame_kernel, dim3(stream_generic_groups(threads, FPOW_THREADS, a.grid_limit)), dim3(FPOW_THREADS), 0, a.stream,
                       a.work, a.state, a.state_out, a.codes, a.power, a.Bo, a.K, a.plan.chunk0, a.plan.done, a.plan.chunks,
                       (uint32_t)a.plan.touched, a.scale, a.ref_power);
    return hipGetLastError();
}

hipError_t launch_fpow(const FpowArgs &a)
{
    FpowPlan again;
    if (a.B < 1 || a.B > (int)FPOW_MAX_BINS || a.G < 1 || a.G > (int)FPOW_MAX_GROUP || a.Bo < 1 || a.first < 0 ||
        (int64_t)a.first + (int64_t)a.G * a.Bo > a.B || a.K < 1 || a.K > (int)FPOW_MAX_FRAMES || a.F < 1 ||
        (uint64_t)a.F > FPOW_MAX_CALL_FRAMES || a.plan.chunk0 >= fpow_chunks_per_frame((uint32_t)a.K) || a.plan.skip >= (uint32_t)FPOW_CHUNK ||
        !fpow_plan((uint64_t)a.plan.chunk0 * FPOW_CHUNK + a.plan.skip, (uint64_t)a.F, (uint32_t)a.K, &again) ||
        again.chunk0 != a.plan.chunk0 || again.skip != a.plan.skip || again.chunks != a.plan.chunks || again.done != a.plan.done || again.touched != a.plan.touched || again.frames != a.plan.frames ||
        a.plan.chunks < 1 || a.plan.chunks * (uint64_t)a.Bo > FPOW_MAX_WORK)
        return hipErrorInvalidValue;
    if (a.G == 1)
        return a.in_i16 ? launch_t<true, true>(a) : launch_t<false, true>(a);
    return a.in_i16 ? launch_t<true, false>(a) : launch_t<false, false>(a);
}

} // namespace if_fir
