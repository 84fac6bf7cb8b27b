// if_fir_stream_dev.h — what the kernel units of the streaming families (STREAM_FAMILIES in the Makefile) share: the device
// counterpart of if_fir_stream_ctx.h, under the same rule -- nothing here branches on which family includes it.  The sample load
// of a call, the compensated addition, the single-LDS-reads attribute, the launchers' one-time setup and their grid sizes.
// (ip_load, the interpolator's and the combiner's sample load, is in if_fir_interp_dev.h: DESIGN.md §3.11, Device side.)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "if_fir_kernels.h"

// LDS reads as single ds_read_b64 / ds_read_b32 (a ds_read2_b64 pair takes 8 LDS cycles on 32 banks, two single reads 2 each on
// 64; measured on the decimator's overlap-save units, if_fir_fft_dev.h, IF_FIR_LDS_SINGLE_READS): the machine-level pairing is
// switched off per kernel here (device pass only: the host pass does not know the feature), the IR-level vectorizer for the
// whole unit (csrc/Makefile, NOPAIR)
#if defined(__HIP_DEVICE_COMPILE__)
#define IF_FIR_SINGLE_READS __attribute__((target("no-load-store-opt")))
#else
#define IF_FIR_SINGLE_READS
#endif

namespace if_fir
{

typedef float stream_v2f __attribute__((ext_vector_type(2)));

// input sample j of this call (0 <= j < N, not checked) as float32 (I, Q); int16: (I, Q) packed in a dword, value * 2^15
template <bool I16>
__device__ __forceinline__ stream_v2f stream_sample(const void *__restrict__ in, int64_t j)
{
    stream_v2f v;
    if constexpr (I16)
    {
        const int w = static_cast<const int *>(in)[j];
        v.x = (float)(short)(w & 0xffff) * (1.0f / 32768.0f);
        v.y = (float)(w >> 16) * (1.0f / 32768.0f);
    }
    else
    {
        const float2 s = static_cast<const float2 *>(in)[j];
        v.x = s.x;
        v.y = s.y;
    }
    return v;
}

// the same, bounds-checked: j < 0 from the history (hist[hist_len + j]), outside both reads 0
template <bool I16>
__device__ __forceinline__ stream_v2f stream_load(const void *__restrict__ in, const float2 *__restrict__ hist, int64_t hist_len,
                                                  int64_t N, int64_t j)
{
    stream_v2f v = {0.f, 0.f};
    if (j < 0)
    {
        if (j + hist_len >= 0)
        {
            const float2 h = hist[j + hist_len];
            v.x = h.x;
            v.y = h.y;
        }
    }
    else if (j < N)
        v = stream_sample<I16>(in, j);
    return v;
}

// the two again for a stream of REAL samples (one float32, or one int16 = value * 2^15, per sample; the history is float32)
template <bool I16>
__device__ __forceinline__ float stream_sample_real(const void *__restrict__ in, int64_t j)
{
    if constexpr (I16)
        return (float)static_cast<const short *>(in)[j] * (1.0f / 32768.0f);
    else
        return static_cast<const float *>(in)[j];
}

template <bool I16>
__device__ __forceinline__ float stream_load_real(const void *__restrict__ in, const float *__restrict__ hist, int64_t hist_len, int64_t N,
                                                  int64_t j)
{
    float v = 0.f;
    if (j < 0)
    {
        if (j + hist_len >= 0)
            v = hist[j + hist_len];
    }
    else if (j < N)
        v = stream_sample_real<I16>(in, j);
    return v;
}

// the REAL samples j and j + 1 in one load where both lie in the call (8 bytes at a 4-byte boundary, or 4 at a 2-byte one: the
// sample's own alignment is all that holds, j has either parity); at the call's edges two bounds-checked loads
template <bool I16>
__device__ __forceinline__ stream_v2f stream_load_real2(const void *__restrict__ in, const float *__restrict__ hist, int64_t hist_len,
                                                        int64_t N, int64_t j)
{
    if (j >= 0 && j + 1 < N)
    {
        if constexpr (I16)
        {
            short s[2];
            __builtin_memcpy(s, static_cast<const short *>(in) + j, sizeof s);
            return stream_v2f{(float)s[0] * (1.0f / 32768.0f), (float)s[1] * (1.0f / 32768.0f)};
        }
        else
        {
            stream_v2f v;
            __builtin_memcpy(&v, static_cast<const float *>(in) + j, sizeof v);
            return v;
        }
    }
    return stream_v2f{stream_load_real<I16>(in, hist, hist_len, N, j), stream_load_real<I16>(in, hist, hist_len, N, j + 1)};
}

// compensated (two-sum) addition: acc += x, what the rounding of that add lost onto `lost` (float or a vector of floats)
template <class V>
__device__ __forceinline__ void two_sum_add(V &acc, V &lost, const V &x)
{
    const V sum = acc + x, b = sum - acc;
    lost += (acc - (sum - b)) + (x - b);
    acc = sum;
}

// The head of a launcher: the one-time setup of device_setup (if_fir_kernels.h) for Kernel -- its dynamic-LDS limit raised to
// lds_max -- and the device's CU count.  The function-local DeviceSetup is keyed on the kernel's ADDRESS, hence `auto`: two
// instantiations such as fir_ddc_kernel<true> and <false> have the same function type, so a `template <typename K>` form
// would give them one DeviceSetup and skip the second kernel's LDS attribute.
template <auto Kernel>
inline hipError_t stream_kernel_setup(int device, int lds_max, int *cus)
{
    static DeviceSetup setup;
    return device_setup(setup, device, reinterpret_cast<const void *>(Kernel), lds_max, cus);
}

// workgroups of a grid-stride launch over `work` items: per_cu on every CU, at most one per item, at least one (which writes
// the history of a call without outputs), at most grid_limit when that is set (the tests' way to make the stride loop turn)
inline unsigned stream_persistent_groups(int cus, int per_cu, int64_t work, int grid_limit)
{
    int64_t groups = (int64_t)cus * per_cu;
    if (groups > work)
        groups = work > 0 ? work : 1;
    if (grid_limit > 0 && groups > grid_limit)
        groups = grid_limit;
    return (unsigned)groups;
}

// workgroups of a generic kernel, one output per thread and a grid-stride loop beyond 65536 of them; at least one, as above
inline unsigned stream_generic_groups(int64_t M, int threads, int grid_limit)
{
    int64_t groups = (M + threads - 1) / threads;
    if (groups < 1)
        groups = 1;
    if (groups > 65536)
        groups = 65536;
    if (grid_limit > 0 && groups > grid_limit)
        groups = grid_limit;
    return (unsigned)groups;
}

} // namespace if_fir
