// if_fir_psd.h — internal interface between the power-spectrum estimator's C-ABI shim and its HIP kernels (not installed).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "if_fir_psd_plan.h"

namespace if_fir
{

struct PsdArgs
{
    const void *in;          // device, n samples of this call (float32 or int16 I,Q)
    const float2 *carry;     // device, the `carried` samples before this call (float32, most recent last)
    float2 *carry_out;       // device, the other ping-pong buffer: receives the plan's carry
    const float *window;     // device, N float32
    const float2 *twiddle;   // device, N entries exp(-2 pi i t / N)
    const uint16_t *bin_pos; // device, bins entries: where the transform leaves output bin j (psd_bin_position)
    float *work;             // device, chunks x bins chunk sums
    const float *acc;        // device, bins: the open frame's accumulator (read when chunk0 > 0)
    float *acc_out;          // device, bins: the other ping-pong buffer (written when the call leaves a frame open)
    uint16_t *codes;         // device, frames x bins
    float *power;            // device, frames x bins, or nullptr
    int N, H, K, bins, in_i16;
    int64_t n;               // samples of this call
    int64_t carried;         // samples in `carry`
    PsdPlan plan;            // psd_plan(position, carried, n)
    float scale;             // 1 / (K sum w^2)
    double ref_power;
    int grid_limit;          // > 0: at most this many workgroups of the chunk kernel (development hook)
    int device;
    hipStream_t stream;
};

hipError_t launch_psd(const PsdArgs &a);

} // namespace if_fir
