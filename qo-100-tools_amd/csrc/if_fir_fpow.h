// if_fir_fpow.h — internal interface between the frame power stage's C-ABI shim and its HIP kernels (not installed).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "if_fir_fpow_plan.h"

namespace if_fir
{

struct FpowArgs
{
    const void *in;       // device, F frames of B elements (complex64 or int16 pairs)
    float *work;          // device, plan.chunks x Bo chunk sums of this call
    const float *state;   // device, 2 Bo: the open frame's accumulator, then the open chunk's partial sum
    float *state_out;     // device, the other ping-pong buffer: receives what the call leaves open
    uint16_t *codes;      // device, plan.frames x Bo
    float *power;         // device, plan.frames x Bo, or nullptr
    int B, first, G, Bo, K, in_i16;
    int64_t F;            // frames of this call, >= 1
    FpowPlan plan;        // fpow_plan(position, F, K)
    float scale;          // fpow_scale
    double ref_power;
    int grid_limit;       // > 0: at most this many workgroups per kernel (development hook)
    int device;
    hipStream_t stream;
};

hipError_t launch_fpow(const FpowArgs &a);

} // namespace if_fir
