// if_fir_resamp.h — internal interface between the resampler's C-ABI shim and its HIP kernel (not installed).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "if_fir_resamp_plan.h"

namespace if_fir
{

struct ResampArgs
{
    const void *in;        // device, N input samples (float32 or int16 I,Q)
    void *out;             // device, count float32 I,Q outputs
    const float2 *hist;    // device, the K - 1 input samples before this call (float32, most recent last)
    float2 *hist_out;      // device, the other ping-pong buffer: receives the history of the next call
    const float *taps;     // device, the phase-major table of resamp_build_taps
    int T, L, M, ctaps, in_i16;
    int64_t N;             // inputs of this call (> 0)
    int64_t count;         // outputs of this call (resamp_call; may be 0: the history is still written)
    int t0;                // resamp_call
    int grid_limit;        // at most this many workgroups (0 = the launcher's choice); same results
    int device;
    hipStream_t stream;
};

hipError_t launch_resamp(const ResampArgs &a);

} // namespace if_fir
