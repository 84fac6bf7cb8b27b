// if_fir_arb.h — internal interface between the arbitrary-ratio resampler's C-ABI shim and its HIP kernel (not installed).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "if_fir_arb_plan.h"

namespace if_fir
{

struct ArbArgs
{
    const void *in;        // device, N input samples (float32 or int16 I,Q)
    void *out;             // device, count float32 I,Q outputs
    const float2 *hist;    // device, the K - 1 input samples before this call (float32, most recent last)
    float2 *hist_out;      // device, the other ping-pong buffer: receives the history of the next call
    const float *taps;     // device, the table of arb_build_taps
    int T, bits, in_i16;
    uint64_t step;         // R
    uint64_t tau_rel;      // tau - c 2^32 at the start of the call (< 2^34)
    int64_t N;             // inputs of this call (> 0)
    int64_t count;         // outputs of this call (arb_out_count; may be 0: the history is still written)
    int grid_limit;        // at most this many workgroups (0 = the launcher's choice); same results
    int device;
    hipStream_t stream;
};

hipError_t launch_arb(const ArbArgs &a);

} // namespace if_fir
