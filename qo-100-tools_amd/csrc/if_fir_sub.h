// if_fir_sub.h — internal interface between the per-channel FIR stage's C-ABI shim and its HIP kernels (not installed).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "if_fir_sub_plan.h"

namespace if_fir
{

struct SubArgs
{
    const void *in;         // device, F frames of B elements (complex64 or int16 pairs), frame-major
    float2 *out;            // device, call.count frames of B complex64
    const float2 *hist;     // device, the T - 1 frames before this call (float32, most recent last)
    float2 *hist_out;       // device, the other ping-pong buffer: receives the history of the next call
    const float2 *taps;     // device, the table of sub_build_table (tap-major)
    const uint32_t *words;  // device, B phase words (SPEC §3.2; 0 = that bin is not rotated)
    int B, T, R, in_i16;
    int64_t F;              // frames of this call (> 0)
    SubCall call;           // sub_call (count may be 0: the history is still moved)
    int grid_limit;         // at most this many workgroups (0 = the launcher's choice); same results
    int device;
    hipStream_t stream;
};

hipError_t launch_sub(const SubArgs &a);

} // namespace if_fir
