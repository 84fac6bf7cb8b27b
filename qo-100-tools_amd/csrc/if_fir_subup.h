// if_fir_subup.h — internal interface between the per-bin interpolating FIR stage's C-ABI shim and its HIP kernels (not installed).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "if_fir_subup_plan.h"

namespace if_fir
{

struct SubUpArgs
{
    const void *in;         // device, F frames of B elements (complex64 or int16 pairs), frame-major
    float2 *out;            // device, F R frames of B complex64
    const float2 *hist;     // device, the J - 1 frames before this call (float32, most recent last)
    float2 *hist_out;       // device, the other ping-pong buffer: receives the history of the next call
    const float *taps;      // device, the table of subup_build_table (tap-major, zero-padded to J R taps)
    const uint32_t *words;  // device, B phase words (0 = that bin is not rotated)
    int B, T, rows, R, in_i16;
    int64_t F;              // frames of this call (> 0)
    SubUpCall call;         // subup_call
    int grid_limit;         // at most this many workgroups (0 = the launcher's choice); same results
    int device;
    hipStream_t stream;
};

hipError_t launch_subup(const SubUpArgs &a);

} // namespace if_fir
