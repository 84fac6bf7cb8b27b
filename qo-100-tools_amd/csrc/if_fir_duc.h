// if_fir_duc.h — internal interface between the up-converter's C-ABI shim and its HIP kernel (not installed).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "if_fir_duc_plan.h"

namespace if_fir
{

struct DucArgs
{
    const void *in;        // device, N complex input samples (float32 pairs or int16 pairs)
    void *out;             // device, N L real outputs (float32 or int16)
    const float2 *hist;    // device, the K - 1 input samples before this call (unrotated float32, most recent last)
    float2 *hist_out;      // device, the other ping-pong buffer: receives the history of the next call
    const float *taps;     // device, the table of duc_build_table
    int T, L, in_i16, out_i16;
    int64_t N;             // inputs of this call (> 0)
    uint32_t nco_word;     // SPEC §11 phase word P (0 = no rotation)
    uint32_t nco_abs0;     // absolute index (mod 2^32) of the call's first input sample
    int grid_limit;        // at most this many workgroups (0 = the launcher's choice); same results
    int device;
    hipStream_t stream;
};

hipError_t launch_duc(const DucArgs &a);

} // namespace if_fir
