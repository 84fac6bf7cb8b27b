// if_fir_ddc.h — internal interface between the down-converter's C-ABI shim and its HIP kernel (not installed).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "if_fir_ddc_plan.h"

namespace if_fir
{

struct DdcArgs
{
    const void *in;        // device, N real input samples (float32 or int16)
    void *out;             // device, count float32 I,Q outputs
    const float *hist;     // device, the T - 1 input samples before this call (float32, most recent last)
    float *hist_out;       // device, the other ping-pong buffer: receives the history of the next call
    const float *taps;     // device, the table of ddc_build_table
    int T, D, in_i16;
    int64_t N;             // inputs of this call (> 0)
    int64_t count;         // outputs of this call (ddc_call; may be 0: the history is still written)
    int n0;                // ddc_call
    uint32_t nco_word;     // SPEC §3.2 phase word P (0 = no rotation)
    uint32_t nco_abs0;     // absolute index (mod 2^32) of the input sample under the call's first output
    int grid_limit;        // at most this many workgroups (0 = the launcher's choice); same results
    int device;
    hipStream_t stream;
};

hipError_t launch_ddc(const DdcArgs &a);

} // namespace if_fir
