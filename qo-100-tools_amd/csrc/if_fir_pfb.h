// if_fir_pfb.h — internal interface between the polyphase filter bank's C-ABI shim and its HIP kernels (not installed).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "if_fir_pfb_plan.h"

namespace if_fir
{

struct PfbArgs
{
    const void *in;          // device, n samples of this call (float32 or int16 I,Q)
    const float2 *hist;      // device, the hist_len samples before this call (float32, most recent last)
    float2 *hist_out;        // device, the other ping-pong buffer: receives the last hist_len samples of (hist || call)
    const float *taps;       // device, the table of pfb_build_taps: K M float32
    const float2 *twiddle;   // device, M entries exp(-2 pi i t / M)
    const uint16_t *bin_pos; // device, bins entries: where the transform leaves output bin j (pfb_bin_place)
    float2 *out;             // device, frames x bins
    int M, T, K, D, bins, in_i16;
    int hist_len;            // T - 1
    int64_t n;               // samples of this call
    PfbCall call;            // pfb_call(position, n, M, D, T)
    int grid_limit;          // development hook: at most this many workgroups (0 = the launcher's choice)
    int device;
    hipStream_t stream;
};

hipError_t launch_pfb(const PfbArgs &a);

} // namespace if_fir
