// if_fir_rpfb.h — internal interface between the real-input polyphase filter bank's C-ABI shim and its HIP kernels (not installed).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "if_fir_rpfb_plan.h"

namespace if_fir
{

struct RpfbArgs
{
    const void *in;          // device, n REAL samples of this call (float32 or int16)
    const float *hist;       // device, the hist_len samples before this call (float32, most recent last)
    float *hist_out;         // device, the other ping-pong buffer: receives the last hist_len samples of (hist || call)
    const float *taps;       // device, the table of rpfb_build_taps: K M float32
    const float2 *twiddle;   // device, M/2 entries exp(-2 pi i t / (M/2)): the transform's
    const uint32_t *places;  // device, M/2 words of rpfb_build_places
    const float2 *untangle;  // device, M/2 + 1 entries W_M^k of rpfb_build_twiddles
    float2 *out;             // device, frames x bins
    int M, T, K, D, first_bin, bins, in_i16;
    int hist_len;            // T - 1
    int64_t n;               // samples of this call
    RpfbCall call;           // rpfb_call(position, n, M, D, T)
    int grid_limit;          // development hook: at most this many workgroups (0 = the launcher's choice)
    int device;
    hipStream_t stream;
};

hipError_t launch_rpfb(const RpfbArgs &a);

} // namespace if_fir
