// if_fir_rsynth.h — internal interface between the real-output polyphase synthesis bank's C-ABI shim and its HIP kernels (not installed).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "if_fir_rsynth_plan.h"

namespace if_fir
{

struct RsynthArgs
{
    const void *in;         // device, frames x bins elements of this call (float32 or int16 I,Q), frame-major
    const float2 *hist;     // device, the (J-1) bins elements before this call (float32, most recent frame last)
    float2 *hist_out;       // device, the other ping-pong buffer: receives the last (J-1) bins elements of (hist || call)
    const float *taps;      // device, the table of synth_build_taps: J L float32
    const float2 *twiddle;  // device, M/2 entries exp(-2 pi i t / (M/2))
    const uint16_t *place;  // device, M/2 entries: rsynth_slot_place
    const float2 *pretangle; // device, M/4 + 1 entries: rsynth_build_twiddles
    float *work;            // device, work_frames x M floats: the transformed frames of a chunk, natural slot order
    void *out;              // device, frames x L REAL outputs, float32 or int16
    int M, T, J, L, first_bin, bins, in_i16, out_i16;
    int64_t frames;         // F of this call
    uint64_t work_frames;   // rows of `work`: at least J
    SynthCall call;         // synth_call(position, F, M, L, T)
    int grid_limit;         // development hook: at most this many workgroups per kernel (0 = the launcher's choice)
    int device;
    hipStream_t stream;
};

hipError_t launch_rsynth(const RsynthArgs &a);

} // namespace if_fir
