// if_fir_turn.h — internal interface between the corner turn's C-ABI shim and its HIP kernels (not installed).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "if_fir_turn_plan.h"

namespace if_fir
{

struct TurnArgs
{
    const void *in;       // device: F frames of B elements (TO_STREAMS) or C rows of pitch P (TO_FRAMES)
    void *out;            // device: the other side
    const uint16_t *map;  // device: sel[c], C values (TO_STREAMS), or inv[i], B values (TO_FRAMES)
    int direction, B, C, in_i16, out_i16;
    int64_t F;            // frames of this call, >= 1
    int64_t P;            // row pitch in elements, >= F
    int grid_limit;       // > 0: at most this many workgroups (development hook)
    int device;
    hipStream_t stream;
};

hipError_t launch_turn(const TurnArgs &a);

} // namespace if_fir
