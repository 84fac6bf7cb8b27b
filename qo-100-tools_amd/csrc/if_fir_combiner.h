// if_fir_combiner.h — internal interface between the channel combiner's C-ABI shim and its HIP kernels (not installed).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "if_fir_combiner_tables.h"
#include "if_fir_interp.h"

namespace if_fir
{

constexpr int COMBINER_MAX_CHANNELS = 64;

// what the kernels need per channel, handed over BY VALUE with the launch (1 KiB of kernel arguments): a call makes no
// allocation, copy or synchronise of its own
struct CombinerChans
{
    const void *in[COMBINER_MAX_CHANNELS];   // device, N input samples each (float32 or int16 I,Q)
    uint32_t rword[COMBINER_MAX_CHANNELS];   // the residual r of P = G 2^20 + r as a 32-bit word (two's complement)
    uint16_t G[COMBINER_MAX_CHANNELS];       // the nearest point of the 1/4096 grid, 0..4095
    uint16_t table[COMBINER_MAX_CHANNELS];   // which multiply table: 0 = the plain H (r = 0), else one per distinct residual
};

struct CombinerArgs
{
    CombinerChans ch;
    int C;
    void *out;              // device, M = N L float32 I,Q outputs
    const float2 *hist;     // device, C x hist_len: the hist_len input samples of every channel before this call (float32)
    float2 *hist_out;       // device, the other ping-pong buffer: receives the history of the next call
    int hist_len;
    const float2 *H;        // overlap-save: the multiply tables, 4096 entries each (combiner_build_table)
    const float2 *tw;       // overlap-save: W4096^i, i = 0..4095
    const float *taps;      // generic: T real floats or T interleaved complex pairs
    int T, L, ctaps, in_i16;
    int64_t N, M;
    uint32_t first_out;     // absolute index of this call's first output, mod 2^32
    int grid_limit;         // at most this many workgroups (0 = the launcher's choice); same results
    int device;
    hipStream_t stream;
};

bool combiner_fft_supported(int T, int L); // L in {4, 8, 16, 32, 64} (the interpolator's small form), T <= 3073
// host: the multiply table of residual r, FFT_4096(h[k] exp(j 2 pi r k / 2^32)) / 4096: r = 0 the interpolator's H (a channel on
// the 1/4096 grid), else combiner_residual_table (if_fir_combiner_tables.h)
void combiner_build_table(const float *taps, int T, int ctaps, int32_t r, float2 *H);
hipError_t launch_combiner_fft(const CombinerArgs &a);
hipError_t launch_combiner_generic(const CombinerArgs &a);
template <int ROWS>
hipError_t launch_combiner_fft_rows(const CombinerArgs &a); // defined in the unit compiled with IF_FIR_COMBINER_ROWS = ROWS

} // namespace if_fir
