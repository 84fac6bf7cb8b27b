// if_fir_interp.h — internal interface between the interpolator's C-ABI shim and its HIP kernels (not installed).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace if_fir
{

constexpr int INTERP_N = 4096;        // overlap-save block: output-rate points
constexpr int INTERP_MAX_L = 64;
constexpr int INTERP_FFT_MAX_TAPS = 3073; // one partition: 48 overlap rows

struct InterpArgs
{
    const void *in;         // device, N input samples (float32 or int16 I,Q)
    void *out;              // device, M = N L float32 I,Q outputs
    const float2 *hist;     // device, the hist_len input samples before this call (float32, most recent last)
    float2 *hist_out;       // device, the other ping-pong buffer: receives the history of the next call
    int hist_len;
    const float2 *H;        // overlap-save: FFT_4096(taps) / 4096 (interp_build_table)
    const float2 *tw;       // overlap-save: W4096^i, i = 0..4095
    const float *taps;      // generic: T real floats or T interleaved complex pairs
    int T, L, ctaps, in_i16;
    int64_t N, M;
    uint32_t nco_word;      // up-mix: output n is rotated by exp(+j 2 pi nco_word n / 2^32), n = absolute output index
    uint32_t nco_phi0;      // nco_word * (absolute index of this call's first output) mod 2^32
    int full;               // overlap-save: the 4096-point forward transform of the zero-stuffed block for every L
    int grid_limit;         // at most this many workgroups (0 = the launcher's choice); same results
    int device;
    hipStream_t stream;
};

bool interp_fft_supported(int T, int L);
int interp_overlap_rows(int T);           // 4, 8, 16, 32 or 48: the smallest overlap of 64 ROWS outputs >= T - 1
int interp_hist_len(int T, int L);        // input samples of history a context keeps
// host: the multiply table H[k] = sum_t h[t] W4096^(k t) / 4096 (float64 arithmetic, rounded once) and the twiddles W4096^i
void interp_build_tables(const float *taps, int T, int ctaps, float2 *H, float2 *tw);
hipError_t launch_interp_fft(const InterpArgs &a);
hipError_t launch_interp_generic(const InterpArgs &a);
template <int ROWS>
hipError_t launch_interp_fft_rows(const InterpArgs &a); // defined in the unit compiled with IF_FIR_INTERP_ROWS = ROWS

} // namespace if_fir
