// if_fir_combiner_tables.h — the channel combiner's host arithmetic (docs/SPEC.md §9): the split of a phase word into a point of
// the 1/4096 grid and a residual, and the multiply table of a residual.  Plain C++, no HIP: the shim and if_fir_combiner.hip use
// it, and tests/c/combiner_tables_asan.cpp walks it under the sanitizers.
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

namespace if_fir
{

constexpr int COMBINER_TABLE_N = 4096; // = INTERP_N, the overlap-save block

// the phase word P = round(f 2^32) mod 2^32 split as P = G 2^20 + r (mod 2^32): G = ((P + 2^19) mod 2^32) >> 20 in 0..4095, r the
// signed rest in -2^19 .. 2^19 - 1
inline void combiner_split_word(uint32_t P, uint32_t *G, int32_t *r)
{
    *G = (uint32_t)(P + (1u << 19)) >> 20;
    *r = (int32_t)(P - (*G << 20));
}

// H[k] = FFT_4096(g)[k] / 4096 as 4096 (re, im) float pairs, g[k] = h[k] exp(j 2 pi r k / 2^32): float64 arithmetic (a radix-2
// transform, decimation in time), rounded once.  taps: T floats, or T (re, im) pairs with ctaps; 1 <= T <= 4096.
inline void combiner_residual_table(const float *taps, int T, int ctaps, int32_t r, float *H)
{
    constexpr int N = COMBINER_TABLE_N, LOG_N = 12;
    const double two_pi = 6.283185307179586476925286766559;
    std::vector<double> re(N, 0.0), im(N, 0.0), wc(N / 2), ws(N / 2);
    for (int i = 0; i < N / 2; i++)
    {
        wc[i] = cos(two_pi * i / N);
        ws[i] = -sin(two_pi * i / N);
    }
    for (int t = 0; t < T && t < N; t++)
    {
        const double hr = ctaps ? taps[2 * t] : taps[t], hi = ctaps ? taps[2 * t + 1] : 0.0;
        const double ang = two_pi * ((double)r * (double)t) / 4294967296.0; // r t is an integer below 2^31: exact
        const double c = cos(ang), s = sin(ang);
        unsigned rev = 0;
        for (int b = 0; b < LOG_N; b++)
            rev |= (((unsigned)t >> b) & 1u) << (LOG_N - 1 - b);
        re[rev] = hr * c - hi * s;
        im[rev] = hr * s + hi * c;
    }
    for (int len = 2; len <= N; len <<= 1)
    {
        const int half = len / 2, step = N / len;
        for (int base = 0; base < N; base += len)
            for (int k = 0; k < half; k++)
            {
                const double c = wc[k * step], s = ws[k * step];
                const int i0 = base + k, i1 = i0 + half;
                const double tr = re[i1] * c - im[i1] * s, ti = re[i1] * s + im[i1] * c;
                re[i1] = re[i0] - tr;
                im[i1] = im[i0] - ti;
                re[i0] += tr;
                im[i0] += ti;
            }
    }
    for (int k = 0; k < N; k++)
    {
        H[2 * k] = (float)(re[k] / N);
        H[2 * k + 1] = (float)(im[k] / N);
    }
}

} // namespace if_fir
