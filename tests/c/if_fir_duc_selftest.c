/* The up-converter's C ABI from plain C99 (tests/test_duc_c_abi.py compiles and runs it): 255 taps, interpolation 16, an NCO at
 * 0.2 cycles/sample, a complex stream fed in two calls through if_fir_duc_process, in both output formats, against a direct
 * evaluation of the definition in double precision (docs/SPEC.md §11):
 * y[m] = Re{ exp(+j 2 pi ((P m) mod 2^32) / 2^32) sum_{k = m mod L, step L} h[k] x[(m - k) / L] }. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include "if_fir.h"

#define T 255
#define L 16
#define N 2000
#define CUT 667
#define OUT (N * L)

static const double two_pi = 6.283185307179586476925286766559;

/* the definition into ref; returns its peak */
static double definition(const float *h, const float *x, uint32_t word, double *ref)
{
    double peak = 0.0;
    long i, k;
    for (i = 0; i < OUT; i++)
    {
        double re = 0.0, im = 0.0;
        const double ph = two_pi * ((double)(uint32_t)(word * (uint32_t)i) / 4294967296.0);
        for (k = i % L; k < T && k <= i; k += L)
        {
            re += h[k] * (double)x[2 * ((i - k) / L)];
            im += h[k] * (double)x[2 * ((i - k) / L) + 1];
        }
        ref[i] = re * cos(ph) - im * sin(ph);
        peak = fmax(peak, fabs(ref[i]));
    }
    return peak;
}

int main(void)
{
    float h[T];
    static float x[2 * N], y[OUT + 2];
    static int16_t y16[OUT + 2];
    static double ref[OUT];
    if_fir_duc_t *ctx = NULL;
    uint64_t m1 = 0, m2 = 0;
    double err = 0.0, peak = 0.0, f = 0.0, scale;
    uint32_t word;
    long i, k, lsb = 0;
    if (!if_bpf_design(h, T, 0.0, 0.45 / L, IF_BPF_WINDOW_BLACKMAN))
        return printf("if_bpf_design failed\n"), 1;
    for (i = 0; i < N; i++)
    {
        x[2 * i] = (float)(sin(two_pi * 0.05 * i + 1e-6 * i * i) * 0.5);
        x[2 * i + 1] = (float)(cos(0.0013 * i * i) * 0.4);
    }
    word = (uint32_t)llround(0.2 * 4294967296.0);
    peak = definition(h, x, word, ref);
    /* taps of gain 0.9 / peak: the int16 output then peaks at 0.9 of full scale */
    scale = 0.9 / peak;
    for (k = 0; k < T; k++)
        h[k] = (float)(h[k] * scale);
    peak = definition(h, x, word, ref);
    if (if_fir_duc_init(&ctx, h, T, 0, N, 0) || ctx || !*if_fir_duc_last_error(NULL))
        return printf("interpolation 0 was not refused\n"), 1;
    if (if_fir_duc_init(&ctx, h, T, 65, N, 0) || ctx)
        return printf("interpolation 65 was not refused\n"), 1;
    if (if_fir_duc_init(&ctx, h, 4097, L, N, 0) || ctx)
        return printf("4097 taps were not refused\n"), 1;
    if (!if_fir_duc_init(&ctx, h, T, L, N, 0))
        return printf("init: %s\n", if_fir_duc_last_error(NULL)), 1;
    if (if_fir_duc_set_nco(ctx, 0.6) || !*if_fir_duc_last_error(ctx))
        return printf("a frequency of 0.6 was not refused\n"), 1;
    if (if_fir_duc_set_output_format(ctx, 2) || if_fir_duc_set_input_format(ctx, 2))
        return printf("an unknown format was not refused\n"), 1;
    if (!if_fir_duc_set_nco(ctx, 0.2) || !if_fir_duc_get_nco(ctx, &f))
        return printf("set_nco: %s\n", if_fir_duc_last_error(ctx)), 1;
    if (f != (double)word / 4294967296.0)
        return printf("get_nco returned %.17g\n", f), 1;
    if (if_fir_duc_process(ctx, x, y, N + 1, &m1) || !*if_fir_duc_last_error(ctx))
        return printf("a call above ullMaxSamples was not refused\n"), 1;
    if (if_fir_duc_process(ctx, NULL, y, 10, &m1) || if_fir_duc_process(ctx, x, NULL, 10, &m1))
        return printf("a NULL buffer was not refused\n"), 1;
    if (!if_fir_duc_process(ctx, x, y, 0, &m1) || m1 != 0)
        return printf("an empty call: %s\n", if_fir_duc_last_error(ctx)), 1;
    if (if_fir_duc_out_count(ctx, CUT) != (uint64_t)CUT * L)
        return printf("out_count\n"), 1;
    /* float32 output, two calls */
    if (!if_fir_duc_process(ctx, x, y, CUT, &m1) || m1 != (uint64_t)CUT * L)
        return printf("process 1: %s\n", if_fir_duc_last_error(ctx)), 1;
    if (!if_fir_duc_process(ctx, x + 2 * CUT, y + m1, N - CUT, &m2) || m1 + m2 != OUT)
        return printf("process 2: %s (%llu + %llu outputs)\n", if_fir_duc_last_error(ctx), (unsigned long long)m1,
                      (unsigned long long)m2), 1;
    for (i = 0; i < OUT; i++)
        err = fmax(err, fabs(y[i] - ref[i]));
    /* int16 output of the same stream, the format switched at the cut of a second pass: the first part again as float32 */
    if (!if_fir_duc_reset(ctx))
        return printf("reset: %s\n", if_fir_duc_last_error(ctx)), 1;
    if (!if_fir_duc_process(ctx, x, y, CUT, &m1) || !if_fir_duc_set_output_format(ctx, IF_FIR_OUTPUT_I16) ||
        !if_fir_duc_process(ctx, x + 2 * CUT, y16 + m1, N - CUT, &m2) || m1 + m2 != OUT)
        return printf("int16 pass: %s\n", if_fir_duc_last_error(ctx)), 1;
    for (i = (long)m1; i < OUT; i++)
    {
        const long want = lrint(ref[i] * 32768.0), d = labs((long)y16[i] - want);
        lsb = d > lsb ? d : lsb;
        /* the same float32 result, rounded: exactly */
        if (y16[i] != (int16_t)lrintf(y[i] * 32768.0f))
            return printf("int16 output %ld is %d, the float32 one %.9g\n", i, y16[i], y[i]), 1;
    }
    if_fir_duc_destroy(ctx);
    if (!(err <= 1e-6 * peak))
        return printf("max error %g of peak %g\n", err, peak), 1;
    if (lsb > 1)
        return printf("int16 output %ld LSB from the reference\n", lsb), 1;
    printf("up-converted %d samples to %llu outputs, max error %.3g of peak %.3g, int16 within %ld LSB: all checks passed\n", N,
           (unsigned long long)(m1 + m2), err, peak, lsb);
    return 0;
}
