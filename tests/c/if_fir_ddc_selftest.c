/* The down-converter's C ABI from plain C99 (tests/test_ddc_c_abi.py compiles and runs it): 255 taps, decimation 16, an NCO at
 * 0.2 cycles/sample, a real stream fed in two calls through if_fir_ddc_process against a direct evaluation of the definition
 * in double precision (docs/SPEC.md §10): y[m] = sum_k h[k] r[m D - k] exp(-j 2 pi ((P (m D - k)) mod 2^32) / 2^32). */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include "if_fir.h"

#define T 255
#define D 16
#define N 20000
#define CUT 6667
#define OUT ((N + D - 1) / D)

int main(void)
{
    float h[T];
    static float r[N], y[2 * OUT + 2];
    if_fir_ddc_t *ctx = NULL;
    uint64_t m1 = 0, m2 = 0, want;
    double err = 0.0, peak = 0.0, f = 0.0;
    const double two_pi = 6.283185307179586476925286766559;
    uint32_t word;
    long i, k;
    if (!if_bpf_design(h, T, 0.0, 0.45 / D, IF_BPF_WINDOW_BLACKMAN))
        return printf("if_bpf_design failed\n"), 1;
    for (i = 0; i < N; i++)
        r[i] = (float)(sin(two_pi * 0.2 * i + 1e-7 * i * i) * 0.5 + sin(0.001 * i * i) * 0.25);
    if (if_fir_ddc_init(&ctx, h, T, 0, N, 0) || ctx || !*if_fir_ddc_last_error(NULL))
        return printf("decimation 0 was not refused\n"), 1;
    if (if_fir_ddc_init(&ctx, h, 4097, D, N, 0) || ctx)
        return printf("4097 taps were not refused\n"), 1;
    if (!if_fir_ddc_init(&ctx, h, T, D, N, 0))
        return printf("init: %s\n", if_fir_ddc_last_error(NULL)), 1;
    if (if_fir_ddc_set_nco(ctx, 0.6) || !*if_fir_ddc_last_error(ctx))
        return printf("a frequency of 0.6 was not refused\n"), 1;
    if (!if_fir_ddc_set_nco(ctx, 0.2) || !if_fir_ddc_get_nco(ctx, &f))
        return printf("set_nco: %s\n", if_fir_ddc_last_error(ctx)), 1;
    word = (uint32_t)llround(0.2 * 4294967296.0);
    if (f != (double)word / 4294967296.0)
        return printf("get_nco returned %.17g\n", f), 1;
    if (if_fir_ddc_process(ctx, r, y, N + 1, &m1) || !*if_fir_ddc_last_error(ctx))
        return printf("a call above ullMaxSamples was not refused\n"), 1;
    if (!if_fir_ddc_process(ctx, r, y, 0, &m1) || m1 != 0)
        return printf("an empty call: %s\n", if_fir_ddc_last_error(ctx)), 1;
    want = if_fir_ddc_out_count(ctx, CUT);
    if (!if_fir_ddc_process(ctx, r, y, CUT, &m1) || m1 != want || m1 != (CUT + D - 1) / D)
        return printf("process 1: %s\n", if_fir_ddc_last_error(ctx)), 1;
    want = if_fir_ddc_out_count(ctx, N - CUT);
    if (!if_fir_ddc_process(ctx, r + CUT, y + 2 * m1, N - CUT, &m2) || m2 != want || m1 + m2 != OUT)
        return printf("process 2: %s (%llu + %llu outputs)\n", if_fir_ddc_last_error(ctx), (unsigned long long)m1,
                      (unsigned long long)m2), 1;
    for (i = 0; i < OUT; i++)
    {
        double re = 0.0, im = 0.0;
        for (k = 0; k < T && k <= i * D; k++)
        {
            const uint32_t a = (uint32_t)(i * D - k);
            const double ph = two_pi * ((double)(uint32_t)(word * a) / 4294967296.0);
            re += h[k] * (double)r[i * D - k] * cos(ph);
            im -= h[k] * (double)r[i * D - k] * sin(ph);
        }
        err = fmax(err, fmax(fabs(y[2 * i] - re), fabs(y[2 * i + 1] - im)));
        peak = fmax(peak, fmax(fabs(re), fabs(im)));
    }
    if (!if_fir_ddc_reset(ctx) || if_fir_ddc_out_count(ctx, N) != OUT)
        return printf("reset: %s\n", if_fir_ddc_last_error(ctx)), 1;
    if_fir_ddc_destroy(ctx);
    if (!(err <= 1e-6 * peak))
        return printf("max error %g of peak %g\n", err, peak), 1;
    printf("down-converted %d real samples to %llu outputs, max error %.3g of peak %.3g: all checks passed\n", N,
           (unsigned long long)(m1 + m2), err, peak);
    return 0;
}
