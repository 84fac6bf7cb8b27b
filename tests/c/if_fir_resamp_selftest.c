/* The resampler's C ABI from plain C99 (tests/test_resamp_c_abi.py compiles and runs it): 95 taps, L/M = 3/4, a stream fed in
 * two calls through if_fir_resamp_process against a direct evaluation of the definition in double precision (docs/SPEC.md §7):
 * y[m] = sum_k h[k] u[m M - k], u[n] = x[n / L] where L divides n. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include "if_fir.h"

#define T 95
#define L 3
#define M 4
#define N 5000
#define CUT 1667
#define OUT ((N * L + M - 1) / M)

int main(void)
{
    float h[T];
    static float x[2 * N], y[2 * OUT + 2];
    if_fir_resamp_t *ctx = NULL;
    uint64_t m1 = 0, m2 = 0, want;
    double err = 0.0, peak = 0.0;
    long i, k;
    if (!if_bpf_design(h, T, 0.0, 0.45 / M, IF_BPF_WINDOW_BLACKMAN))
        return printf("if_bpf_design failed\n"), 1;
    for (i = 0; i < T; i++)
        h[i] *= (float)L;
    for (i = 0; i < 2 * N; i++)
        x[i] = (float)sin(0.001 * i * i) * 0.5f;
    if (if_fir_resamp_init(&ctx, h, T, 0, M, N, 0) || ctx || !*if_fir_resamp_last_error(NULL))
        return printf("interpolation 0 was not refused\n"), 1;
    if (if_fir_resamp_init(&ctx, h, T, L, 65, N, 0) || ctx)
        return printf("decimation 65 was not refused\n"), 1;
    if (!if_fir_resamp_init(&ctx, h, T, L, M, N, 0))
        return printf("init: %s\n", if_fir_resamp_last_error(NULL)), 1;
    if (if_fir_resamp_process(ctx, x, y, N + 1, &m1) || !*if_fir_resamp_last_error(ctx))
        return printf("a call above ullMaxSamples was not refused\n"), 1;
    if (!if_fir_resamp_process(ctx, x, y, 0, &m1) || m1 != 0)
        return printf("an empty call: %s\n", if_fir_resamp_last_error(ctx)), 1;
    want = if_fir_resamp_out_count(ctx, CUT);
    if (!if_fir_resamp_process(ctx, x, y, CUT, &m1) || m1 != want || m1 != (CUT * L + M - 1) / M)
        return printf("process 1: %s\n", if_fir_resamp_last_error(ctx)), 1;
    want = if_fir_resamp_out_count(ctx, N - CUT);
    if (!if_fir_resamp_process(ctx, x + 2 * CUT, y + 2 * m1, N - CUT, &m2) || m2 != want || m1 + m2 != OUT)
        return printf("process 2: %s (%llu + %llu outputs)\n", if_fir_resamp_last_error(ctx), (unsigned long long)m1,
                      (unsigned long long)m2), 1;
    for (i = 0; i < OUT; i++)
    {
        double re = 0.0, im = 0.0;
        for (k = (i * M) % L; k < T && k <= i * M; k += L)
        {
            re += h[k] * (double)x[2 * ((i * M - k) / L)];
            im += h[k] * (double)x[2 * ((i * M - k) / L) + 1];
        }
        err = fmax(err, fmax(fabs(y[2 * i] - re), fabs(y[2 * i + 1] - im)));
        peak = fmax(peak, fmax(fabs(re), fabs(im)));
    }
    if (!if_fir_resamp_reset(ctx) || if_fir_resamp_out_count(ctx, N) != OUT)
        return printf("reset: %s\n", if_fir_resamp_last_error(ctx)), 1;
    if_fir_resamp_destroy(ctx);
    if (!(err <= 1e-6 * peak))
        return printf("max error %g of peak %g\n", err, peak), 1;
    printf("resampled %d inputs to %llu outputs, max error %.3g of peak %.3g: all checks passed\n", N,
           (unsigned long long)(m1 + m2), err, peak);
    return 0;
}
