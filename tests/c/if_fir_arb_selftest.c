/* The arbitrary-ratio resampler's C ABI from plain C99 (tests/test_arb_c_abi.py compiles and runs it): 1537 taps at P = 64
 * phases, a step from if_fir_arb_step_from_rates, a stream fed in two calls through if_fir_arb_process with a retune between
 * them, against a direct evaluation of the definition in double precision with the time kept in integers (docs/SPEC.md §12):
 * q = tau >> 32, f = tau mod 2^32, p = f >> 26, mu = (f mod 2^26) / 2^26,
 * y = sum_j [(1 - mu) h[p + j P] + mu h[p + 1 + j P]] x[q - j], tau += R. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include "if_fir.h"

#define T 1537
#define BITS 6
#define P (1 << BITS)
#define K ((T + P - 1) / P)
#define N 5000
#define CUT 1667
#define MAXOUT (2 * N)

static double tap(const float *h, long k)
{
    return k < T ? (double)h[k] : 0.0;
}

int main(void)
{
    static float h[T], x[2 * N], y[2 * MAXOUT];
    if_fir_arb_t *ctx = NULL;
    uint64_t m1 = 0, m2 = 0, want, tau = 0, r1, r2, total;
    double err = 0.0, peak = 0.0;
    long i, j;
    if (!if_bpf_design(h, T, 0.0, 0.45 / P, IF_BPF_WINDOW_BLACKMAN))
        return printf("if_bpf_design failed\n"), 1;
    for (i = 0; i < T; i++)
        h[i] *= (float)P;
    for (i = 0; i < 2 * N; i++)
        x[i] = (float)sin(0.001 * i * i) * 0.5f;
    r1 = if_fir_arb_step_from_rates(1.0e6, 2.0 * 333.0e3); /* three samples per symbol of 333 kBd become two */
    r2 = if_fir_arb_step_from_rates(1.0e6, 2.0 * 333.0e3 * 1.000003);
    if (r1 != (uint64_t)llrint(1.0e6 / 666.0e3 * 4294967296.0) || r2 == 0 || r2 >= r1 || if_fir_arb_step_from_rates(65.0, 1.0) ||
        if_fir_arb_step_from_rates(1.0, 65.0))
        return printf("if_fir_arb_step_from_rates: %llu %llu\n", (unsigned long long)r1, (unsigned long long)r2), 1;
    if (if_fir_arb_init(&ctx, h, T, 3, r1, N, 0) || ctx || !*if_fir_arb_last_error(NULL))
        return printf("3 phase bits were not refused\n"), 1;
    if (if_fir_arb_init(&ctx, h, T, BITS, ((uint64_t)1 << 34) + 1, N, 0) || ctx)
        return printf("a step above 4 was not refused\n"), 1;
    if (if_fir_arb_init(&ctx, h, IF_FIR_ARB_MAX_TAPS + 1, BITS, r1, N, 0) || ctx)
        return printf("8193 taps were not refused\n"), 1;
    if (!if_fir_arb_init(&ctx, h, T, BITS, r1, N, 0))
        return printf("init: %s\n", if_fir_arb_last_error(NULL)), 1;
    if (if_fir_arb_process(ctx, x, y, N + 1, &m1) || !*if_fir_arb_last_error(ctx))
        return printf("a call above ullMaxSamples was not refused\n"), 1;
    if (if_fir_arb_set_step(ctx, 1) || !*if_fir_arb_last_error(ctx))
        return printf("a step of 1 was not refused\n"), 1;
    if (!if_fir_arb_process(ctx, x, y, 0, &m1) || m1 != 0)
        return printf("an empty call: %s\n", if_fir_arb_last_error(ctx)), 1;
    want = if_fir_arb_out_count(ctx, CUT);
    if (!if_fir_arb_process(ctx, x, y, CUT, &m1) || m1 != want || m1 != (((uint64_t)CUT << 32) + r1 - 1) / r1)
        return printf("process 1: %s\n", if_fir_arb_last_error(ctx)), 1;
    if (!if_fir_arb_set_step(ctx, r2))
        return printf("set_step: %s\n", if_fir_arb_last_error(ctx)), 1;
    want = if_fir_arb_out_count(ctx, N - CUT);
    if (!if_fir_arb_process(ctx, x + 2 * CUT, y + 2 * m1, N - CUT, &m2) || m2 != want || m1 + m2 > MAXOUT)
        return printf("process 2: %s (%llu + %llu outputs)\n", if_fir_arb_last_error(ctx), (unsigned long long)m1,
                      (unsigned long long)m2), 1;
    total = m1 + m2;
    for (i = 0; i < (long)total; i++)
    {
        const long q = (long)(tau >> 32), p = (long)((tau & 0xffffffffu) >> (32 - BITS));
        const double mu = (double)(tau & ((1u << (32 - BITS)) - 1u)) / (double)(1u << (32 - BITS));
        double re = 0.0, im = 0.0;
        for (j = 0; j < K && j <= q; j++)
        {
            const double g = (1.0 - mu) * tap(h, p + j * P) + mu * tap(h, p + 1 + j * P);
            re += g * (double)x[2 * (q - j)];
            im += g * (double)x[2 * (q - j) + 1];
        }
        if (q >= N)
            return printf("output %ld lies past the stream\n", i), 1;
        err = fmax(err, fmax(fabs(y[2 * i] - re), fabs(y[2 * i + 1] - im)));
        peak = fmax(peak, fmax(fabs(re), fabs(im)));
        tau += (uint64_t)i < m1 ? r1 : r2;
    }
    if ((tau >> 32) < N)
        return printf("an output of the stream was left behind\n"), 1;
    if (!if_fir_arb_reset(ctx) || if_fir_arb_out_count(ctx, N) != (((uint64_t)N << 32) + r2 - 1) / r2)
        return printf("reset: %s\n", if_fir_arb_last_error(ctx)), 1;
    if_fir_arb_destroy(ctx);
    if (!(err <= 1e-6 * peak))
        return printf("max error %g of peak %g\n", err, peak), 1;
    printf("resampled %d inputs to %llu outputs, max error %.3g of peak %.3g: all checks passed\n", N, (unsigned long long)total, err,
           peak);
    return 0;
}
