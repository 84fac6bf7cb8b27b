/* The channel combiner's C ABI from plain C99 (tests/test_combiner_c_abi.py compiles and runs it): 63 taps, L = 4, three
 * channels at off-grid centres, one call through if_fir_combiner_process against a direct evaluation of the definition in double
 * precision (docs/SPEC.md §9), and the refusals. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include "if_fir.h"

#define T 63
#define L 4
#define C 3
#define N 5000

static const double PI2 = 6.283185307179586476925286766559;

int main(void)
{
    static float h[T], x[C][2 * N], y[2 * N * L];
    const double centre[C] = {0.2003, -0.3107, 37.0 / 4096.0}, bad_centre[C] = {0.2003, 0.6, 0.0};
    double got[C], err = 0.0, peak = 0.0;
    const void *in[C];
    if_fir_combiner_t *ctx = NULL;
    uint64_t m = 0;
    int i, k, c;
    if (!if_bpf_design(h, T, 0.0, 0.1, IF_BPF_WINDOW_BLACKMAN))
        return printf("if_bpf_design failed\n"), 1;
    for (i = 0; i < T; i++)
        h[i] *= (float)L;
    h[0] = 1.0f; /* loud at both ends: a boundary off by one shows */
    h[T - 1] = -1.0f;
    for (c = 0; c < C; c++)
    {
        for (i = 0; i < 2 * N; i++)
            x[c][i] = (float)sin(0.001 * (c + 1) * i * i + c) * 0.5f;
        in[c] = x[c];
    }
    if (if_fir_combiner_init(&ctx, h, T, L, 0, centre, N, 0) || ctx || !*if_fir_combiner_last_error(NULL))
        return printf("0 channels were not refused\n"), 1;
    if (if_fir_combiner_init(&ctx, h, T, L, IF_FIR_COMBINER_MAX_CHANNELS + 1, centre, N, 0) || ctx)
        return printf("65 channels were not refused\n"), 1;
    if (if_fir_combiner_init(&ctx, h, T, L, C, bad_centre, N, 0) || ctx)
        return printf("a centre of 0.6 was not refused\n"), 1;
    if (!if_fir_combiner_init(&ctx, h, T, L, C, centre, N, 0))
        return printf("init: %s\n", if_fir_combiner_last_error(NULL)), 1;
    if (if_fir_combiner_get_backend(ctx) != IF_FIR_BACKEND_HIP_FFT)
        return printf("AUTO did not pick the overlap-save backend\n"), 1;
    if (if_fir_combiner_set_backend(ctx, IF_FIR_BACKEND_HIP_DIRECT) || !*if_fir_combiner_last_error(ctx))
        return printf("the direct backend was not refused\n"), 1;
    if (if_fir_combiner_set_centres(ctx, bad_centre) || !if_fir_combiner_get_centres(ctx, got))
        return printf("set_centres took a centre of 0.6\n"), 1;
    for (c = 0; c < C; c++)
        if (fabs(got[c] - centre[c]) > 1.0 / 4294967296.0)
            return printf("centre %d reads back as %.12g\n", c, got[c]), 1;
    if (if_fir_combiner_process(ctx, in, y, N + 1, &m) || !*if_fir_combiner_last_error(ctx))
        return printf("a call beyond ullMaxSamples was not refused\n"), 1;
    if (if_fir_combiner_out_count(ctx, N) != (uint64_t)N * L)
        return printf("out_count\n"), 1;
    if (!if_fir_combiner_process(ctx, in, y, N, &m) || m != (uint64_t)N * L)
        return printf("process: %s\n", if_fir_combiner_last_error(ctx)), 1;
    for (i = 0; i < N * L; i++)
    {
        double sr = 0.0, si = 0.0;
        for (c = 0; c < C; c++)
        {
            double re = 0.0, im = 0.0, ph, cs, sn;
            for (k = i % L; k < T && k <= i; k += L)
            {
                re += h[k] * (double)x[c][2 * ((i - k) / L)];
                im += h[k] * (double)x[c][2 * ((i - k) / L) + 1];
            }
            ph = fmod(got[c] * (double)i, 1.0); /* the quantised centre times n: exact in double at these sizes */
            cs = cos(PI2 * ph);
            sn = sin(PI2 * ph);
            sr += re * cs - im * sn;
            si += re * sn + im * cs;
        }
        err = fmax(err, fmax(fabs(y[2 * i] - sr), fabs(y[2 * i + 1] - si)));
        peak = fmax(peak, fmax(fabs(sr), fabs(si)));
    }
    if_fir_combiner_destroy(ctx);
    if (!(err <= 1e-6 * peak))
        return printf("max error %g of peak %g\n", err, peak), 1;
    printf("combined %d channels into %llu outputs, max error %.3g of peak %.3g: all checks passed\n", C, (unsigned long long)m, err, peak);
    return 0;
}
