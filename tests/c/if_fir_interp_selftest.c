/* The interpolator's C ABI from plain C99 (tests/test_interp_gpu.py compiles and runs it): 63 taps, L = 4, one call through
 * if_fir_interp_process against a direct evaluation of the definition in double precision (docs/SPEC.md §6). */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include "if_fir.h"

#define T 63
#define L 4
#define N 5000

int main(void)
{
    float h[T], x[2 * N];
    static float y[2 * N * L];
    if_fir_interp_t *ctx = NULL;
    uint64_t m = 0;
    double err = 0.0, peak = 0.0;
    int i, k;
    if (!if_bpf_design(h, T, 0.0, 0.1, IF_BPF_WINDOW_BLACKMAN))
        return printf("if_bpf_design failed\n"), 1;
    for (i = 0; i < T; i++)
        h[i] *= (float)L;
    for (i = 0; i < 2 * N; i++)
        x[i] = (float)sin(0.001 * i * i) * 0.5f;
    if (!if_fir_interp_init(&ctx, h, T, L, N, 0))
        return printf("init: %s\n", if_fir_interp_last_error(NULL)), 1;
    if (if_fir_interp_get_backend(ctx) != IF_FIR_BACKEND_HIP_FFT)
        return printf("AUTO did not pick the overlap-save backend\n"), 1;
    if (if_fir_interp_set_backend(ctx, IF_FIR_BACKEND_HIP_DIRECT) || !*if_fir_interp_last_error(ctx))
        return printf("the direct backend was not refused\n"), 1;
    if (!if_fir_interp_process(ctx, x, y, N, &m) || m != (uint64_t)N * L)
        return printf("process: %s\n", if_fir_interp_last_error(ctx)), 1;
    for (i = 0; i < N * L; i++)
    {
        double re = 0.0, im = 0.0;
        for (k = i % L; k < T && k <= i; k += L)
        {
            re += h[k] * (double)x[2 * ((i - k) / L)];
            im += h[k] * (double)x[2 * ((i - k) / L) + 1];
        }
        err = fmax(err, fmax(fabs(y[2 * i] - re), fabs(y[2 * i + 1] - im)));
        peak = fmax(peak, fmax(fabs(re), fabs(im)));
    }
    if_fir_interp_destroy(ctx);
    if (!(err <= 1e-6 * peak))
        return printf("max error %g of peak %g\n", err, peak), 1;
    printf("interpolated %llu outputs, max error %.3g of peak %.3g: all checks passed\n", (unsigned long long)m, err, peak);
    return 0;
}
