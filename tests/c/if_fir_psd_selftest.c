/* The power-spectrum estimator's C ABI from plain C99 (tests/test_psd_c_abi.py compiles and runs it): N = 256, H = 128, K = 3,
 * 100 bins from -30, the default window; a stream fed in two calls through if_fir_psd_process against a direct evaluation of
 * the definition in double precision (docs/SPEC.md §8), codes within one of the mapping of the returned power. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include "if_fir.h"

#define N 256
#define H 128
#define K 3
#define FIRST (-30)
#define BINS 100
#define FRAMES 2
#define SAMPLES ((FRAMES * K - 1) * H + N + 50)
#define CUT 301
#define PI 3.14159265358979323846

int main(void)
{
    static float x[2 * SAMPLES], power[FRAMES * BINS];
    static uint16_t codes[FRAMES * BINS];
    static double w[N];
    if_fir_psd_config_t cfg = {N, H, K, FIRST, BINS, 0.5f, IF_FIR_INPUT_F32};
    if_fir_psd_config_t bad;
    if_fir_psd_t *ctx = NULL;
    uint32_t f1 = 7, f2 = 7;
    double energy = 0.0, err = 0.0, peak = 0.0;
    long i, f, s, j, n;
    for (i = 0; i < SAMPLES; i++)
    {
        x[2 * i] = (float)(0.4 * cos(2.0 * PI * 10.0 / N * i) + 0.1 * sin(0.0007 * i * i));
        x[2 * i + 1] = (float)(0.4 * sin(2.0 * PI * 10.0 / N * i) + 0.1 * cos(0.0011 * i * i));
    }
    for (i = 0; i < N; i++)
    {
        w[i] = (double)(float)(0.5 - 0.5 * cos(2.0 * PI * i / N));
        energy += w[i] * w[i];
    }
    bad = cfg;
    bad.ulSize = 300;
    if (if_fir_psd_init(&ctx, &bad, NULL, SAMPLES, 0) || ctx || !*if_fir_psd_last_error(NULL))
        return printf("size 300 was not refused\n"), 1;
    bad = cfg;
    bad.ulHop = 0;
    if (if_fir_psd_init(&ctx, &bad, NULL, SAMPLES, 0) || ctx)
        return printf("hop 0 was not refused\n"), 1;
    bad = cfg;
    bad.lFirstBin = 100;
    if (if_fir_psd_init(&ctx, &bad, NULL, SAMPLES, 0) || ctx)
        return printf("bins past N/2 were not refused\n"), 1;
    if (!if_fir_psd_init(&ctx, &cfg, NULL, SAMPLES, 0))
        return printf("init: %s\n", if_fir_psd_last_error(NULL)), 1;
    if (if_fir_psd_process(ctx, x, SAMPLES + 1, codes, power, &f1) || !*if_fir_psd_last_error(ctx))
        return printf("a call above ullMaxSamples was not refused\n"), 1;
    if (!if_fir_psd_process(ctx, x, 0, codes, power, &f1) || f1 != 0)
        return printf("an empty call: %s\n", if_fir_psd_last_error(ctx)), 1;
    if (if_fir_psd_frame_count(ctx, SAMPLES) != FRAMES || if_fir_psd_frame_count(ctx, CUT) != 0)
        return printf("frame_count from the start\n"), 1;
    if (!if_fir_psd_process(ctx, x, CUT, codes, power, &f1) || f1 != 0)
        return printf("process 1: %s\n", if_fir_psd_last_error(ctx)), 1;
    if (if_fir_psd_frame_count(ctx, SAMPLES - CUT) != FRAMES)
        return printf("frame_count after the cut\n"), 1;
    if (!if_fir_psd_process(ctx, x + 2 * CUT, SAMPLES - CUT, codes, power, &f2) || f2 != FRAMES)
        return printf("process 2: %s (%u frames)\n", if_fir_psd_last_error(ctx), f2), 1;
    for (f = 0; f < FRAMES; f++)
        for (j = 0; j < BINS; j++)
        {
            const long k = ((FIRST + j) % N + N) % N;
            double p = 0.0, db, code;
            for (s = f * K; s < (f + 1) * K; s++)
            {
                double re = 0.0, im = 0.0;
                for (n = 0; n < N; n++)
                {
                    const double a = -2.0 * PI * (double)((k * n) % N) / N, c = cos(a), d = sin(a);
                    const double xr = w[n] * x[2 * (s * H + n)], xi = w[n] * x[2 * (s * H + n) + 1];
                    re += xr * c - xi * d;
                    im += xr * d + xi * c;
                }
                p += re * re + im * im;
            }
            p /= K * energy;
            err = fmax(err, fabs(power[f * BINS + j] - p));
            peak = fmax(peak, p);
            db = 10.0 * log10((double)power[f * BINS + j] / 0.5);
            code = fmin(fmax(rint((db + 3.35) / ((16.7 + 3.35) / 65535)), 0.0), 65535.0);
            if (fabs((double)codes[f * BINS + j] - code) > 1.0)
                return printf("frame %ld bin %ld: code %u, the mapping of its power gives %.0f\n", f, j, codes[f * BINS + j], code), 1;
        }
    if (!(err <= 1e-5 * peak))
        return printf("power error %g of peak %g\n", err, peak), 1;
    if (!if_fir_psd_reset(ctx) || if_fir_psd_frame_count(ctx, SAMPLES) != FRAMES)
        return printf("reset: %s\n", if_fir_psd_last_error(ctx)), 1;
    if (!if_fir_psd_set_input_format(ctx, IF_FIR_INPUT_I16) || if_fir_psd_set_input_format(ctx, 9))
        return printf("set_input_format\n"), 1;
    if (!if_fir_psd_synchronize(ctx))
        return printf("synchronize: %s\n", if_fir_psd_last_error(ctx)), 1;
    if_fir_psd_destroy(ctx);
    printf("power error %.3g of peak %.3g\nall checks passed\n", err, peak);
    return 0;
}
