/* The frame power stage's C ABI from plain C99 (tests/test_fpow_c_abi.py compiles and runs it): frames of 37 elements, output
 * bins of 3 elements from element 2 on, K = 5; a stream fed in three calls through if_fir_fpow_process against a direct
 * evaluation of the definition in double precision (docs/SPEC.md §19), codes within one of the mapping of the returned power;
 * the same frames as int16 through the same context. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include "if_fir.h"

#define B 37
#define FIRST 2
#define G 3
#define BO 11
#define K 5
#define OUT 4
#define FRAMES (OUT * K + 3)
#define CUT1 7
#define CUT2 8
#define NORM 0.8125f
#define REF 0.02f

static int check(const float *power, const uint16_t *codes, const double *want, double *err)
{
    long f, j;
    for (f = 0; f < OUT; f++)
        for (j = 0; j < BO; j++)
        {
            const double p = want[f * BO + j], got = (double)power[f * BO + j];
            const double db = 10.0 * log10(got / (double)REF);
            const double code = fmin(fmax(rint((db + 3.35) / ((16.7 + 3.35) / 65535)), 0.0), 65535.0);
            *err = fmax(*err, fabs(got - p) / p);
            if (fabs((double)codes[f * BO + j] - code) > 1.0)
                return printf("frame %ld bin %ld: code %u, the mapping of its power gives %.0f\n", f, j, codes[f * BO + j], code), 1;
        }
    /* SPEC §19: (G + ceil(K / 8) + 12) 2^-24 of the value */
    if (!(*err <= (G + 1 + 12) / 16777216.0))
        return printf("power error %g of the value\n", *err), 1;
    return 0;
}

int main(void)
{
    static float x[2 * FRAMES * B], power[OUT * BO];
    static int16_t xi[2 * FRAMES * B];
    static uint16_t codes[OUT * BO];
    static double want[OUT * BO], wanti[OUT * BO];
    if_fir_fpow_config_t cfg = {B, FIRST, G, BO, K, NORM, REF, IF_FIR_INPUT_F32};
    if_fir_fpow_config_t bad;
    if_fir_fpow_t *ctx = NULL;
    uint32_t f1 = 7, f2 = 7, f3 = 7;
    double err = 0.0, erri = 0.0;
    long i, f, a, j, g;
    for (i = 0; i < 2 * FRAMES * B; i++)
    {
        x[i] = (float)(0.1 * cos(0.37 * i) + 0.05 * sin(0.0011 * i * i) + 0.02);
        xi[i] = (int16_t)lrint(3000.0 * cos(0.41 * i) + 900.0 * sin(0.0013 * i * i) + 50.0);
    }
    for (f = 0; f < OUT; f++)
        for (j = 0; j < BO; j++)
        {
            double p = 0.0, pi = 0.0;
            for (a = f * K; a < (f + 1) * K; a++)
                for (g = 0; g < G; g++)
                {
                    const long e = 2 * (a * B + FIRST + j * G + g);
                    p += (double)x[e] * x[e] + (double)x[e + 1] * x[e + 1];
                    pi += ((double)xi[e] * xi[e] + (double)xi[e + 1] * xi[e + 1]) / 1073741824.0;
                }
            want[f * BO + j] = p / (K * G * (double)NORM);
            wanti[f * BO + j] = pi / (K * G * (double)NORM);
        }
    bad = cfg;
    bad.ulBins = 8193;
    if (if_fir_fpow_init(&ctx, &bad, FRAMES, 0) || ctx || !*if_fir_fpow_last_error(NULL))
        return printf("8193 bins were not refused\n"), 1;
    bad = cfg;
    bad.ulOutBins = 12;
    if (if_fir_fpow_init(&ctx, &bad, FRAMES, 0) || ctx)
        return printf("output bins past the frame were not refused\n"), 1;
    bad = cfg;
    bad.fNorm = 0.0f;
    if (if_fir_fpow_init(&ctx, &bad, FRAMES, 0) || ctx)
        return printf("fNorm 0 was not refused\n"), 1;
    if (!if_fir_fpow_init(&ctx, &cfg, FRAMES, 0))
        return printf("init: %s\n", if_fir_fpow_last_error(NULL)), 1;
    if (if_fir_fpow_process(ctx, x, FRAMES + 1, codes, power, &f1) || !*if_fir_fpow_last_error(ctx))
        return printf("a call above ullMaxFrames was not refused\n"), 1;
    if (!if_fir_fpow_process(ctx, x, 0, codes, power, &f1) || f1 != 0)
        return printf("an empty call: %s\n", if_fir_fpow_last_error(ctx)), 1;
    if (if_fir_fpow_frame_count(ctx, FRAMES) != OUT || if_fir_fpow_frame_count(ctx, K - 1) != 0)
        return printf("frame_count from the start\n"), 1;
    if (!if_fir_fpow_process(ctx, x, CUT1, codes, power, &f1) || f1 != 1)
        return printf("process 1: %s (%u frames)\n", if_fir_fpow_last_error(ctx), f1), 1;
    if (if_fir_fpow_frame_count(ctx, CUT2) != 2)
        return printf("frame_count after the cut\n"), 1;
    if (!if_fir_fpow_process(ctx, x + 2 * CUT1 * B, CUT2, codes + f1 * BO, power + f1 * BO, &f2) || f2 != 2)
        return printf("process 2: %s (%u frames)\n", if_fir_fpow_last_error(ctx), f2), 1;
    if (!if_fir_fpow_process(ctx, x + 2 * (CUT1 + CUT2) * B, FRAMES - CUT1 - CUT2, codes + 3 * BO, power + 3 * BO, &f3) || f3 != 1)
        return printf("process 3: %s (%u frames)\n", if_fir_fpow_last_error(ctx), f3), 1;
    if (check(power, codes, want, &err))
        return 1;
    if (!if_fir_fpow_reset(ctx) || if_fir_fpow_frame_count(ctx, FRAMES) != OUT)
        return printf("reset: %s\n", if_fir_fpow_last_error(ctx)), 1;
    if (!if_fir_fpow_set_input_format(ctx, IF_FIR_INPUT_I16) || if_fir_fpow_set_input_format(ctx, 9))
        return printf("set_input_format\n"), 1;
    /* int16, and no powers asked for in the first of two calls */
    if (!if_fir_fpow_process(ctx, xi, K + 2, codes, NULL, &f1) || f1 != 1)
        return printf("process int16 1: %s\n", if_fir_fpow_last_error(ctx)), 1;
    if (!if_fir_fpow_reset(ctx) || !if_fir_fpow_process(ctx, xi, FRAMES, codes, power, &f2) || f2 != OUT)
        return printf("process int16 2: %s\n", if_fir_fpow_last_error(ctx)), 1;
    if (check(power, codes, wanti, &erri))
        return 1;
    if (!if_fir_fpow_synchronize(ctx))
        return printf("synchronize: %s\n", if_fir_fpow_last_error(ctx)), 1;
    if_fir_fpow_destroy(ctx);
    printf("power error %.3g (float32 input), %.3g (int16 input) of the value\nall checks passed\n", err, erri);
    return 0;
}
