/* if_fir_sub_selftest.c — the per-channel FIR stage's C ABI from plain C99: include/if_fir.h and libif_fir.so only (no HIP
 * headers).  tests/test_sub_c_abi.py compiles it with gcc and runs it on the GPU.
 *
 * 1. A single 1 in bin 3 of frame 0, a tap row per bin, R = 2: bin 3 of output frame n is h_3[2 n] (0 once 2 n >= T), every
 *    other bin 0: each bin meets its own row.
 * 2. A constant 1 in every bin through the 4-tap boxcar h = 1/4 at R = 1 with bin j mixed by f_j = j / 8 cycles per frame:
 *    y_j[n] = 1/4 sum_{k <= min(n, 3)} e^{-j 2 pi j (n - k) / 8}, in closed form; the same frames as int16 (16384 = 0.5), in
 *    two calls, give half of it; get_nco returns the frequencies (+0.5 comes back as -0.5).
 * 3. Refused arguments leave a message and the context usable. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "if_fir.h"

#define CHECK(cond, ...)                  \
    do                                    \
    {                                     \
        if (!(cond))                      \
        {                                 \
            printf("FAILED: " __VA_ARGS__); \
            printf("\n");                 \
            return 1;                     \
        }                                 \
    } while (0)

enum { B = 5, T = 4, R = 2, F = 12 };

int main(void)
{
    static float taps[B * T], x[2 * B * F], y[2 * B * F], box[T], ones[2 * B * F], yt[2 * B * F];
    static short ones16[2 * B * F];
    static double freq[B], got[B];
    const double two_pi = 6.283185307179586476925286766559;
    if_fir_sub_t *ctx = NULL;
    if_fir_sub_config_t cfg;
    uint64_t frames = 0;
    int n, j, k, i;

    for (j = 0; j < B; j++)
        for (k = 0; k < T; k++)
            taps[j * T + k] = (float)(j + 1) + 0.125f * (float)k;
    memset(x, 0, sizeof x);
    x[2 * 3] = 1.0f;

    /* refused configurations: a message for the NULL context, no context */
    cfg.ulBins = 4097;
    cfg.ulTaps = T;
    cfg.ulTapRows = 1;
    cfg.ulDecimation = R;
    CHECK(!if_fir_sub_init(&ctx, &cfg, taps, F, 0) && ctx == NULL && !strcmp(if_fir_sub_last_error(NULL), "if_fir_sub_init: bins must be 1..4096 (got 4097)"),
          "4097 bins: %s", if_fir_sub_last_error(NULL));
    cfg.ulBins = B;
    cfg.ulTapRows = 2;
    CHECK(!if_fir_sub_init(&ctx, &cfg, taps, F, 0) && ctx == NULL, "2 tap rows for 5 bins were accepted");
    cfg.ulTapRows = B;
    cfg.ulTaps = 129;
    CHECK(!if_fir_sub_init(&ctx, &cfg, taps, F, 0) && ctx == NULL, "129 taps were accepted");
    cfg.ulTaps = T;
    cfg.ulDecimation = 65;
    CHECK(!if_fir_sub_init(&ctx, &cfg, taps, F, 0) && ctx == NULL, "decimation 65 was accepted");
    cfg.ulDecimation = R;

    /* 1. the single 1 */
    CHECK(if_fir_sub_init(&ctx, &cfg, taps, F, 0), "init: %s", if_fir_sub_last_error(NULL));
    CHECK(if_fir_sub_frame_count(ctx, F) == F / R && if_fir_sub_frame_count(ctx, 1) == 1, "frame count %llu",
          (unsigned long long)if_fir_sub_frame_count(ctx, F));
    CHECK(if_fir_sub_process(ctx, x, y, F, &frames) && frames == F / R, "process: %s", if_fir_sub_last_error(ctx));
    for (n = 0; n < F / R; n++)
        for (j = 0; j < B; j++)
        {
            const float want = (j == 3 && R * n < T) ? taps[3 * T + R * n] : 0.0f;
            CHECK(y[2 * (n * B + j)] == want && y[2 * (n * B + j) + 1] == 0.0f, "single 1: frame %d bin %d is (%g, %g), want %g", n, j,
                  y[2 * (n * B + j)], y[2 * (n * B + j) + 1], want);
        }
    /* a refused call leaves the position: the next frame is frame F (even), so one frame in gives one out */
    CHECK(!if_fir_sub_process(ctx, x, y, F + 1, &frames) && strstr(if_fir_sub_last_error(ctx), "ullMaxFrames"),
          "a call above ullMaxFrames was accepted");
    CHECK(!if_fir_sub_set_input_format(ctx, 7), "format 7 was accepted");
    freq[0] = 0.6;
    CHECK(!if_fir_sub_set_nco(ctx, freq) && strstr(if_fir_sub_last_error(ctx), "+-0.5"), "0.6 cycles per frame were accepted");
    CHECK(if_fir_sub_process(ctx, x, y, 0, &frames) && frames == 0, "a call without a frame: %s", if_fir_sub_last_error(ctx));
    CHECK(if_fir_sub_frame_count(ctx, 1) == 1 && if_fir_sub_process(ctx, x, y, 1, &frames) && frames == 1, "the stream did not continue: %s",
          if_fir_sub_last_error(ctx));
    CHECK(y[2 * 3] == taps[3 * T] && y[2 * 2] == 0.0f, "frame %d: bin 3 is %g", F, y[2 * 3]);
    CHECK(if_fir_sub_frame_count(ctx, 1) == 0 && if_fir_sub_reset(ctx) && if_fir_sub_frame_count(ctx, 1) == 1, "reset");
    if_fir_sub_destroy(ctx);
    ctx = NULL;

    /* 2. every bin mixed by its own frequency */
    for (k = 0; k < T; k++)
        box[k] = 0.25f;
    for (i = 0; i < B * F; i++)
    {
        ones[2 * i] = 1.0f;
        ones[2 * i + 1] = 0.0f;
        ones16[2 * i] = 16384;
        ones16[2 * i + 1] = 0;
    }
    for (j = 0; j < B; j++)
        freq[j] = (double)j / 8.0;
    cfg.ulTapRows = 1;
    cfg.ulDecimation = 1;
    CHECK(if_fir_sub_init(&ctx, &cfg, box, F, 0), "init: %s", if_fir_sub_last_error(NULL));
    CHECK(if_fir_sub_get_nco(ctx, got) && got[1] == 0.0 && got[4] == 0.0, "the words after init");
    CHECK(if_fir_sub_set_nco(ctx, freq) && if_fir_sub_get_nco(ctx, got), "set_nco: %s", if_fir_sub_last_error(ctx));
    for (j = 0; j < B; j++)
        CHECK(got[j] == (j == 4 ? -0.5 : freq[j]), "get_nco: bin %d has %g", j, got[j]);
    CHECK(if_fir_sub_process(ctx, ones, yt, F, &frames) && frames == F, "process: %s", if_fir_sub_last_error(ctx));
    for (i = 0; i < 2; i++)
    {
        const double level = i ? 0.5 : 1.0;
        for (n = 0; n < F; n++)
            for (j = 0; j < B; j++)
            {
                double re = 0.0, im = 0.0;
                for (k = 0; k < T && k <= n; k++)
                {
                    const double a = -two_pi * (double)((j * (n - k)) % 8) / 8.0;
                    re += 0.25 * level * cos(a);
                    im += 0.25 * level * sin(a);
                }
                CHECK(fabs(yt[2 * (n * B + j)] - re) <= 1e-6 && fabs(yt[2 * (n * B + j) + 1] - im) <= 1e-6,
                      "%s: frame %d bin %d is (%g, %g), want (%g, %g)", i ? "int16" : "float32", n, j, yt[2 * (n * B + j)], yt[2 * (n * B + j) + 1], re,
                      im);
            }
        if (i)
            break;
        CHECK(if_fir_sub_reset(ctx) && if_fir_sub_set_input_format(ctx, IF_FIR_INPUT_I16), "int16: %s", if_fir_sub_last_error(ctx));
        CHECK(if_fir_sub_process(ctx, ones16, yt, 1, &frames) && frames == 1, "int16, first call: %s", if_fir_sub_last_error(ctx));
        CHECK(if_fir_sub_process(ctx, ones16 + 2 * B, yt + 2 * B, F - 1, &frames) && frames == F - 1, "int16, second call: %s",
              if_fir_sub_last_error(ctx));
    }
    CHECK(if_fir_sub_set_nco(ctx, NULL) && if_fir_sub_get_nco(ctx, got) && got[3] == 0.0, "set_nco(NULL)");
    if_fir_sub_destroy(ctx);
    if_fir_sub_destroy(NULL);
    printf("all checks passed\n");
    return 0;
}
