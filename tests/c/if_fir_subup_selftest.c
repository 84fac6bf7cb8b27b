/* if_fir_subup_selftest.c — the per-bin interpolating FIR stage's C ABI from plain C99: include/if_fir.h and libif_fir.so only
 * (no HIP headers).  tests/test_subup_c_abi.py compiles it with gcc and runs it on the GPU.
 *
 * 1. A single 1 in bin 3 of frame 0, a tap row per bin, R = 2: bin 3 of output frame n is h_3[n] (0 once n >= T), every other
 *    bin 0: each bin meets its own row, and the taps come as given (no gain of R).
 * 2. A constant 1 in every bin through the 4-tap boxcar h = 1/4 at R = 2 with bin j mixed by f_j = j / 8 cycles per output
 *    frame: y_j[n] = v[n] e^{+j 2 pi j n / 8}, v[n] = 1/4 of the k <= min(n, 3) with n - k even; the same frames as int16
 *    (16384 = 0.5), in two calls, give half of it; get_nco returns the frequencies (+0.5 comes back as -0.5).
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
    static float taps[B * T], x[2 * B * F], y[2 * B * F * R], box[T], ones[2 * B * F], yt[2 * B * F * R];
    static short ones16[2 * B * F];
    static double freq[B], got[B];
    const double two_pi = 6.283185307179586476925286766559;
    if_fir_subup_t *ctx = NULL;
    if_fir_subup_config_t cfg;
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
    cfg.ulInterpolation = R;
    CHECK(!if_fir_subup_init(&ctx, &cfg, taps, F, 0) && ctx == NULL &&
              !strcmp(if_fir_subup_last_error(NULL), "if_fir_subup_init: bins must be 1..4096 (got 4097)"),
          "4097 bins: %s", if_fir_subup_last_error(NULL));
    cfg.ulBins = B;
    cfg.ulTapRows = 2;
    CHECK(!if_fir_subup_init(&ctx, &cfg, taps, F, 0) && ctx == NULL, "2 tap rows for 5 bins were accepted");
    cfg.ulTapRows = B;
    cfg.ulTaps = 2049;
    CHECK(!if_fir_subup_init(&ctx, &cfg, taps, F, 0) && ctx == NULL, "2049 taps were accepted");
    cfg.ulTaps = 66;
    CHECK(!if_fir_subup_init(&ctx, &cfg, taps, F, 0) && ctx == NULL && strstr(if_fir_subup_last_error(NULL), "J = ceil(66 / 2) = 33"),
          "33 taps per phase: %s", if_fir_subup_last_error(NULL));
    cfg.ulTaps = T;
    cfg.ulInterpolation = 65;
    CHECK(!if_fir_subup_init(&ctx, &cfg, taps, F, 0) && ctx == NULL, "interpolation 65 was accepted");
    cfg.ulInterpolation = R;

    /* 1. the single 1 */
    CHECK(if_fir_subup_init(&ctx, &cfg, taps, F, 0), "init: %s", if_fir_subup_last_error(NULL));
    CHECK(if_fir_subup_frame_count(ctx, F) == F * R && if_fir_subup_frame_count(ctx, 1) == R && if_fir_subup_frame_count(ctx, 0) == 0,
          "frame count %llu", (unsigned long long)if_fir_subup_frame_count(ctx, F));
    CHECK(if_fir_subup_process(ctx, x, y, F, &frames) && frames == F * R, "process: %s", if_fir_subup_last_error(ctx));
    for (n = 0; n < F * R; n++)
        for (j = 0; j < B; j++)
        {
            const float want = (j == 3 && n < T) ? taps[3 * T + n] : 0.0f;
            CHECK(y[2 * (n * B + j)] == want && y[2 * (n * B + j) + 1] == 0.0f, "single 1: frame %d bin %d is (%g, %g), want %g", n, j,
                  y[2 * (n * B + j)], y[2 * (n * B + j) + 1], want);
        }
    /* refused calls leave the stream: the next frame is frame F, whose history holds nothing of the 1 */
    CHECK(!if_fir_subup_process(ctx, x, y, F + 1, &frames) && strstr(if_fir_subup_last_error(ctx), "ullMaxFrames"),
          "a call above ullMaxFrames was accepted");
    CHECK(!if_fir_subup_set_input_format(ctx, 7), "format 7 was accepted");
    freq[0] = 0.6;
    CHECK(!if_fir_subup_set_nco(ctx, freq) && strstr(if_fir_subup_last_error(ctx), "+-0.5"), "0.6 cycles per frame were accepted");
    CHECK(if_fir_subup_process(ctx, x, y, 0, &frames) && frames == 0, "a call without a frame: %s", if_fir_subup_last_error(ctx));
    CHECK(if_fir_subup_process(ctx, x, y, 1, &frames) && frames == R, "the stream did not continue: %s", if_fir_subup_last_error(ctx));
    CHECK(y[2 * 3] == taps[3 * T] && y[2 * (B + 3)] == taps[3 * T + 1] && y[2 * 2] == 0.0f, "frame %d: bin 3 is %g, %g", F, y[2 * 3],
          y[2 * (B + 3)]);
    /* the frame after it carries the 1 of that call in its history: taps 2 and 3 */
    memset(yt, 0, sizeof yt);
    CHECK(if_fir_subup_process(ctx, x + 2 * B, y, 1, &frames) && frames == R && y[2 * 3] == taps[3 * T + 2] && y[2 * (B + 3)] == taps[3 * T + 3],
          "the history: bin 3 is %g, %g", y[2 * 3], y[2 * (B + 3)]);
    CHECK(if_fir_subup_reset(ctx) && if_fir_subup_process(ctx, x + 2 * B, y, 1, &frames) && y[2 * 3] == 0.0f && y[2 * (B + 3)] == 0.0f, "reset");
    if_fir_subup_destroy(ctx);
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
    CHECK(if_fir_subup_init(&ctx, &cfg, box, F, 0), "init: %s", if_fir_subup_last_error(NULL));
    CHECK(if_fir_subup_get_nco(ctx, got) && got[1] == 0.0 && got[4] == 0.0, "the words after init");
    CHECK(if_fir_subup_set_nco(ctx, freq) && if_fir_subup_get_nco(ctx, got), "set_nco: %s", if_fir_subup_last_error(ctx));
    for (j = 0; j < B; j++)
        CHECK(got[j] == (j == 4 ? -0.5 : freq[j]), "get_nco: bin %d has %g", j, got[j]);
    CHECK(if_fir_subup_process(ctx, ones, yt, F, &frames) && frames == F * R, "process: %s", if_fir_subup_last_error(ctx));
    for (i = 0; i < 2; i++)
    {
        const double level = i ? 0.5 : 1.0;
        for (n = 0; n < F * R; n++)
            for (j = 0; j < B; j++)
            {
                double v = 0.0, re, im;
                for (k = 0; k < T && k <= n; k++)
                    if ((n - k) % R == 0)
                        v += 0.25 * level;
                re = v * cos(two_pi * (double)((j * n) % 8) / 8.0);
                im = v * sin(two_pi * (double)((j * n) % 8) / 8.0);
                CHECK(fabs(yt[2 * (n * B + j)] - re) <= 1e-6 && fabs(yt[2 * (n * B + j) + 1] - im) <= 1e-6,
                      "%s: frame %d bin %d is (%g, %g), want (%g, %g)", i ? "int16" : "float32", n, j, yt[2 * (n * B + j)], yt[2 * (n * B + j) + 1], re,
                      im);
            }
        if (i)
            break;
        CHECK(if_fir_subup_reset(ctx) && if_fir_subup_set_input_format(ctx, IF_FIR_INPUT_I16), "int16: %s", if_fir_subup_last_error(ctx));
        CHECK(if_fir_subup_process(ctx, ones16, yt, 1, &frames) && frames == R, "int16, first call: %s", if_fir_subup_last_error(ctx));
        CHECK(if_fir_subup_process(ctx, ones16 + 2 * B, yt + 2 * B * R, F - 1, &frames) && frames == (F - 1) * R, "int16, second call: %s",
              if_fir_subup_last_error(ctx));
    }
    CHECK(if_fir_subup_set_nco(ctx, NULL) && if_fir_subup_get_nco(ctx, got) && got[3] == 0.0, "set_nco(NULL)");
    if_fir_subup_destroy(ctx);
    if_fir_subup_destroy(NULL);
    printf("all checks passed\n");
    return 0;
}
