/* if_fir_rpfb_selftest.c — the real-input polyphase filter bank's C ABI from plain C99: include/if_fir.h and libif_fir.so only
 * (no HIP headers).  tests/test_rpfb_c_abi.py compiles it with gcc and runs it on the GPU.
 *
 * 1. An impulse at sample 0: y_k[m] = h[m D] e^{-j 2 pi k 0 / M} = h[m D] in every bin k = 0 .. M/2 (0 once m D >= T), in closed
 *    form; the bins 0 and M/2 have an imaginary part of exactly zero.
 * 2. A real tone on channel 5, r[a] = cos(2 pi 5 a / M), through the M-tap boxcar h = 1/M at D = M: from frame 1 on (a full
 *    window) bin 5 holds 1/2 and every other bin nothing; with 1 + (-1)^a added, bin 0 holds 1 and bin M/2 holds 1 as well.  The
 *    same stream as int16, in two calls, lands there too.  A span of three bins from 4 holds the bins 4, 5, 6.
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

enum { M = 128, H = M / 2, BINS = H + 1, T = 300, D = 32, N = 640 };

int main(void)
{
    static float taps[T], x[N], y[2 * BINS * (N / D)], box[M], tone[4 * M], yt[2 * BINS * 4], ys[2 * 3 * 4];
    static short tone16[4 * M];
    const double two_pi = 6.283185307179586476925286766559;
    if_fir_rpfb_t *ctx = NULL;
    if_fir_rpfb_config_t cfg;
    uint64_t frames = 0;
    int m, k, i;

    for (i = 0; i < T; i++)
        taps[i] = (float)(i + 1) / (float)T * ((i & 1) ? -1.0f : 1.0f);
    memset(x, 0, sizeof x);
    x[0] = 1.0f;

    /* refused configurations: a message for the NULL context, no context */
    cfg.ulChannels = 64;
    cfg.ulHop = D;
    cfg.ulFirstBin = 0;
    cfg.ulBins = 33;
    CHECK(!if_fir_rpfb_init(&ctx, &cfg, taps, T, N, 0) && ctx == NULL && strstr(if_fir_rpfb_last_error(NULL), "got 64"), "64 channels were accepted");
    cfg.ulChannels = M;
    cfg.ulBins = BINS + 1;
    CHECK(!if_fir_rpfb_init(&ctx, &cfg, taps, T, N, 0) && ctx == NULL && strstr(if_fir_rpfb_last_error(NULL), "span"), "M/2 + 2 bins were accepted");
    cfg.ulBins = BINS;
    CHECK(!if_fir_rpfb_init(&ctx, &cfg, taps, 16 * M + 1, N, 0) && ctx == NULL, "more than 16 M taps were accepted");
    cfg.ulHop = M + 1;
    CHECK(!if_fir_rpfb_init(&ctx, &cfg, taps, T, N, 0) && ctx == NULL, "a hop above M was accepted");
    cfg.ulHop = D;

    /* 1. the impulse */
    CHECK(if_fir_rpfb_init(&ctx, &cfg, taps, T, N, 0), "init: %s", if_fir_rpfb_last_error(NULL));
    CHECK(if_fir_rpfb_frame_count(ctx, N) == N / D, "frame count %llu", (unsigned long long)if_fir_rpfb_frame_count(ctx, N));
    CHECK(if_fir_rpfb_process(ctx, x, y, N, &frames) && frames == N / D, "process: %s", if_fir_rpfb_last_error(ctx));
    for (m = 0; m < N / D; m++)
        for (k = 0; k < BINS; k++)
        {
            const float want = m * D < T ? taps[m * D] : 0.0f;
            const float re = y[2 * (m * BINS + k)], im = y[2 * (m * BINS + k) + 1];
            CHECK(fabsf(re - want) <= 1e-6f && fabsf(im) <= 1e-6f, "impulse: frame %d bin %d is (%g, %g), want (%g, 0)", m, k, re, im, want);
            CHECK((k != 0 && k != H) || im == 0.0f, "impulse: frame %d bin %d has the imaginary part %g", m, k, im);
        }
    /* a refused call leaves the position: the next call is frame N / D's */
    CHECK(!if_fir_rpfb_process(ctx, x, y, N + 1, &frames) && strstr(if_fir_rpfb_last_error(ctx), "ullMaxSamples"), "a call above ullMaxSamples was accepted");
    CHECK(!if_fir_rpfb_set_input_format(ctx, 7), "format 7 was accepted");
    CHECK(if_fir_rpfb_frame_count(ctx, 1) == 1 && if_fir_rpfb_process(ctx, x + 1, y, 1, &frames) && frames == 1, "the stream did not continue: %s",
          if_fir_rpfb_last_error(ctx));
    CHECK(if_fir_rpfb_frame_count(ctx, D - 1) == 0 && if_fir_rpfb_process(ctx, x + 1, y, D - 1, &frames) && frames == 0, "a call without a frame");
    CHECK(if_fir_rpfb_reset(ctx) && if_fir_rpfb_frame_count(ctx, 1) == 1, "reset");
    if_fir_rpfb_destroy(ctx);
    ctx = NULL;

    /* 2. the tone on channel 5, DC and the highest channel */
    for (i = 0; i < M; i++)
        box[i] = 1.0f / (float)M;
    for (i = 0; i < 4 * M; i++)
    {
        const double v = cos(two_pi * (double)((5 * i) % M) / (double)M) + 1.0 + ((i & 1) ? -1.0 : 1.0);
        tone[i] = (float)v;
        tone16[i] = (short)lrint(8192.0 * v);
    }
    cfg.ulHop = M;
    CHECK(if_fir_rpfb_init(&ctx, &cfg, box, M, 4 * M, 0), "init: %s", if_fir_rpfb_last_error(NULL));
    CHECK(if_fir_rpfb_process(ctx, tone, yt, 4 * M, &frames) && frames == 4, "process: %s", if_fir_rpfb_last_error(ctx));
    for (m = 1; m < 4; m++)
        for (k = 0; k < BINS; k++)
        {
            const float re = yt[2 * (m * BINS + k)], im = yt[2 * (m * BINS + k) + 1], want = k == 5 ? 0.5f : (k == 0 || k == H) ? 1.0f : 0.0f;
            CHECK(fabsf(re - want) <= 1e-5f && fabsf(im) <= 1e-5f, "tone: frame %d bin %d is (%g, %g)", m, k, re, im);
        }
    CHECK(if_fir_rpfb_reset(ctx) && if_fir_rpfb_set_input_format(ctx, IF_FIR_INPUT_I16), "int16: %s", if_fir_rpfb_last_error(ctx));
    CHECK(if_fir_rpfb_process(ctx, tone16, yt, M + 7, &frames) && frames == 2, "int16, first call: %s", if_fir_rpfb_last_error(ctx));
    CHECK(if_fir_rpfb_process(ctx, tone16 + (M + 7), yt + 2 * 2 * BINS, 3 * M - 7, &frames) && frames == 2, "int16, second call: %s",
          if_fir_rpfb_last_error(ctx));
    for (m = 1; m < 4; m++)
        for (k = 0; k < BINS; k++)
        {
            const float re = yt[2 * (m * BINS + k)], im = yt[2 * (m * BINS + k) + 1], want = k == 5 ? 0.125f : (k == 0 || k == H) ? 0.25f : 0.0f;
            CHECK(fabsf(re - want) <= 1e-4f && fabsf(im) <= 1e-4f, "int16 tone: frame %d bin %d is (%g, %g)", m, k, re, im);
        }
    if_fir_rpfb_destroy(ctx);
    ctx = NULL;
    cfg.ulFirstBin = 4;
    cfg.ulBins = 3;
    CHECK(if_fir_rpfb_init(&ctx, &cfg, box, M, 4 * M, 0), "init of a span: %s", if_fir_rpfb_last_error(NULL));
    CHECK(if_fir_rpfb_process(ctx, tone, ys, 4 * M, &frames) && frames == 4, "process of a span: %s", if_fir_rpfb_last_error(ctx));
    for (m = 1; m < 4; m++)
        for (k = 0; k < 3; k++)
            CHECK(fabsf(ys[2 * (m * 3 + k)] - (k == 1 ? 0.5f : 0.0f)) <= 1e-5f && fabsf(ys[2 * (m * 3 + k) + 1]) <= 1e-5f, "span: frame %d bin %d is (%g, %g)",
                  m, 4 + k, ys[2 * (m * 3 + k)], ys[2 * (m * 3 + k) + 1]);
    if_fir_rpfb_destroy(ctx);
    if_fir_rpfb_destroy(NULL);
    printf("all checks passed\n");
    return 0;
}
