/* if_fir_pfb_selftest.c — the polyphase filter bank's C ABI from plain C99: include/if_fir.h and libif_fir.so only (no HIP
 * headers).  tests/test_pfb_c_abi.py compiles it with gcc and runs it on the GPU.
 *
 * 1. An impulse at sample 0: y_k[m] = h[m D] e^{-j 2 pi k 0 / M} = h[m D] in every bin k (0 once m D >= T), in closed form.
 * 2. A tone on channel 5, x[a] = e^{+j 2 pi 5 a / M}, through the M-tap boxcar h = 1/M at D = M: from frame 1 on (a full window)
 *    bin 5 holds 1 and every other bin nothing; the same stream as int16, in two calls, lands there too.
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

enum { M = 64, T = 150, D = 16, N = 320 };

int main(void)
{
    static float taps[T], x[2 * N], y[2 * M * (N / D)], box[M], tone[2 * 4 * M], yt[2 * M * 4];
    static short tone16[2 * 4 * M];
    const double two_pi = 6.283185307179586476925286766559;
    if_fir_pfb_t *ctx = NULL;
    if_fir_pfb_config_t cfg;
    uint64_t frames = 0;
    int m, k, i;

    for (i = 0; i < T; i++)
        taps[i] = (float)(i + 1) / (float)T * ((i & 1) ? -1.0f : 1.0f);
    memset(x, 0, sizeof x);
    x[0] = 1.0f;

    /* refused configurations: a message for the NULL context, no context */
    cfg.ulChannels = 96;
    cfg.ulHop = D;
    cfg.lFirstBin = 0;
    cfg.ulBins = 96;
    CHECK(!if_fir_pfb_init(&ctx, &cfg, taps, T, N, 0) && ctx == NULL && strlen(if_fir_pfb_last_error(NULL)) > 0, "96 channels were accepted");
    cfg.ulChannels = M;
    cfg.ulBins = M;
    CHECK(!if_fir_pfb_init(&ctx, &cfg, taps, 16 * M + 1, N, 0) && ctx == NULL, "more than 16 M taps were accepted");
    cfg.ulHop = M + 1;
    CHECK(!if_fir_pfb_init(&ctx, &cfg, taps, T, N, 0) && ctx == NULL, "a hop above M was accepted");
    cfg.ulHop = D;

    /* 1. the impulse */
    CHECK(if_fir_pfb_init(&ctx, &cfg, taps, T, N, 0), "init: %s", if_fir_pfb_last_error(NULL));
    CHECK(if_fir_pfb_frame_count(ctx, N) == N / D, "frame count %llu", (unsigned long long)if_fir_pfb_frame_count(ctx, N));
    CHECK(if_fir_pfb_process(ctx, x, y, N, &frames) && frames == N / D, "process: %s", if_fir_pfb_last_error(ctx));
    for (m = 0; m < N / D; m++)
        for (k = 0; k < M; k++)
        {
            const float want = m * D < T ? taps[m * D] : 0.0f;
            const float re = y[2 * (m * M + k)], im = y[2 * (m * M + k) + 1];
            CHECK(fabsf(re - want) <= 1e-6f && fabsf(im) <= 1e-6f, "impulse: frame %d bin %d is (%g, %g), want (%g, 0)", m, k, re, im, want);
        }
    /* a refused call leaves the position: the next call is frame N / D's */
    CHECK(!if_fir_pfb_process(ctx, x, y, N + 1, &frames) && strstr(if_fir_pfb_last_error(ctx), "ullMaxSamples"), "a call above ullMaxSamples was accepted");
    CHECK(!if_fir_pfb_set_input_format(ctx, 7), "format 7 was accepted");
    CHECK(if_fir_pfb_frame_count(ctx, 1) == 1 && if_fir_pfb_process(ctx, x + 2, y, 1, &frames) && frames == 1, "the stream did not continue: %s",
          if_fir_pfb_last_error(ctx));
    CHECK(if_fir_pfb_frame_count(ctx, D - 1) == 0 && if_fir_pfb_process(ctx, x + 2, y, D - 1, &frames) && frames == 0, "a call without a frame");
    CHECK(if_fir_pfb_reset(ctx) && if_fir_pfb_frame_count(ctx, 1) == 1, "reset");
    if_fir_pfb_destroy(ctx);
    ctx = NULL;

    /* 2. the tone on channel 5 */
    for (i = 0; i < M; i++)
        box[i] = 1.0f / (float)M;
    for (i = 0; i < 4 * M; i++)
    {
        const double a = two_pi * (double)((5 * i) % M) / (double)M;
        tone[2 * i] = (float)cos(a);
        tone[2 * i + 1] = (float)sin(a);
        tone16[2 * i] = (short)lrint(16384.0 * cos(a));
        tone16[2 * i + 1] = (short)lrint(16384.0 * sin(a));
    }
    cfg.ulHop = M;
    CHECK(if_fir_pfb_init(&ctx, &cfg, box, M, 4 * M, 0), "init: %s", if_fir_pfb_last_error(NULL));
    CHECK(if_fir_pfb_process(ctx, tone, yt, 4 * M, &frames) && frames == 4, "process: %s", if_fir_pfb_last_error(ctx));
    for (m = 1; m < 4; m++)
        for (k = 0; k < M; k++)
        {
            const float re = yt[2 * (m * M + k)], im = yt[2 * (m * M + k) + 1], want = k == 5 ? 1.0f : 0.0f;
            CHECK(fabsf(re - want) <= 1e-5f && fabsf(im) <= 1e-5f, "tone: frame %d bin %d is (%g, %g)", m, k, re, im);
        }
    CHECK(if_fir_pfb_reset(ctx) && if_fir_pfb_set_input_format(ctx, IF_FIR_INPUT_I16), "int16: %s", if_fir_pfb_last_error(ctx));
    CHECK(if_fir_pfb_process(ctx, tone16, yt, M + 7, &frames) && frames == 2, "int16, first call: %s", if_fir_pfb_last_error(ctx));
    CHECK(if_fir_pfb_process(ctx, tone16 + 2 * (M + 7), yt + 2 * 2 * M, 3 * M - 7, &frames) && frames == 2, "int16, second call: %s",
          if_fir_pfb_last_error(ctx));
    for (m = 1; m < 4; m++)
        for (k = 0; k < M; k++)
        {
            const float re = yt[2 * (m * M + k)], im = yt[2 * (m * M + k) + 1], want = k == 5 ? 0.5f : 0.0f;
            CHECK(fabsf(re - want) <= 1e-4f && fabsf(im) <= 1e-4f, "int16 tone: frame %d bin %d is (%g, %g)", m, k, re, im);
        }
    if_fir_pfb_destroy(ctx);
    if_fir_pfb_destroy(NULL);
    printf("all checks passed\n");
    return 0;
}
