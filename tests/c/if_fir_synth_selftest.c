/* if_fir_synth_selftest.c — the polyphase synthesis bank's C ABI from plain C99: include/if_fir.h and libif_fir.so only (no HIP
 * headers).  tests/test_synth_c_abi.py compiles it with gcc and runs it on the GPU.
 *
 * 1. A single 1 on channel 5 of frame 0: y[n] = h[n] e^{+j 2 pi 5 n / M} (0 once n >= T), in closed form.
 * 2. A constant 1 on channel 5 of every frame through the M-tap boxcar h = 1 at L = M: the tone e^{+j 2 pi 5 n / M}; the same
 *    frames as int16 (16384 = 0.5), in two calls, give half of it.
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

enum { M = 64, T = 150, L = 16, F = 12 };

int main(void)
{
    static float taps[T], x[2 * M * F], y[2 * L * F], box[M], ones[2 * M * 4], yt[2 * M * 4];
    static short ones16[2 * M * 4];
    const double two_pi = 6.283185307179586476925286766559;
    if_fir_synth_t *ctx = NULL;
    if_fir_synth_config_t cfg;
    uint64_t samples = 0;
    int n, i;

    for (i = 0; i < T; i++)
        taps[i] = (float)(i + 1) / (float)T * ((i & 1) ? -1.0f : 1.0f);
    memset(x, 0, sizeof x);
    x[2 * 5] = 1.0f;

    /* refused configurations: a message for the NULL context, no context */
    cfg.ulChannels = 96;
    cfg.ulHop = L;
    cfg.lFirstBin = 0;
    cfg.ulBins = 96;
    CHECK(!if_fir_synth_init(&ctx, &cfg, taps, T, F, 0) && ctx == NULL && strlen(if_fir_synth_last_error(NULL)) > 0, "96 channels were accepted");
    cfg.ulChannels = M;
    cfg.ulBins = M;
    CHECK(!if_fir_synth_init(&ctx, &cfg, taps, 16 * M + 1, F, 0) && ctx == NULL, "more than 16 M taps were accepted");
    cfg.ulHop = M + 1;
    CHECK(!if_fir_synth_init(&ctx, &cfg, taps, T, F, 0) && ctx == NULL, "a hop above M was accepted");
    cfg.ulHop = 4;
    CHECK(!if_fir_synth_init(&ctx, &cfg, taps, T, F, 0) && ctx == NULL, "150 taps at hop 4 (38 terms) were accepted");
    cfg.ulHop = L;

    /* 1. the single 1 */
    CHECK(if_fir_synth_init(&ctx, &cfg, taps, T, F, 0), "init: %s", if_fir_synth_last_error(NULL));
    CHECK(if_fir_synth_sample_count(ctx, F) == F * L, "sample count %llu", (unsigned long long)if_fir_synth_sample_count(ctx, F));
    CHECK(if_fir_synth_process(ctx, x, y, F, &samples) && samples == F * L, "process: %s", if_fir_synth_last_error(ctx));
    for (n = 0; n < F * L; n++)
    {
        const double a = two_pi * (double)((5 * n) % M) / (double)M, h = n < T ? taps[n] : 0.0;
        CHECK(fabs(y[2 * n] - h * cos(a)) <= 2e-6 && fabs(y[2 * n + 1] - h * sin(a)) <= 2e-6, "single 1: output %d is (%g, %g), want (%g, %g)", n,
              y[2 * n], y[2 * n + 1], h * cos(a), h * sin(a));
    }
    /* a refused call leaves the position */
    CHECK(!if_fir_synth_process(ctx, x, y, F + 1, &samples) && strstr(if_fir_synth_last_error(ctx), "ullMaxFrames"),
          "a call above ullMaxFrames was accepted");
    CHECK(!if_fir_synth_set_input_format(ctx, 7), "format 7 was accepted");
    CHECK(if_fir_synth_process(ctx, x, y, 0, &samples) && samples == 0, "a call without a frame: %s", if_fir_synth_last_error(ctx));
    /* frame F of the stream (all zeros but for the 1): the tail of frame 0 has passed (F L >= T), so only this frame's taps show */
    CHECK(if_fir_synth_process(ctx, x, y, 1, &samples) && samples == L, "the stream did not continue: %s", if_fir_synth_last_error(ctx));
    for (n = 0; n < L; n++)
    {
        const double a = two_pi * (double)((5 * (F * L + n)) % M) / (double)M;
        CHECK(fabs(y[2 * n] - taps[n] * cos(a)) <= 2e-6 && fabs(y[2 * n + 1] - taps[n] * sin(a)) <= 2e-6, "frame %d: output %d is (%g, %g)", F, n,
              y[2 * n], y[2 * n + 1]);
    }
    CHECK(if_fir_synth_reset(ctx) && if_fir_synth_sample_count(ctx, 3) == 3 * L, "reset");
    if_fir_synth_destroy(ctx);
    ctx = NULL;

    /* 2. the tone from channel 5 */
    memset(ones, 0, sizeof ones);
    memset(ones16, 0, sizeof ones16);
    for (i = 0; i < M; i++)
        box[i] = 1.0f;
    for (i = 0; i < 4; i++)
    {
        ones[2 * (i * M + 5)] = 1.0f;
        ones16[2 * (i * M + 5)] = 16384;
    }
    cfg.ulHop = M;
    CHECK(if_fir_synth_init(&ctx, &cfg, box, M, 4, 0), "init: %s", if_fir_synth_last_error(NULL));
    CHECK(if_fir_synth_process(ctx, ones, yt, 4, &samples) && samples == 4 * M, "process: %s", if_fir_synth_last_error(ctx));
    for (n = 0; n < 4 * M; n++)
    {
        const double a = two_pi * (double)((5 * n) % M) / (double)M;
        CHECK(fabs(yt[2 * n] - cos(a)) <= 1e-5 && fabs(yt[2 * n + 1] - sin(a)) <= 1e-5, "tone: output %d is (%g, %g)", n, yt[2 * n], yt[2 * n + 1]);
    }
    CHECK(if_fir_synth_reset(ctx) && if_fir_synth_set_input_format(ctx, IF_FIR_INPUT_I16), "int16: %s", if_fir_synth_last_error(ctx));
    CHECK(if_fir_synth_process(ctx, ones16, yt, 1, &samples) && samples == M, "int16, first call: %s", if_fir_synth_last_error(ctx));
    CHECK(if_fir_synth_process(ctx, ones16 + 2 * M, yt + 2 * M, 3, &samples) && samples == 3 * M, "int16, second call: %s",
          if_fir_synth_last_error(ctx));
    for (n = 0; n < 4 * M; n++)
    {
        const double a = two_pi * (double)((5 * n) % M) / (double)M;
        CHECK(fabs(yt[2 * n] - 0.5 * cos(a)) <= 1e-5 && fabs(yt[2 * n + 1] - 0.5 * sin(a)) <= 1e-5, "int16 tone: output %d is (%g, %g)", n, yt[2 * n],
              yt[2 * n + 1]);
    }
    if_fir_synth_destroy(ctx);
    if_fir_synth_destroy(NULL);
    printf("all checks passed\n");
    return 0;
}
