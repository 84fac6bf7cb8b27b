/* if_fir_rsynth_selftest.c — the real-output polyphase synthesis bank's C ABI from plain C99: include/if_fir.h and libif_fir.so
 * only (no HIP headers).  tests/test_rsynth_c_abi.py compiles it with gcc and runs it on the GPU.
 *
 * 1. A single 1 + 0.25j on channel 5 of frame 0: y[n] = 2 h[n] (cos(2 pi 5 n / M) - 0.25 sin(2 pi 5 n / M)) (0 once n >= T), in
 *    closed form; the same on channel 0, whose imaginary part is ignored: y[n] = h[n].
 * 2. A constant 1 on channel 5 of every frame through the M-tap boxcar h = 1 at L = M: the tone 2 cos(2 pi 5 n / M); the same
 *    frames as int16 (16384 = 0.5), in two calls, give half of it, and as int16 output that half times 2^15, saturated at 32767.
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

enum { M = 128, H = M / 2, BINS = H + 1, T = 150, L = 16, F = 12 };

int main(void)
{
    static float taps[T], x[2 * BINS * F], y[L * F], box[M], ones[2 * BINS * 4], yt[M * 4];
    static short ones16[2 * BINS * 4], yq[M * 4];
    const double two_pi = 6.283185307179586476925286766559;
    if_fir_rsynth_t *ctx = NULL;
    if_fir_rsynth_config_t cfg;
    uint64_t samples = 0;
    int n, i;

    for (i = 0; i < T; i++)
        taps[i] = (float)(i + 1) / (float)T * ((i & 1) ? -1.0f : 1.0f);
    memset(x, 0, sizeof x);
    x[2 * 5] = 1.0f;
    x[2 * 5 + 1] = 0.25f;

    /* refused configurations: a message for the NULL context, no context */
    cfg.ulChannels = 64;
    cfg.ulHop = L;
    cfg.ulFirstBin = 0;
    cfg.ulBins = 33;
    CHECK(!if_fir_rsynth_init(&ctx, &cfg, taps, T, F, 0) && ctx == NULL && strlen(if_fir_rsynth_last_error(NULL)) > 0, "64 channels were accepted");
    cfg.ulChannels = 16384;
    CHECK(!if_fir_rsynth_init(&ctx, &cfg, taps, T, F, 0) && ctx == NULL, "16384 channels were accepted");
    cfg.ulChannels = M;
    cfg.ulBins = BINS + 1;
    CHECK(!if_fir_rsynth_init(&ctx, &cfg, taps, T, F, 0) && ctx == NULL, "a span past channel M/2 was accepted");
    cfg.ulBins = BINS;
    CHECK(!if_fir_rsynth_init(&ctx, &cfg, taps, 16 * M + 1, F, 0) && ctx == NULL, "more than 16 M taps were accepted");
    cfg.ulHop = M + 1;
    CHECK(!if_fir_rsynth_init(&ctx, &cfg, taps, T, F, 0) && ctx == NULL, "a hop above M was accepted");
    cfg.ulHop = 4;
    CHECK(!if_fir_rsynth_init(&ctx, &cfg, taps, T, F, 0) && ctx == NULL, "150 taps at hop 4 (38 terms) were accepted");
    cfg.ulHop = L;

    /* 1. the single 1 + 0.25j */
    CHECK(if_fir_rsynth_init(&ctx, &cfg, taps, T, F, 0), "init: %s", if_fir_rsynth_last_error(NULL));
    CHECK(if_fir_rsynth_sample_count(ctx, F) == F * L, "sample count %llu", (unsigned long long)if_fir_rsynth_sample_count(ctx, F));
    CHECK(if_fir_rsynth_process(ctx, x, y, F, &samples) && samples == F * L, "process: %s", if_fir_rsynth_last_error(ctx));
    for (n = 0; n < F * L; n++)
    {
        const double a = two_pi * (double)((5 * n) % M) / (double)M, h = n < T ? taps[n] : 0.0, want = 2.0 * h * (cos(a) - 0.25 * sin(a));
        CHECK(fabs(y[n] - want) <= 4e-6, "single 1: output %d is %g, want %g", n, y[n], want);
    }
    /* a refused call leaves the position */
    CHECK(!if_fir_rsynth_process(ctx, x, y, F + 1, &samples) && strstr(if_fir_rsynth_last_error(ctx), "ullMaxFrames"),
          "a call above ullMaxFrames was accepted");
    CHECK(!if_fir_rsynth_set_input_format(ctx, 7), "input format 7 was accepted");
    CHECK(!if_fir_rsynth_set_output_format(ctx, 7), "output format 7 was accepted");
    CHECK(if_fir_rsynth_process(ctx, x, y, 0, &samples) && samples == 0, "a call without a frame: %s", if_fir_rsynth_last_error(ctx));
    /* frame F of the stream (all zeros but for the 1): the tail of frame 0 has passed (F L >= T), so only this frame's taps show */
    CHECK(if_fir_rsynth_process(ctx, x, y, 1, &samples) && samples == L, "the stream did not continue: %s", if_fir_rsynth_last_error(ctx));
    for (n = 0; n < L; n++)
    {
        const double a = two_pi * (double)((5 * (F * L + n)) % M) / (double)M, want = 2.0 * taps[n] * (cos(a) - 0.25 * sin(a));
        CHECK(fabs(y[n] - want) <= 4e-6, "frame %d: output %d is %g, want %g", F, n, y[n], want);
    }
    /* the same value on channel 0: its imaginary part is ignored */
    CHECK(if_fir_rsynth_reset(ctx) && if_fir_rsynth_sample_count(ctx, 3) == 3 * L, "reset");
    x[2 * 5] = x[2 * 5 + 1] = 0.0f;
    x[0] = 1.0f;
    x[1] = 0.25f;
    CHECK(if_fir_rsynth_process(ctx, x, y, F, &samples) && samples == F * L, "process: %s", if_fir_rsynth_last_error(ctx));
    for (n = 0; n < F * L; n++)
        CHECK(y[n] == (n < T ? taps[n] : 0.0f), "channel 0: output %d is %g", n, y[n]);
    if_fir_rsynth_destroy(ctx);
    ctx = NULL;

    /* 2. the tone from channel 5 */
    memset(ones, 0, sizeof ones);
    memset(ones16, 0, sizeof ones16);
    for (i = 0; i < M; i++)
        box[i] = 1.0f;
    for (i = 0; i < 4; i++)
    {
        ones[2 * (i * BINS + 5)] = 1.0f;
        ones16[2 * (i * BINS + 5)] = 16384;
    }
    cfg.ulHop = M;
    CHECK(if_fir_rsynth_init(&ctx, &cfg, box, M, 4, 0), "init: %s", if_fir_rsynth_last_error(NULL));
    CHECK(if_fir_rsynth_process(ctx, ones, yt, 4, &samples) && samples == 4 * M, "process: %s", if_fir_rsynth_last_error(ctx));
    for (n = 0; n < 4 * M; n++)
    {
        const double a = two_pi * (double)((5 * n) % M) / (double)M;
        CHECK(fabs(yt[n] - 2.0 * cos(a)) <= 1e-5, "tone: output %d is %g", n, yt[n]);
    }
    CHECK(if_fir_rsynth_reset(ctx) && if_fir_rsynth_set_input_format(ctx, IF_FIR_INPUT_I16), "int16: %s", if_fir_rsynth_last_error(ctx));
    CHECK(if_fir_rsynth_process(ctx, ones16, yt, 1, &samples) && samples == M, "int16, first call: %s", if_fir_rsynth_last_error(ctx));
    CHECK(if_fir_rsynth_process(ctx, ones16 + 2 * BINS, yt + M, 3, &samples) && samples == 3 * M, "int16, second call: %s",
          if_fir_rsynth_last_error(ctx));
    for (n = 0; n < 4 * M; n++)
    {
        const double a = two_pi * (double)((5 * n) % M) / (double)M;
        CHECK(fabs(yt[n] - cos(a)) <= 1e-5, "int16 tone: output %d is %g", n, yt[n]);
    }
    /* int16 out: the float32 result of the same frames times 2^15, to nearest even, saturated (cos = 1 gives 32767) */
    CHECK(if_fir_rsynth_reset(ctx) && if_fir_rsynth_set_output_format(ctx, IF_FIR_OUTPUT_I16), "int16 out: %s", if_fir_rsynth_last_error(ctx));
    CHECK(if_fir_rsynth_process(ctx, ones16, yq, 4, &samples) && samples == 4 * M, "int16 out: %s", if_fir_rsynth_last_error(ctx));
    for (n = 0; n < 4 * M; n++)
    {
        double want = nearbyint((double)yt[n] * 32768.0);
        want = want > 32767.0 ? 32767.0 : want < -32768.0 ? -32768.0 : want;
        CHECK((double)yq[n] == want, "int16 out: output %d is %d, want %g", n, yq[n], want);
    }
    CHECK(yq[0] == 32767 && yq[M] == 32767, "int16 out: the peak is %d, not saturated", yq[0]);
    if_fir_rsynth_destroy(ctx);
    if_fir_rsynth_destroy(NULL);
    printf("all checks passed\n");
    return 0;
}
