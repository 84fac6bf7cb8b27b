/* The corner turn's C ABI from plain C99 (tests/test_turn_c_abi.py compiles and runs it): frames of 37 elements, five listed
 * bins in a scattered order, rows of pitch FRAMES + 3; TO_STREAMS through if_fir_turn_process in two calls with the pointers
 * advanced by hand, every format pair against the definition (docs/SPEC.md §20) element by element, the rows' tails untouched;
 * TO_FRAMES back gives the frames with the unlisted bins zeroed; the span form; refusals. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "if_fir.h"

#define B 37
#define C 5
#define FRAMES 71
#define PITCH (FRAMES + 3)
#define CUT 29

static const uint32_t sel[C] = {36, 0, 17, 5, 18};

/* SPEC §20's conversion of one component, written out */
static int16_t to_i16(float v)
{
    const float s = nearbyintf(v * 32768.0f);
    if (v != v)
        return 0;
    return (int16_t)(s > 32767.0f ? 32767.0f : s < -32768.0f ? -32768.0f : s);
}

int main(void)
{
    static float x[2 * FRAMES * B], rows[2 * C * PITCH], back[2 * FRAMES * B];
    static int16_t xi[2 * FRAMES * B], rowsi[2 * C * PITCH];
    if_fir_turn_config_t cfg = {IF_FIR_TURN_TO_STREAMS, B, C, 0, IF_FIR_INPUT_F32, IF_FIR_OUTPUT_F32};
    if_fir_turn_config_t bad;
    const uint32_t twice[C] = {36, 0, 17, 5, 17}, outside[C] = {36, 0, 37, 5, 18};
    if_fir_turn_t *down = NULL, *up = NULL, *span = NULL;
    long i, a, c, k;
    for (i = 0; i < 2 * FRAMES * B; i++)
    {
        x[i] = (float)(0.7 * cos(0.37 * i) + 0.5 * sin(0.0011 * i * i));   /* some beyond +-1: the int16 rule saturates them */
        xi[i] = (int16_t)lrint(30000.0 * cos(0.41 * i));
    }
    x[2 * (3 * B + 17)] = NAN;
    x[2 * (4 * B + 17) + 1] = INFINITY;
    x[2 * (5 * B + 17)] = -INFINITY;
    x[2 * (6 * B + 17)] = -0.0f;
    bad = cfg;
    bad.ulChannels = B + 1;
    if (if_fir_turn_init(&down, &bad, NULL, FRAMES, 0) || down || !*if_fir_turn_last_error(NULL))
        return printf("more channels than bins were not refused\n"), 1;
    if (if_fir_turn_init(&down, &cfg, twice, FRAMES, 0) || down || !strstr(if_fir_turn_last_error(NULL), "listed twice"))
        return printf("a repeated bin was not refused: %s\n", if_fir_turn_last_error(NULL)), 1;
    if (if_fir_turn_init(&down, &cfg, outside, FRAMES, 0) || down || !strstr(if_fir_turn_last_error(NULL), "outside the frame"))
        return printf("a bin past the frame was not refused: %s\n", if_fir_turn_last_error(NULL)), 1;
    bad = cfg;
    bad.ulFirst = 1;
    if (if_fir_turn_init(&down, &bad, sel, FRAMES, 0) || down || !strstr(if_fir_turn_last_error(NULL), "ulFirst must be 0"))
        return printf("ulFirst beside a list was not refused: %s\n", if_fir_turn_last_error(NULL)), 1;
    if (!if_fir_turn_init(&down, &cfg, sel, FRAMES, 0))
        return printf("init: %s\n", if_fir_turn_last_error(NULL)), 1;
    if (if_fir_turn_process(down, x, rows, FRAMES + 1, PITCH) || !strstr(if_fir_turn_last_error(down), "exceed ullMaxFrames"))
        return printf("a call above ullMaxFrames was not refused\n"), 1;
    if (if_fir_turn_process(down, x, rows, FRAMES, FRAMES - 1) || !strstr(if_fir_turn_last_error(down), "row pitch"))
        return printf("a pitch below the frames was not refused\n"), 1;
    if (if_fir_turn_process(down, NULL, rows, 4, PITCH) || !strstr(if_fir_turn_last_error(down), "NULL"))
        return printf("a NULL buffer was not refused\n"), 1;
    if (!if_fir_turn_process(down, NULL, NULL, 0, 0))
        return printf("an empty call: %s\n", if_fir_turn_last_error(down)), 1;
    /* float32 to float32 in two calls: the bits, and the tails as they were */
    for (i = 0; i < 2 * C * PITCH; i++)
        rows[i] = 77.0f;
    if (!if_fir_turn_process(down, x, rows, CUT, PITCH) ||
        !if_fir_turn_process(down, x + 2 * CUT * B, rows + 2 * CUT, FRAMES - CUT, PITCH))
        return printf("process: %s\n", if_fir_turn_last_error(down)), 1;
    for (c = 0; c < C; c++)
        for (a = 0; a < PITCH; a++)
        {
            const float *got = rows + 2 * (c * PITCH + a);
            if (a < FRAMES ? memcmp(got, x + 2 * (a * B + sel[c]), 8) != 0 : (got[0] != 77.0f || got[1] != 77.0f))
                return printf("float32 row %ld frame %ld\n", c, a), 1;
        }
    /* float32 to int16 */
    if (!if_fir_turn_set_output_format(down, IF_FIR_OUTPUT_I16) || if_fir_turn_set_output_format(down, 9))
        return printf("set_output_format\n"), 1;
    memset(rowsi, 0x11, sizeof rowsi);
    if (!if_fir_turn_process(down, x, rowsi, FRAMES, PITCH))
        return printf("process to int16: %s\n", if_fir_turn_last_error(down)), 1;
    for (c = 0; c < C; c++)
        for (a = 0; a < PITCH; a++)
            for (k = 0; k < 2; k++)
            {
                const int16_t got = rowsi[2 * (c * PITCH + a) + k];
                if (got != (a < FRAMES ? to_i16(x[2 * (a * B + sel[c]) + k]) : 0x1111))
                    return printf("int16 row %ld frame %ld part %ld: %d\n", c, a, k, got), 1;
            }
    if (rowsi[2 * (2 * PITCH + 3)] != 0 || rowsi[2 * (2 * PITCH + 4) + 1] != 32767 || rowsi[2 * (2 * PITCH + 5)] != -32768)
        return printf("NaN, +inf, -inf: %d %d %d\n", rowsi[2 * (2 * PITCH + 3)], rowsi[2 * (2 * PITCH + 4) + 1], rowsi[2 * (2 * PITCH + 5)]), 1;
    /* int16 to float32: exact, and int16 to int16: a copy */
    if (!if_fir_turn_set_input_format(down, IF_FIR_INPUT_I16) || if_fir_turn_set_input_format(down, 9) ||
        !if_fir_turn_set_output_format(down, IF_FIR_OUTPUT_F32) || !if_fir_turn_process(down, xi, rows, FRAMES, PITCH))
        return printf("process from int16: %s\n", if_fir_turn_last_error(down)), 1;
    for (c = 0; c < C; c++)
        for (a = 0; a < FRAMES; a++)
            for (k = 0; k < 2; k++)
                if (rows[2 * (c * PITCH + a) + k] != (float)xi[2 * (a * B + sel[c]) + k] / 32768.0f)
                    return printf("int16 to float32 row %ld frame %ld\n", c, a), 1;
    if (!if_fir_turn_set_output_format(down, IF_FIR_OUTPUT_I16) || !if_fir_turn_process(down, xi, rowsi, FRAMES, PITCH))
        return printf("process int16 to int16: %s\n", if_fir_turn_last_error(down)), 1;
    for (c = 0; c < C; c++)
        for (a = 0; a < FRAMES; a++)
            if (memcmp(rowsi + 2 * (c * PITCH + a), xi + 2 * (a * B + sel[c]), 4))
                return printf("int16 copy row %ld frame %ld\n", c, a), 1;
    /* back: float32 rows to frames; the unlisted bins are +0 */
    if (!if_fir_turn_set_input_format(down, IF_FIR_INPUT_F32) || !if_fir_turn_set_output_format(down, IF_FIR_OUTPUT_F32) ||
        !if_fir_turn_process(down, x, rows, FRAMES, PITCH))
        return printf("process again: %s\n", if_fir_turn_last_error(down)), 1;
    cfg.ulDirection = IF_FIR_TURN_TO_FRAMES;
    if (!if_fir_turn_init(&up, &cfg, sel, FRAMES, 0))
        return printf("init to frames: %s\n", if_fir_turn_last_error(NULL)), 1;
    memset(back, 0x11, sizeof back);
    if (!if_fir_turn_process(up, rows, back, FRAMES, PITCH))
        return printf("process to frames: %s\n", if_fir_turn_last_error(up)), 1;
    for (a = 0; a < FRAMES; a++)
        for (i = 0; i < B; i++)
        {
            static const float zero[2] = {0.0f, 0.0f};
            int listed = 0;
            for (c = 0; c < C; c++)
                listed |= sel[c] == (uint32_t)i;
            if (memcmp(back + 2 * (a * B + i), listed ? x + 2 * (a * B + i) : zero, 8))
                return printf("round trip frame %ld bin %ld\n", a, i), 1;
        }
    /* the span form: bins 30 .. 34 */
    cfg.ulDirection = IF_FIR_TURN_TO_STREAMS;
    cfg.ulFirst = 30;
    if (!if_fir_turn_init(&span, &cfg, NULL, FRAMES, 0) || !if_fir_turn_process(span, x, rows, FRAMES, PITCH))
        return printf("span: %s\n", if_fir_turn_last_error(span)), 1;
    for (c = 0; c < C; c++)
        for (a = 0; a < FRAMES; a++)
            if (memcmp(rows + 2 * (c * PITCH + a), x + 2 * (a * B + 30 + c), 8))
                return printf("span row %ld frame %ld\n", c, a), 1;
    if (!if_fir_turn_synchronize(down) || !if_fir_turn_set_stream(down, NULL))
        return printf("synchronize: %s\n", if_fir_turn_last_error(down)), 1;
    if_fir_turn_destroy(down);
    if_fir_turn_destroy(up);
    if_fir_turn_destroy(span);
    if_fir_turn_destroy(NULL);
    printf("all checks passed\n");
    return 0;
}
