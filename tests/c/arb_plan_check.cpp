// arb_plan_check.cpp — walks qo-100-tools_amd/csrc/if_fir_arb_plan.h, the planning the arbitrary-ratio resampler's shim and kernel
// use, with a plain host compiler (tests/test_arb_host.py; that test also builds it with -fsanitize=address,undefined and runs
// the self-check).
//
// Without arguments, the self-check: for every b in 4..10 and T in {1, P-1, P, P+1, 255, 8192} the table of arb_build_taps,
// built into a heap buffer of exactly 2 P KP floats, holds (h[p + j P], h[p + 1 + j P]) with zeros where the index reaches T;
// for steps at the ends of the range and seeded ones, time offsets at the ends of theirs, and tiles up to the last one of the
// largest call: arb_time equals tau_rel + i R in 128-bit arithmetic, every place of the tile (arb_place) has p < P, mu in
// [0, 1] (28 low bits of ones round up to 1), and its K samples inside the window of arb_window; a random walk of calls and retunes keeps arb_state_ok.
//
// With `query`, answers one request per line of standard input (all numbers decimal; tau up to 96 bits):
//   count c tau n R      -> the outputs of the call, or -1 when refused, and arb_state_ok(c, tau)
//   time tau_rel i R     -> q f of arb_time
//   place f0 l R b       -> dq p mu (mu as a hexadecimal float)
//   shape T b R          -> K KP P tile_out x_len tap_entries lds_bytes
//   table b T            -> the table of the taps h[k] = k + 1: P rows of KP pairs "first:second"
//   step rate_in rate_out -> arb_step_from_rates
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "if_fir_arb_plan.h"

using namespace if_fir;

static arb_u128 parse_u128(const char *s)
{
    arb_u128 v = 0;
    for (; *s >= '0' && *s <= '9'; s++)
        v = v * 10 + (arb_u128)(*s - '0');
    return v;
}

static int fail(const char *what, int b, int T, unsigned long long R, unsigned long long a, unsigned long long c)
{
    printf("FAILED: %s at b=%d T=%d R=%llu (%llu, %llu)\n", what, b, T, R, a, c);
    return 1;
}

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint64_t rnd()
{
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}

static int query()
{
    char line[512], a[5][128];
    while (fgets(line, sizeof line, stdin))
    {
        const int n = sscanf(line, "%127s %127s %127s %127s %127s", a[0], a[1], a[2], a[3], a[4]);
        if (n < 1)
            continue;
        if (!strcmp(a[0], "count") && n == 5)
        {
            const uint64_t c = strtoull(a[1], nullptr, 10), cnt = strtoull(a[3], nullptr, 10), R = strtoull(a[4], nullptr, 10);
            const arb_u128 tau = parse_u128(a[2]);
            uint64_t count = 0;
            if (arb_out_count(c, tau, cnt, R, &count))
                printf("%" PRIu64 " %d\n", count, (int)arb_state_ok(c, tau));
            else
                printf("-1 %d\n", (int)arb_state_ok(c, tau));
        }
        else if (!strcmp(a[0], "time") && n == 4)
        {
            int64_t q;
            uint32_t f;
            arb_time(strtoull(a[1], nullptr, 10), strtoull(a[2], nullptr, 10), strtoull(a[3], nullptr, 10), &q, &f);
            printf("%" PRId64 " %" PRIu32 "\n", q, f);
        }
        else if (!strcmp(a[0], "place") && n == 5)
        {
            int dq, p;
            float mu;
            arb_place((uint32_t)strtoull(a[1], nullptr, 10), atoi(a[2]), strtoull(a[3], nullptr, 10), atoi(a[4]), &dq, &p, &mu);
            printf("%d %d %a\n", dq, p, (double)mu);
        }
        else if (!strcmp(a[0], "shape") && n == 4)
        {
            const uint64_t R = strtoull(a[3], nullptr, 10);
            if (!arb_valid((uint32_t)atoi(a[1]), (uint32_t)atoi(a[2]), R))
                return 2;
            const ArbShape s = arb_shape(atoi(a[1]), atoi(a[2]), R);
            printf("%d %d %d %d %d %d %zu\n", s.K, s.KP, s.P, s.tile_out, s.x_len, s.tap_entries, arb_lds_bytes(s));
        }
        else if (!strcmp(a[0], "table") && n == 3)
        {
            const int b = atoi(a[1]), T = atoi(a[2]);
            if (!arb_valid((uint32_t)T, (uint32_t)b, ARB_MIN_STEP))
                return 2;
            const ArbShape s = arb_shape(T, b, ARB_MIN_STEP);
            std::vector<float> h(T), g((size_t)s.tap_entries * 2, -1.0f);
            for (int k = 0; k < T; k++)
                h[k] = (float)(k + 1);
            arb_build_taps(h.data(), T, b, g.data());
            printf("%d %d\n", s.K, s.KP);
            for (int p = 0; p < s.P; p++, printf("\n"))
                for (int j = 0; j < s.KP; j++)
                    printf("%g:%g ", g[((size_t)p * s.KP + j) * 2], g[((size_t)p * s.KP + j) * 2 + 1]);
        }
        else if (!strcmp(a[0], "step") && n == 3)
            printf("%" PRIu64 "\n", arb_step_from_rates(strtod(a[1], nullptr), strtod(a[2], nullptr)));
        else
            return 2;
    }
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 2 && !strcmp(argv[1], "query"))
        return query();
    if (argc != 1)
        return 2;
    unsigned long long tables = 0, tiles = 0, calls = 0;
    std::vector<uint64_t> steps = {ARB_MIN_STEP, ARB_MIN_STEP + 1, ((uint64_t)1 << 32) - 1, (uint64_t)1 << 32, ((uint64_t)1 << 32) + 1,
                                   ARB_MAX_STEP - 1, ARB_MAX_STEP};
    for (int i = 0; i < 20; i++)
        steps.push_back(ARB_MIN_STEP + rnd() % (ARB_MAX_STEP - ARB_MIN_STEP + 1));
    for (int b = ARB_MIN_BITS; b <= ARB_MAX_BITS; b++)
    {
        const int P = 1 << b;
        const int Ts[6] = {1, P - 1, P, P + 1, 255, ARB_MAX_TAPS};
        for (int T : Ts)
        {
            const int K = arb_phase_taps(T, b), KP = arb_row_stride(K);
            if (K < 1 || K > 512 || KP < K || KP % 2 == 0)
                return fail("phase taps", b, T, 0, K, KP);
            // the table, in a heap buffer of exactly its size
            std::vector<float> h(T);
            for (int k = 0; k < T; k++)
                h[k] = (float)(k + 1);
            float *g = new float[(size_t)2 * P * KP];
            arb_build_taps(h.data(), T, b, g);
            for (int p = 0; p < P; p++)
                for (int j = 0; j < KP; j++)
                    for (int e = 0; e < 2; e++)
                    {
                        const int k = p + e + j * P;
                        const float want = (j < K && k < T) ? (float)(k + 1) : 0.0f;
                        if (g[((size_t)p * KP + j) * 2 + e] != want)
                        {
                            delete[] g;
                            return fail("table entry", b, T, 0, p, j);
                        }
                    }
            delete[] g;
            tables++;
            for (uint64_t R : steps)
            {
                if (!arb_valid((uint32_t)T, (uint32_t)b, R))
                    return fail("arb_valid", b, T, R, 0, 0);
                const ArbShape s = arb_shape(T, b, R);
                if (arb_lds_bytes(s) > (size_t)ARB_LDS_MAX || s.tile_out != ARB_TILE_OUT || s.tap_entries != P * KP)
                    return fail("shape", b, T, R, arb_lds_bytes(s), s.x_len);
                const uint64_t offsets[4] = {0, 1, R - 1, ((uint64_t)1 << 34) - 1};
                const uint64_t tile_ids[5] = {0, 1, 4194303, ((uint64_t)1 << 32) / ARB_TILE_OUT, (ARB_MAX_SAMPLES * 64) / ARB_TILE_OUT};
                for (uint64_t off : offsets)
                    for (uint64_t tile : tile_ids)
                    {
                        const uint64_t i = tile * ARB_TILE_OUT;
                        int64_t q0;
                        uint32_t f0;
                        arb_time(off, i, R, &q0, &f0);
                        const arb_u128 t = (arb_u128)off + (arb_u128)i * R;
                        if ((arb_u128)q0 != t >> 32 || f0 != (uint32_t)t)
                            return fail("arb_time", b, T, R, off, i);
                        const int ls[6] = {0, 1, 255, 256, ARB_TILE_OUT - 2, ARB_TILE_OUT - 1};
                        for (int l : ls)
                        {
                            int dq, p;
                            float mu;
                            arb_place(f0, l, R, b, &dq, &p, &mu);
                            const arb_u128 tl = t + (arb_u128)l * R;
                            const uint32_t f = (uint32_t)tl;
                            if ((arb_u128)(q0 + dq) != tl >> 32 || p != (int)(f >> (32 - b)) || p < 0 || p >= P || !(mu >= 0.0f) || !(mu <= 1.0f) ||
                                dq < 0 || dq + K > s.x_len)
                                return fail("arb_place", b, T, R, off, (unsigned long long)l);
                            // mu: the low bits scaled, rounded once
                            const float want = (float)(f & ((1u << (32 - b)) - 1u)) / (float)(1u << (32 - b));
                            if (mu != want)
                                return fail("mu", b, T, R, off, (unsigned long long)l);
                        }
                        tiles++;
                    }
            }
        }
    }
    // a random walk of calls and retunes from positions below and above 2^32 and at 2^63
    const uint64_t starts[4] = {0, ((uint64_t)1 << 32) - 5, ((uint64_t)1 << 40) + 12345, (uint64_t)1 << 63};
    for (uint64_t start : starts)
    {
        uint64_t c = start, R = steps[rnd() % steps.size()];
        arb_u128 tau = ((arb_u128)c << 32) + rnd() % R;
        for (int k = 0; k < 20000; k++)
        {
            const uint64_t pick = rnd() % 8;
            const uint64_t n = pick == 0 ? 0 : pick < 4 ? rnd() % 4 : pick < 7 ? rnd() % 5000 : rnd() % ((uint64_t)1 << 30);
            if (rnd() % 3 == 0)
                R = rnd() % 2 ? steps[rnd() % steps.size()] : ARB_MIN_STEP + rnd() % (ARB_MAX_STEP - ARB_MIN_STEP + 1);
            uint64_t count = 0;
            if (!arb_out_count(c, tau, n, R, &count))
                return fail("arb_out_count refused", 0, 0, R, c, n);
            const arb_u128 end = (arb_u128)(c + n) << 32;
            // the outputs emitted are exactly those below the end of the call
            if (count && !(tau + (arb_u128)(count - 1) * R < end))
                return fail("an output past the call", 0, 0, R, c, n);
            if (!(tau + (arb_u128)count * R >= end))
                return fail("an output left behind", 0, 0, R, c, n);
            c += n;
            tau += (arb_u128)count * R;
            if (!arb_state_ok(c, tau))
                return fail("state invariant", 0, 0, R, c, n);
            calls++;
        }
    }
    uint64_t count = 0;
    if (arb_out_count(UINT64_MAX - 3, (arb_u128)(UINT64_MAX - 3) << 32, 4, ARB_MIN_STEP, &count))
        return fail("a position past 2^64 was not refused", 0, 0, 0, 0, 0);
    printf("%llu tables, %llu tiles, %llu calls checked: OK\n", tables, tiles, calls);
    return 0;
}
