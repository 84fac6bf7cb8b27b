// stream_plan_check.cpp — walks qo-100-tools_amd/csrc/if_fir_stream_plan.h, what the plan headers of the streaming families
// share, with a plain host compiler (tests/test_stream_plan_host.py builds it with -fsanitize=address,undefined and runs it
// directly).  Each function against a restatement in 128-bit arithmetic or by brute force:
//
//   stream_decim_call    D in 1..64 and 65, 4095, 4096; c in {0, 1, D-1, D, 2^32-3 .. 2^32+3, 2^40+3, 2^63, 2^63+D-1, 2^64-1-n};
//                        n in {0, 1, 2, D-1, D, D+1, 1000}: n0 < D, c + n0 = 0 mod D, count = the multiples of D in [c, c + n),
//                        counted one by one; c + n = 2^64 is refused and writes nothing
//   stream_groups_per_cu every byte count k KB - 2 .. k KB + 2, k = 0 .. 2 STREAM_LDS_PER_CU / 1 KB, from 1 byte on: the largest
//                        g <= 8 with g bytes <= STREAM_LDS_PER_CU, at least 1
//   stream_top_segment   every K in 1..4096: in 1..16, and K - top is a multiple of 16
//   stream_mix_taps      words {0, 1, 2^31, 2^32-1, llround(0.2 2^32)}, real and complex taps, T in {1, 2, 255}, against
//                        h e^{+j 2 pi ((P k) mod 2^32) / 2^32} in long double: within half a float32 ulp of it, plus what the
//                        header's float64 evaluation may be off before it rounds (bound derived at mix_slack below); word 0
//                        gives the taps bit for bit
//   stream_size_ok       every size in 0..8193 at the lower bounds 64 and 256
//   stream_bank_batch, stream_bank_lds_bytes   the seven bank sizes
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "if_fir_stream_plan.h"

typedef unsigned __int128 u128;
typedef unsigned long long ull;

static int fail(const char *what, ull a, ull b, ull c)
{
    printf("FAILED: %s at %llu %llu %llu\n", what, a, b, c);
    return 1;
}

// The header evaluates g in float64 and rounds once.  Before that rounding its value is off the exact one by at most:
// a = 2 pi f carries the roundings of the constant and of the product, |da| <= 2 pi 2^-52 < 1.4e-15, which moves cos a and
// sin a by as much; their own roundings, the two products' and the sum's add less than 5 2^-53 < 5.6e-16.  Together below
// 2^-48 = 3.6e-15 per unit of |h_r| + |h_i|.
static long double mix_slack(long double hr, long double hi)
{
    return (fabsl(hr) + fabsl(hi)) * ldexpl(1.0L, -48);
}

// half the spacing of float32 around a value of magnitude |v| (the binade of v itself; subnormal spacing below 2^-126)
static long double half_ulp_f32(long double v)
{
    if (v == 0.0L)
        return ldexpl(1.0L, -150);
    const int e = ilogbl(fabsl(v));
    return ldexpl(1.0L, (e < -126 ? -126 : e) - 24);
}

int main()
{
    using namespace if_fir;
    ull checks = 0;

    std::vector<ull> Ds;
    for (ull D = 1; D <= 64; D++)
        Ds.push_back(D);
    Ds.push_back(65);
    Ds.push_back(4095);
    Ds.push_back(4096);
    for (ull D : Ds)
    {
        const ull ns[7] = {0, 1, 2, D - 1, D, D + 1, 1000};
        for (ull n : ns)
        {
            const ull cs[15] = {0, 1, D - 1, D, 4294967293ull, 4294967294ull, 4294967295ull, 4294967296ull, 4294967297ull,
                                4294967298ull, 4294967299ull, (1ull << 40) + 3, 1ull << 63, (1ull << 63) + D - 1, ~0ull - n};
            for (ull c : cs)
            {
                checks++;
                uint32_t n0 = 0xdeadbeefu;
                uint64_t count = 0xdeadbeefdeadbeefull;
                if (!stream_decim_call(c, n, D, &n0, &count))
                    return fail("stream_decim_call refused", D, c, n);
                const u128 first = ((u128)c + D - 1) / D, last = ((u128)c + n + D - 1) / D; // multiples m D with c <= m D < c + n
                if (n0 >= D || ((u128)c + n0) % D != 0 || (u128)n0 != first * D - c)
                    return fail("n0", D, c, n);
                ull brute = 0;
                for (u128 a = c; a < (u128)c + n; a++)
                    brute += a % D == 0;
                if ((u128)count != last - first || count != brute)
                    return fail("count", D, c, n);
                if (count && ((u128)c + n0 + (u128)(count - 1) * D >= (u128)c + n))
                    return fail("last output", D, c, n);
            }
            if (n)
            {
                // c + n = 2^64: refused, nothing written
                checks++;
                uint32_t n0 = 0xdeadbeefu;
                uint64_t count = 0xdeadbeefdeadbeefull;
                if (stream_decim_call(~0ull - n + 1, n, D, &n0, &count) || n0 != 0xdeadbeefu || count != 0xdeadbeefdeadbeefull)
                    return fail("a position past 2^64 was accepted", D, ~0ull - n + 1, n);
            }
        }
    }

    for (long long kb = 0; kb <= 2 * STREAM_LDS_PER_CU / 1024; kb++)
        for (long long d = -2; d <= 2; d++)
        {
            const long long bytes = kb * 1024 + d;
            if (bytes < 1)
                continue;
            checks++;
            int want = 1;
            for (int g = 2; g <= 8; g++)
                if ((u128)g * (u128)bytes <= (u128)STREAM_LDS_PER_CU)
                    want = g;
            if (stream_groups_per_cu((size_t)bytes) != want)
                return fail("stream_groups_per_cu", (ull)bytes, (ull)want, 0);
        }
    static_assert(stream_groups_per_cu(1) == 8 && stream_groups_per_cu(STREAM_LDS_PER_CU) == 1, "usable in constant expressions");

    for (int K = 1; K <= 4096; K++)
    {
        checks++;
        const int top = stream_top_segment(K);
        if (top < 1 || top > STREAM_SEG || (K - top) % STREAM_SEG || STREAM_SEG != 16)
            return fail("stream_top_segment", (ull)K, (ull)top, 0);
    }

    const uint32_t words[5] = {0u, 1u, 1u << 31, 0xffffffffu, (uint32_t)llround(0.2 * 4294967296.0)};
    const int Ts[3] = {1, 2, 255};
    for (uint32_t word : words)
        for (int T : Ts)
            for (int ctaps = 0; ctaps < 2; ctaps++)
            {
                std::vector<float> h((size_t)T * (ctaps ? 2 : 1)), g(2 * (size_t)T, -7.0f);
                for (int k = 0; k < T; k++)
                {
                    const float v = (float)(k + 1) / (float)T;
                    if (ctaps)
                    {
                        h[2 * k] = v;
                        h[2 * k + 1] = -0.5f * v;
                    }
                    else
                        h[k] = v;
                }
                stream_mix_taps(h.data(), T, ctaps, word, g.data());
                for (int k = 0; k < T; k++)
                {
                    checks++;
                    const float fr = ctaps ? h[2 * k] : h[k], fi = ctaps ? h[2 * k + 1] : 0.0f;
                    if (word == 0)
                    {
                        if (memcmp(&g[2 * k], &fr, 4) || memcmp(&g[2 * k + 1], &fi, 4))
                            return fail("word 0 changes the taps", (ull)T, (ull)ctaps, (ull)k);
                        continue;
                    }
                    const long double hr = fr, hi = fi;
                    const long double a = 6.283185307179586476925286766559L * ((long double)(uint32_t)(word * (uint32_t)k) / 4294967296.0L);
                    const long double wr = hr * cosl(a) - hi * sinl(a), wi = hr * sinl(a) + hi * cosl(a);
                    if (fabsl((long double)g[2 * k] - wr) > half_ulp_f32(wr) + mix_slack(hr, hi) ||
                        fabsl((long double)g[2 * k + 1] - wi) > half_ulp_f32(wi) + mix_slack(hr, hi))
                        return fail("stream_mix_taps", (ull)word, (ull)T * 2 + ctaps, (ull)k);
                }
            }

    for (uint32_t size = 0; size <= 8193; size++)
    {
        checks++;
        const bool pow2 = size == 64 || size == 128 || size == 256 || size == 512 || size == 1024 || size == 2048 || size == 4096;
        if (stream_size_ok(size, 64) != pow2 || stream_size_ok(size, 256) != (pow2 && size >= 256))
            return fail("stream_size_ok", size, 0, 0);
    }

    for (uint32_t M = 64; M <= 4096; M *= 2)
    {
        checks++;
        uint32_t B = 1;
        while (B * M < (uint32_t)STREAM_BANK_POINTS)
            B++;
        if (stream_bank_batch(M) != B || stream_bank_lds_bytes(M) != (size_t)B * M * 8 + (size_t)M * 10)
            return fail("bank shape", M, B, 0);
    }

    printf("%llu checks: OK\n", checks);
    return 0;
}
