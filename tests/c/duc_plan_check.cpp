// duc_plan_check.cpp — walks qo-100-tools_amd/csrc/if_fir_duc_plan.h, the planning the up-converter's shim and kernel use, with
// a plain host compiler (tests/test_duc_host.py builds it with -fsanitize=address,undefined and runs it directly).
//
// Every L in 1..64 with T in {1, L-1, L, L+1, 2L, 2L+1, 15L, 16L, 16L+1, 17L, 33L, 255, 1023, 4095, 4096} (the row and segment
// edges): the tile shape fits its LDS budget; the fill writes every window sample once; every 16-byte read of the first and the
// last lane of a run is aligned, inside the window area and -- except the look-ahead pair that no FMA uses -- written; every
// 16-byte store into the staging area is aligned and every element of it is written once; the store pass finds the output
// q L + p at stage[p RS + q] through the multiply-shift division, for EVERY output index of a tile; the joins fall on
// even entries and the last one on KP; the table holds the pair of the tap p + j L at row p, entry KP-1-j, zeros elsewhere;
// and -- the index algebra of the kernel -- output q of a tile finds the sample of the tap (p, j) at window index q + KP-1-j
// of the window that starts KP - 1 samples before the tile's first input.  For stream positions c around 2^32, at 2^40 + 3 and
// near 2^64 / L, and N in {0, 1, 2, L, 1000}: count = N L, and a call whose (c + N) L passes 2^64 is refused (128-bit
// arithmetic here).
//
// `duc_plan_check shape T L` prints K, KP, top, Q, tile_out, RS, LDS bytes, workgroups per CU; `duc_plan_check table T L` the
// table of the taps (k + 1, -(k + 1)), one row per line; `duc_plan_check call c N L` the count or `refused`; `duc_plan_check
// mix T word` the pairs of duc_mix_taps for h[k] = (k + 1) / T, real and complex, as hexadecimal floats; `duc_plan_check i16
// v...` duc_to_i16 of each hexadecimal float.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "if_fir_duc_plan.h"

typedef unsigned __int128 u128;

static int fail(const char *what, int T, int L, unsigned long long c, unsigned long long n)
{
    printf("FAILED: %s at T=%d L=%d c=%llu N=%llu\n", what, T, L, c, n);
    return 1;
}

int main(int argc, char **argv)
{
    using namespace if_fir;
    if (argc == 4 && (argv[1][0] == 's' || argv[1][0] == 't'))
    {
        const int T = atoi(argv[2]), L = atoi(argv[3]);
        if (L < 1 || L > DUC_MAX_L || T < 1 || T > DUC_MAX_TAPS)
            return 2;
        const DucShape s = duc_shape(T, L);
        if (argv[1][0] == 's')
        {
            printf("%d %d %d %d %d %d %zu %d\n", s.K, s.KP, s.top, s.Q, s.tile_out, s.RS, duc_lds_bytes(s, L), duc_groups_per_cu(s, L));
            return 0;
        }
        std::vector<float> g(2 * (size_t)T), tab(2 * (size_t)s.tap_entries, -1.0f);
        for (int k = 0; k < T; k++)
        {
            g[2 * k] = (float)(k + 1);
            g[2 * k + 1] = -(float)(k + 1);
        }
        duc_build_table(g.data(), T, L, tab.data());
        for (int r = 0; r < L; r++, printf("\n"))
            for (int e = 0; e < 2 * s.KP; e++)
                printf("%g ", tab[(size_t)r * 2 * s.KP + e]);
        return 0;
    }
    if (argc == 5 && argv[1][0] == 'c')
    {
        uint64_t count;
        const unsigned long long c = strtoull(argv[2], nullptr, 10), n = strtoull(argv[3], nullptr, 10);
        if (!duc_call(c, n, atoi(argv[4]), &count))
        {
            printf("refused\n");
            return 0;
        }
        printf("%llu\n", (unsigned long long)count);
        return 0;
    }
    if (argc == 4 && argv[1][0] == 'm')
    {
        const int T = atoi(argv[2]);
        const uint32_t word = (uint32_t)strtoull(argv[3], nullptr, 10);
        if (T < 1 || T > DUC_MAX_TAPS)
            return 2;
        std::vector<float> h(2 * (size_t)T), g(2 * (size_t)T), gc(2 * (size_t)T);
        for (int k = 0; k < T; k++)
            h[k] = (float)(k + 1) / (float)T;
        duc_mix_taps(h.data(), T, 0, word, g.data());
        for (int k = T - 1; k >= 0; k--) // the same taps as complex ones (im = -re / 2)
        {
            h[2 * k] = h[k];
            h[2 * k + 1] = -0.5f * h[k];
        }
        duc_mix_taps(h.data(), T, 1, word, gc.data());
        for (int k = 0; k < T; k++)
            printf("%a %a %a %a\n", g[2 * k], g[2 * k + 1], gc[2 * k], gc[2 * k + 1]);
        return 0;
    }
    if (argc >= 2 && argv[1][0] == 'i')
    {
        for (int i = 2; i < argc; i++)
            printf("%d\n", (int)duc_to_i16(strtof(argv[i], nullptr)));
        return 0;
    }
    unsigned long long shapes = 0, calls = 0;
    for (int L = 1; L <= DUC_MAX_L; L++)
    {
        const int Ts[15] = {1, L - 1, L, L + 1, 2 * L, 2 * L + 1, 15 * L, 16 * L, 16 * L + 1, 17 * L, 33 * L, 255, 1023, 4095, 4096};
        for (int T : Ts)
        {
            if (T < 1 || T > DUC_MAX_TAPS)
                continue;
            shapes++;
            const DucShape s = duc_shape(T, L);
            const int K = s.K, KP = s.KP;
            if (K != (T + L - 1) / L || KP % 2 || KP < K || KP > K + 1 || K != duc_phase_taps(T, L) || KP != duc_row_taps(T, L))
                return fail("row taps", T, L, 0, 0);
            // the joins: after `top` entries, then after every 16th; the last one after the row's last entry
            if (s.top < 2 || s.top > DUC_SEG || s.top % 2 || (KP - s.top) % DUC_SEG || s.top - (KP - K) != K - ((K - 1) / DUC_SEG) * DUC_SEG)
                return fail("segments", T, L, 0, 0);
            if (s.Q < DUC_RUN || s.Q % DUC_RUN || s.Q > DUC_Q_MAX || s.tile_out != s.Q * L || s.tile_out > DUC_TILE_OUT_MAX || s.tile_out % 2 ||
                (s.Q < DUC_Q_MAX && (s.Q + DUC_RUN) * L <= DUC_TILE_OUT_MAX) || s.window != s.Q + KP - 1 || s.RS % 4 || s.RS < s.Q ||
                s.x_floats != 2 * (s.Q + KP) || s.x_floats % 4 || s.tap_entries != L * KP ||
                duc_lds_bytes(s, L) != ((size_t)s.x_floats + (size_t)s.RS * L) * 4 || duc_lds_bytes(s, L) > (size_t)DUC_LDS_MAX)
                return fail("tile shape", T, L, 0, 0);
            const int per_cu = duc_groups_per_cu(s, L);
            if (per_cu < 1 || per_cu > 8 || (size_t)per_cu * duc_lds_bytes(s, L) > (size_t)DUC_LDS_PER_CU ||
                (per_cu < 8 && (size_t)(per_cu + 1) * duc_lds_bytes(s, L) <= (size_t)DUC_LDS_PER_CU))
                return fail("workgroups per CU", T, L, 0, 0);
            // the fill: thread tid writes the window samples tid, tid + 256, ...
            std::vector<char> written((size_t)s.x_floats / 2, 0);
            for (int tid = 0; tid < DUC_THREADS; tid++)
                for (int w = tid; w < s.window; w += DUC_THREADS)
                {
                    if (w >= s.x_floats / 2 || written[(size_t)w])
                        return fail("fill", T, L, (unsigned long long)w, 0);
                    written[(size_t)w] = 1;
                }
            // the reads of a run's first and last lane, every run: pairs of samples at q0 + 2 i, i = 0 .. KP / 2 + 1; the FMAs
            // of step e use the samples q0 + e .. q0 + e + 4
            const int lanes[2] = {0, 63};
            for (int qb = 0; qb < s.Q / DUC_RUN; qb++)
                for (int lane : lanes)
                {
                    const int q0 = qb * DUC_RUN + DUC_R * lane;
                    for (int i = 0; i <= KP / 2 + 1; i++)
                        if ((2 * (q0 + 2 * i)) % 4 || 2 * (q0 + 2 * i) + 3 >= s.x_floats)
                            return fail("window read", T, L, (unsigned long long)q0, (unsigned long long)i);
                    for (int e = 0; e < KP; e += 2)
                        for (int u = 0; u <= 4; u++)
                            if (!written[(size_t)(q0 + e + u)])
                                return fail("window sample", T, L, (unsigned long long)q0, (unsigned long long)e);
                }
            // the staging area: the 16-byte store of (p, q0), then the store pass's element of every output index
            std::vector<char> staged((size_t)s.RS * L, 0);
            for (int it = 0; it < L * (s.Q / DUC_RUN); it++)
            {
                const int qb = it / L, p = it - qb * L;
                for (int lane = 0; lane < 64; lane++)
                {
                    const int at = p * s.RS + qb * DUC_RUN + DUC_R * lane;
                    if (at % 4 || at + 3 >= s.RS * L)
                        return fail("stage store", T, L, (unsigned long long)it, (unsigned long long)lane);
                    for (int u = 0; u < 4; u++)
                    {
                        if (staged[(size_t)(at + u)])
                            return fail("stage store twice", T, L, (unsigned long long)it, (unsigned long long)lane);
                        staged[(size_t)(at + u)] = 1;
                    }
                }
            }
            const uint32_t magic = duc_div_magic(L);
            for (int n = 0; n < s.tile_out; n++)
            {
                const int q = (int)(((uint64_t)n * magic) >> DUC_DIV_SHIFT), p = n - q * L;
                if (q != n / L || p != n % L || !staged[(size_t)(p * s.RS + q)])
                    return fail("store pass", T, L, (unsigned long long)n, 0);
            }
            // the table and the index algebra
            std::vector<float> g(2 * (size_t)T), tab(2 * (size_t)s.tap_entries, -1.0f);
            for (int k = 0; k < T; k++)
            {
                g[2 * k] = (float)(k + 1);
                g[2 * k + 1] = -(float)(k + 1);
            }
            duc_build_table(g.data(), T, L, tab.data());
            const int outs[3] = {0, 1, s.Q - 1};
            for (int p = 0; p < L; p++)
                for (int e = 0; e < KP; e++)
                {
                    const int j = KP - 1 - e, k = p + j * L;
                    const float want = k < T ? (float)(k + 1) : 0.0f;
                    if (tab[2 * ((size_t)p * KP + e)] != want || tab[2 * ((size_t)p * KP + e) + 1] != -want)
                        return fail("tap table", T, L, (unsigned long long)p, (unsigned long long)e);
                    for (int q : outs)
                    {
                        // input q of the tile sits at window index KP - 1 + q; the tap j wants the input q - j
                        const int w = KP - 1 + q - j;
                        if (w != q + e || w < 0 || w >= s.window)
                            return fail("window index", T, L, (unsigned long long)k, (unsigned long long)q);
                    }
                }
            const unsigned long long uL = (unsigned long long)L, top = ~0ull / uL;
            const unsigned long long cs[12] = {0, 1, 4294967293ull, 4294967295ull, 4294967296ull, 4294967299ull, (1ull << 40) + 3,
                                               1ull << 57, top - 1000, top - 1, top, ~0ull - 1000};
            const unsigned long long ns[5] = {0, 1, 2, uL, 1000};
            for (unsigned long long c : cs)
                for (unsigned long long n : ns)
                {
                    calls++;
                    uint64_t count = 0;
                    const bool fits = ((u128)c + n) * uL <= (u128)~0ull;
                    if (duc_call(c, n, L, &count) != fits)
                        return fail(fits ? "duc_call refused" : "a position past 2^64 was accepted", T, L, c, n);
                    if (fits && (u128)count != (u128)n * uL)
                        return fail("count", T, L, c, n);
                }
        }
    }
    // the int16 rule at ties, at the rails and beyond
    const float vs[10] = {0.5f / 32768, 1.5f / 32768, 2.5f / 32768, -0.5f / 32768, -1.5f / 32768, 32766.5f / 32768, 1.0f, -1.0f, -1.7f, 1.7f};
    const int want[10] = {0, 2, 2, 0, -2, 32766, 32767, -32768, -32768, 32767};
    for (int i = 0; i < 10; i++)
        if (duc_to_i16(vs[i]) != want[i])
            return fail("int16 rule", 0, 0, (unsigned long long)i, 0);
    printf("%llu shapes, %llu calls checked: OK\n", shapes, calls);
    return 0;
}
