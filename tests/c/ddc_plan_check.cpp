// ddc_plan_check.cpp — walks qo-100-tools_amd/csrc/if_fir_ddc_plan.h, the planning the down-converter's shim and kernel use, with
// a plain host compiler (tests/test_ddc_host.py builds it with -fsanitize=address,undefined and runs it directly).
//
// Every D in 1..64 with T in {1, D-1, D, D+1, 4D, 4D+1, 16D, 16D+1, 17D, 255, 1023, 4095, 4096} (the row and segment edges): the
// tile shape fits its LDS budget, every LDS word the kernel's fill writes and every 16-byte read of every lane lies inside
// it, the table holds g[rho + j D] at row D-1-rho, entry K-1-j, zeros elsewhere, and -- the index algebra of the kernel --
// output i of a tile finds the sample of tap (rho, j) at row D-1-rho, column K-1-j+i of the window that starts K D - 1 samples
// before the tile's first output.  For stream positions c in {0, 1, D-1, D, 2^32-3 .. 2^32+3, 2^40+3, 2^63, 2^63+D-1} and N
// in {0, 1, 2, D-1, D, D+1, 1000}: n0 < D, c + n0 = 0 mod D, count = the outputs in [c, c+N) (128-bit arithmetic here); a
// position past 2^64 is refused.
//
// `ddc_plan_check shape T D` prints K, G, tile_out, tile_in, cols, RS; `ddc_plan_check table T D` the table of the taps
// (k + 1, -(k + 1)), one row per line; `ddc_plan_check call c N D` n0, count, first; `ddc_plan_check mix T word` the taps
// g[k] of ddc_mix_taps for h[k] = (k + 1) / T as hexadecimal floats.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "if_fir_ddc_plan.h"

typedef unsigned __int128 u128;

static int fail(const char *what, int T, int D, unsigned long long c, unsigned long long n)
{
    printf("FAILED: %s at T=%d D=%d c=%llu N=%llu\n", what, T, D, c, n);
    return 1;
}

int main(int argc, char **argv)
{
    using namespace if_fir;
    if (argc == 4 && (argv[1][0] == 's' || argv[1][0] == 't'))
    {
        const int T = atoi(argv[2]), D = atoi(argv[3]);
        if (D < 1 || D > DDC_MAX_D || T < 1 || T > DDC_MAX_TAPS)
            return 2;
        const DdcShape s = ddc_shape(T, D);
        if (argv[1][0] == 's')
        {
            printf("%d %d %d %d %d %d\n", s.K, s.G, s.tile_out, s.tile_in, s.cols, s.RS);
            return 0;
        }
        std::vector<float> g(2 * (size_t)T), tab(2 * (size_t)s.tap_entries, -1.0f);
        for (int k = 0; k < T; k++)
        {
            g[2 * k] = (float)(k + 1);
            g[2 * k + 1] = -(float)(k + 1);
        }
        ddc_build_table(g.data(), T, D, tab.data());
        for (int r = 0; r < D; r++, printf("\n"))
            for (int e = 0; e < 2 * s.K; e++)
                printf("%g ", tab[(size_t)r * 2 * s.K + e]);
        return 0;
    }
    if (argc == 5 && argv[1][0] == 'c')
    {
        DdcCall call;
        const unsigned long long c = strtoull(argv[2], nullptr, 10), n = strtoull(argv[3], nullptr, 10);
        if (!ddc_call(c, n, atoi(argv[4]), &call))
        {
            printf("refused\n");
            return 0;
        }
        printf("%u %llu %llu\n", call.n0, (unsigned long long)call.count, (unsigned long long)call.first);
        return 0;
    }
    if (argc == 4 && argv[1][0] == 'm')
    {
        const int T = atoi(argv[2]);
        const uint32_t word = (uint32_t)strtoull(argv[3], nullptr, 10);
        if (T < 1 || T > DDC_MAX_TAPS)
            return 2;
        std::vector<float> h(2 * (size_t)T), g(2 * (size_t)T), gc(2 * (size_t)T);
        for (int k = 0; k < T; k++)
            h[k] = (float)(k + 1) / (float)T;
        ddc_mix_taps(h.data(), T, 0, word, g.data());
        for (int k = T - 1; k >= 0; k--) // the same taps as complex ones (im = -re / 2)
        {
            h[2 * k] = h[k];
            h[2 * k + 1] = -0.5f * h[k];
        }
        ddc_mix_taps(h.data(), T, 1, word, gc.data());
        for (int k = 0; k < T; k++)
            printf("%a %a %a %a\n", g[2 * k], g[2 * k + 1], gc[2 * k], gc[2 * k + 1]);
        return 0;
    }
    unsigned long long shapes = 0, calls = 0;
    for (int D = 1; D <= DDC_MAX_D; D++)
    {
        const int Ts[13] = {1, D - 1, D, D + 1, 4 * D, 4 * D + 1, 16 * D, 16 * D + 1, 17 * D, 255, 1023, 4095, 4096};
        for (int T : Ts)
        {
            if (T < 1 || T > DDC_MAX_TAPS)
                continue;
            shapes++;
            const DdcShape s = ddc_shape(T, D);
            const int K = s.K;
            if (K % 4 || K < (T + D - 1) / D || K >= (T + D - 1) / D + 4 || K != ddc_row_taps(T, D))
                return fail("row taps", T, D, 0, 0);
            if (s.G != (K <= DDC_SEG ? DDC_SEG / K : 1) || s.G < 1 || (K <= DDC_SEG && s.G * K > DDC_SEG))
                return fail("rows per segment", T, D, 0, 0);
            if (s.tile_out < 4 || s.tile_out % 4 || s.tile_out > DDC_THREADS * DDC_R || s.tile_in != s.tile_out * D ||
                s.cols != s.tile_out + K || s.RS < s.cols || s.RS % 4 || (s.RS / 4) % 2 != 1 || s.RS * D > DDC_X_MAX ||
                ddc_lds_bytes(s, D) > (size_t)DDC_LDS_MAX || ddc_lds_bytes(s, D) != (size_t)s.RS * D * 4 || s.tap_entries != D * K)
                return fail("tile shape", T, D, 0, 0);
            const int per_cu = ddc_groups_per_cu(s, D);
            if (per_cu < 1 || per_cu > 8 || (size_t)per_cu * ddc_lds_bytes(s, D) > (size_t)DDC_LDS_PER_CU ||
                (per_cu < 8 && (size_t)(per_cu + 1) * ddc_lds_bytes(s, D) <= (size_t)DDC_LDS_PER_CU))
                return fail("workgroups per CU", T, D, 0, 0);
            // the fill: item q writes the 4 floats at row RS + 4 cq, for the window samples (4 cq + u) D + row
            const long long lds_floats = (long long)ddc_lds_bytes(s, D) / 4, window = (long long)s.cols * D;
            std::vector<char> written((size_t)lds_floats, 0);
            const int items = (s.cols / 4) * D;
            for (int q = 0; q < items; q++)
            {
                const int cq = q / D, row = q - cq * D;
                for (int u = 0; u < 4; u++)
                {
                    const long long at = (long long)row * s.RS + 4 * cq + u, w = (long long)(4 * cq + u) * D + row;
                    if (at < 0 || at >= lds_floats || written[(size_t)at] || w < 0 || w >= window || w % D != row || w / D != 4 * cq + u)
                        return fail("fill", T, D, (unsigned long long)q, (unsigned long long)u);
                    written[(size_t)at] = 1;
                }
            }
            // the reads of the first and the last working lane, every row: 16 bytes at e and at e + 4, aligned and written
            const int lanes[2] = {0, s.tile_out / DDC_R - 1};
            for (int lane : lanes)
                for (int r = 0; r < D; r++)
                    for (int e = 0; e <= K; e += 4)
                        for (int u = 0; u < 4; u++)
                        {
                            const long long at = (long long)r * s.RS + DDC_R * lane + e + u;
                            if ((at - u) % 4 || at >= lds_floats || !written[(size_t)at])
                                return fail("row read", T, D, (unsigned long long)lane, (unsigned long long)e);
                        }
            // the table and the index algebra
            std::vector<float> g(2 * (size_t)T), tab(2 * (size_t)s.tap_entries, -1.0f);
            for (int k = 0; k < T; k++)
            {
                g[2 * k] = (float)(k + 1);
                g[2 * k + 1] = -(float)(k + 1);
            }
            ddc_build_table(g.data(), T, D, tab.data());
            const int outs[3] = {0, 1, s.tile_out - 1};
            for (int r = 0; r < D; r++)
                for (int e = 0; e < K; e++)
                {
                    const int rho = D - 1 - r, j = K - 1 - e, k = rho + j * D;
                    const float want = k < T ? (float)(k + 1) : 0.0f;
                    if (tab[2 * ((size_t)r * K + e)] != want || tab[2 * ((size_t)r * K + e) + 1] != -want)
                        return fail("tap table", T, D, (unsigned long long)r, (unsigned long long)e);
                    for (int i : outs)
                    {
                        // window sample of (output i, tap k): the output sits at window index K D - 1 + i D
                        const long long w = (long long)K * D - 1 + (long long)i * D - k;
                        if (w < 0 || w >= window || w % D != r || w / D != e + i || e + i >= s.cols - 1)
                            return fail("window index", T, D, (unsigned long long)k, (unsigned long long)i);
                    }
                }
            const unsigned long long uD = (unsigned long long)D;
            const unsigned long long cs[15] = {0, 1, uD - 1, uD, 4294967293ull, 4294967294ull, 4294967295ull, 4294967296ull, 4294967297ull,
                                               4294967298ull, 4294967299ull, (1ull << 40) + 3, 1ull << 63, (1ull << 63) + uD - 1,
                                               ~0ull - 1000};
            const unsigned long long ns[7] = {0, 1, 2, uD - 1, uD, uD + 1, 1000};
            for (unsigned long long c : cs)
                for (unsigned long long n : ns)
                {
                    calls++;
                    DdcCall call;
                    if (!ddc_call(c, n, D, &call))
                        return fail("ddc_call refused", T, D, c, n);
                    const u128 first = ((u128)c + D - 1) / D, last = ((u128)c + n + D - 1) / D; // outputs m with c <= m D < c + n
                    if (call.n0 >= (uint32_t)D || (u128)(c + call.n0) % D != 0 || (u128)call.n0 != first * D - c)
                        return fail("n0", T, D, c, n);
                    if ((u128)call.count != last - first)
                        return fail("count", T, D, c, n);
                    if (call.count && (call.first != c + call.n0 || call.first + (call.count - 1) * uD >= c + n))
                        return fail("first", T, D, c, n);
                }
        }
    }
    DdcCall call;
    if (ddc_call(~0ull - 5, 10, 3, &call))
        return fail("a stream position past 2^64 was accepted", 1, 3, ~0ull - 5, 10);
    printf("%llu shapes, %llu calls checked: OK\n", shapes, calls);
    return 0;
}
