// resamp_plan_check.cpp — walks qo-100-tools_amd/csrc/if_fir_resamp_plan.h, the planning the resampler's shim and kernel use, with a
// plain host compiler (tests/test_resamp_host.py; may also be built with -fsanitize=address,undefined and run directly).
//
// Every (L, M) in 1..64 x 1..64 with T in {1, L-1, L, L+1, 255, 4096}: the tile shape fits its LDS budget and the tap table is
// h[p + j L] with zeros elsewhere; for stream positions c in {0, 1, M-1, 2^32-1, 2^32, 2^40+7} and N in {0, 1, 2, L, M, 1000}:
// count = ceil((c+N)L/M) - ceil(cL/M) (128-bit arithmetic here), t0 = m0 M - c L < M, the period table satisfies
// p_r + L dq_r = t0 + r M, every tap index touched is < T or lands on a zero pad, and every input index touched by the call's
// first and last L outputs lies in [-(K-1), N).
//
// `resamp_plan_check table L T` prints the table of taps h[k] = k + 1 (rows of KP entries) for the Python test to compare;
// `resamp_plan_check shape L M T` prints K, W, B, tile_out and tile_in of resamp_shape.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "if_fir_resamp_plan.h"

typedef unsigned __int128 u128;

static int fail(const char *what, int L, int M, int T, unsigned long long c, unsigned long long n)
{
    printf("FAILED: %s at L=%d M=%d T=%d c=%llu N=%llu\n", what, L, M, T, c, n);
    return 1;
}

int main(int argc, char **argv)
{
    using namespace if_fir;
    if (argc == 4 && argv[1][0] == 't')
    {
        const int L = atoi(argv[2]), T = atoi(argv[3]);
        if (L < 1 || L > RESAMP_MAX_L || T < 1 || T > RESAMP_MAX_TAPS)
            return 2;
        const int K = resamp_phase_taps(T, L), KP = resamp_row_stride(K);
        std::vector<float> h(T), g((size_t)L * KP, -1.0f);
        for (int k = 0; k < T; k++)
            h[k] = (float)(k + 1);
        resamp_build_taps(h.data(), T, 0, L, g.data());
        printf("%d %d\n", K, KP);
        for (int p = 0; p < L; p++, printf("\n"))
            for (int j = 0; j < KP; j++)
                printf("%g ", g[(size_t)p * KP + j]);
        return 0;
    }
    if (argc == 5 && argv[1][0] == 's')
    {
        const int L = atoi(argv[2]), M = atoi(argv[3]), T = atoi(argv[4]);
        if (L < 1 || L > RESAMP_MAX_L || M < 1 || M > RESAMP_MAX_M || T < 1 || T > RESAMP_MAX_TAPS)
            return 2;
        const ResampShape s = resamp_shape(T, L, M);
        printf("%d %d %d %d %d\n", s.K, s.W, s.B, s.tile_out, s.tile_in);
        return 0;
    }
    unsigned long long shapes = 0, calls = 0;
    for (int L = 1; L <= RESAMP_MAX_L; L++)
        for (int M = 1; M <= RESAMP_MAX_M; M++)
        {
            const int Ts[6] = {1, L - 1, L, L + 1, 255, 4096};
            for (int T : Ts)
            {
                if (T < 1)
                    continue;
                shapes++;
                const ResampShape s = resamp_shape(T, L, M);
                const int K = s.K;
                if (K != (T + L - 1) / L || s.KP < K || !(s.KP & 1) || s.W % L || s.W <= 0 || s.W > RESAMP_THREADS || s.B < 1 ||
                    s.tile_out != s.B * L || s.tile_in != s.B * M || s.tile_out > s.W * RESAMP_R || s.x_len != s.tile_in + K - 1 ||
                    s.x_len > RESAMP_X_MAX || s.tap_entries != L * s.KP || resamp_lds_bytes(s, 1) > (size_t)RESAMP_LDS_MAX ||
                    resamp_hist_len(T, L) != K - 1)
                    return fail("tile shape", L, M, T, 0, 0);
                // the table: taps k + 1 (real) and (k + 1, -(k + 1)) (complex), the rest zero
                std::vector<float> h(2 * (size_t)T), g((size_t)s.tap_entries, -1.0f), gc(2 * (size_t)s.tap_entries, -1.0f);
                for (int k = 0; k < T; k++)
                    h[k] = (float)(k + 1);
                resamp_build_taps(h.data(), T, 0, L, g.data());
                for (int k = 0; k < T; k++)
                {
                    h[2 * k] = (float)(k + 1);
                    h[2 * k + 1] = -(float)(k + 1);
                }
                resamp_build_taps(h.data(), T, 1, L, gc.data());
                for (int p = 0; p < L; p++)
                    for (int j = 0; j < s.KP; j++)
                    {
                        const int k = p + j * L;
                        const float want = (j < K && k < T) ? (float)(k + 1) : 0.0f;
                        const size_t at = (size_t)p * s.KP + j;
                        if (g[at] != want || gc[2 * at] != want || gc[2 * at + 1] != -want)
                            return fail("tap table", L, M, T, (unsigned long long)p, (unsigned long long)j);
                    }
                const unsigned long long cs[6] = {0, 1, (unsigned long long)(M - 1), 4294967295ull, 4294967296ull, (1ull << 40) + 7};
                const unsigned long long ns[6] = {0, 1, 2, (unsigned long long)L, (unsigned long long)M, 1000};
                for (unsigned long long c : cs)
                    for (unsigned long long n : ns)
                    {
                        calls++;
                        ResampCall call;
                        if (!resamp_call(c, n, L, M, &call))
                            return fail("resamp_call refused", L, M, T, c, n);
                        const u128 m0 = ((u128)c * L + M - 1) / M, m1 = ((u128)(c + n) * L + M - 1) / M;
                        if ((u128)call.m0 != m0 || (u128)call.count != m1 - m0)
                            return fail("count", L, M, T, c, n);
                        if (call.t0 >= (uint32_t)M || (u128)call.t0 != m0 * M - (u128)c * L)
                            return fail("t0", L, M, T, c, n);
                        for (int r = 0; r < L; r++)
                        {
                            int p, dq;
                            resamp_period_entry((int)call.t0, r, L, M, &p, &dq);
                            if (p < 0 || p >= L || dq < 0 || dq >= M || p + L * dq != (int)call.t0 + r * M)
                                return fail("period table", L, M, T, c, n);
                            for (int j = 0; j < K; j++) // a tap index past T must land on a zero pad of row p
                                if (p + j * L >= T && g[(size_t)p * s.KP + j] != 0.0f)
                                    return fail("tap index", L, M, T, c, n);
                        }
                        // the call's first and last L outputs: q from the period table = floor((t0 + i M) / L), inside the call
                        for (int pass = 0; pass < 2; pass++)
                            for (unsigned long long d = 0; d < (unsigned long long)L && d < call.count; d++)
                            {
                                const unsigned long long i = pass ? call.count - 1 - d : d;
                                int p, dq;
                                resamp_period_entry((int)call.t0, (int)(i % L), L, M, &p, &dq);
                                const long long q = (long long)(i / L) * M + dq;
                                if ((u128)q != ((u128)call.t0 + (u128)i * M) / L || q < 0 || q >= (long long)n)
                                    return fail("input index", L, M, T, c, n);
                                if (q - (K - 1) < -(long long)(K - 1))
                                    return fail("history reach", L, M, T, c, n);
                                // inside its tile: the lane's LDS window [x0, x0 + K - 1]
                                const long long tile = (long long)(i / s.tile_out), il = (long long)(i % s.tile_out);
                                const long long x0 = (il / L) * M + dq;
                                if (x0 + K - 1 >= s.x_len || tile * s.tile_in + x0 != q)
                                    return fail("tile window", L, M, T, c, n);
                            }
                    }
            }
        }
    ResampCall call;
    if (resamp_call(~0ull - 5, 10, 3, 2, &call))
        return fail("a stream position past 2^64 was accepted", 3, 2, 1, ~0ull - 5, 10);
    printf("%llu shapes, %llu calls checked: OK\n", shapes, calls);
    return 0;
}
