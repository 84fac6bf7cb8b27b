// pfb_plan_check.cpp — walks qo-100-tools_amd/csrc/if_fir_pfb_plan.h, the planning the polyphase filter bank's shim and kernel
// use, with a plain host compiler (tests/test_pfb_host.py builds it plain and with -fsanitize=address,undefined and runs it
// directly).
//
// Without arguments, every M of the list with T in {1, M-1, M, M+1, 3M-5, 16M-1, 16M} and D in {1, 17, M/2, 3M/4, M-1, M}: the
// batch fills the 256 lanes, a workgroup's run is whole batches, the LDS fits; the tap table, built into a heap buffer of
// exactly its size, holds h[r M + M-1-q] at (r, q) and zeros from T on; the bin places are a permutation; and -- the index
// algebra of the kernel -- the sample of item (q, r) of a frame at a lies at a - t, t = M-1-q + r M, never before the T - 1
// carried samples when t < T, and its slot (a + 1 + q) mod M is (a - t) mod M, at positions up to 2^64 (128-bit arithmetic here).
// For stream positions c in {0, 1, D-1, D, 2^32-1, 2^32, 2^32+1, 2^40+12345, 2^63, 2^63+D-1, 2^64-1001} and N in {0, 1, 2, D-1,
// D, D+1, 1000, 2^36}: n0 < D, c + n0 = 0 mod D, frames = the m with c <= m D < c + N, groups, c mod M, carry; a position past
// 2^64 is refused.
//
// `pfb_plan_check query` answers one request per line of standard input: `call c N M D T` -> frames groups n0 cmod carry (or
// `refused`), `shape M T` -> K batch group_frames lds_bytes groups_per_cu, `taps M T` -> the table of the taps k + 1, one row
// per line, `place M first_bin j` -> channel place.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "if_fir_pfb_plan.h"

typedef unsigned __int128 u128;

static int fail(const char *what, unsigned M, unsigned T, unsigned D, unsigned long long c, unsigned long long n)
{
    printf("FAILED: %s at M=%u T=%u D=%u c=%llu N=%llu\n", what, M, T, D, c, n);
    return 1;
}

static int query()
{
    using namespace if_fir;
    char line[256], word[16];
    while (fgets(line, sizeof line, stdin))
    {
        unsigned long long c = 0, n = 0;
        unsigned M = 0, D = 0, T = 0;
        int first = 0;
        if (sscanf(line, "%15s", word) != 1)
            continue;
        if (!strcmp(word, "call") && sscanf(line, "%*s %llu %llu %u %u %u", &c, &n, &M, &D, &T) == 5)
        {
            PfbCall call;
            if (!pfb_call(c, n, M, D, T, &call))
                printf("refused\n");
            else
                printf("%llu %llu %u %u %u\n", (unsigned long long)call.frames, (unsigned long long)call.groups, call.n0, call.cmod, call.carry);
        }
        else if (!strcmp(word, "shape") && sscanf(line, "%*s %u %u", &M, &T) == 2 && pfb_size_ok(M))
            printf("%u %u %u %zu %d\n", pfb_rows(T, M), pfb_batch(M), pfb_group_frames(M), pfb_lds_bytes(M), pfb_groups_per_cu(M));
        else if (!strcmp(word, "taps") && sscanf(line, "%*s %u %u", &M, &T) == 2 && pfb_size_ok(M) && T >= 1 && T <= PFB_MAX_ROWS * M)
        {
            const unsigned K = pfb_rows(T, M);
            std::vector<float> h(T), tab((size_t)K * M, -1.0f);
            for (unsigned k = 0; k < T; k++)
                h[k] = (float)(k + 1);
            pfb_build_taps(h.data(), T, M, tab.data());
            for (unsigned r = 0; r < K; r++, printf("\n"))
                for (unsigned q = 0; q < M; q++)
                    printf("%g ", tab[(size_t)r * M + q]);
        }
        else if (!strcmp(word, "place") && sscanf(line, "%*s %u %d %u", &M, &first, &D) == 3 && pfb_size_ok(M))
            printf("%u %u\n", pfb_bin_channel(first, D, M), pfb_bin_place(first, D, M));
        else
        {
            printf("bad request: %s", line);
            return 2;
        }
    }
    return 0;
}

int main(int argc, char **argv)
{
    using namespace if_fir;
    if (argc == 2 && !strcmp(argv[1], "query"))
        return query();
    if (argc != 1)
        return 2;
    unsigned long long shapes = 0, calls = 0;
    const unsigned Ms[7] = {64, 128, 256, 512, 1024, 2048, 4096};
    if (pfb_size_ok(32) || pfb_size_ok(96) || pfb_size_ok(8192) || pfb_size_ok(0))
        return fail("a size outside the list was accepted", 0, 0, 0, 0, 0);
    for (unsigned M : Ms)
    {
        if (!pfb_size_ok(M))
            return fail("size refused", M, 0, 0, 0, 0);
        const unsigned B = pfb_batch(M), GF = pfb_group_frames(M);
        if (B < 1 || B * M < (unsigned)PFB_BATCH_POINTS || (B > 1 && B * M != (unsigned)PFB_BATCH_POINTS) || (B * M) % PFB_THREADS || GF % B ||
            GF < 8 || GF < 2 * B)
            return fail("batch", M, 0, 0, 0, 0);
        const int per_cu = pfb_groups_per_cu(M);
        if (pfb_lds_bytes(M) != (size_t)B * M * 8 + (size_t)M * 10 || per_cu < 1 || per_cu > 8 ||
            (size_t)per_cu * pfb_lds_bytes(M) > (size_t)PFB_LDS_PER_CU ||
            (per_cu < 8 && (size_t)(per_cu + 1) * pfb_lds_bytes(M) <= (size_t)PFB_LDS_PER_CU))
            return fail("LDS", M, 0, 0, 0, 0);
        // the bin places: a permutation of the block, the same for every span start
        std::vector<char> seen(M, 0);
        for (unsigned j = 0; j < M; j++)
        {
            const unsigned p = pfb_bin_place(-(int)(M / 2), j, M);
            if (p >= M || seen[p] || pfb_bin_channel(-(int)(M / 2), j, M) != (j + M / 2) % M || pfb_bin_channel((int)M - 1, j, M) != (M - 1 + j) % M)
                return fail("bin place", M, 0, 0, j, 0);
            seen[p] = 1;
        }
        const unsigned Ts[7] = {1, M - 1, M, M + 1, 3 * M - 5, 16 * M - 1, 16 * M};
        const unsigned Ds[6] = {1, 17, M / 2, 3 * M / 4, M - 1, M};
        for (unsigned T : Ts)
        {
            shapes++;
            const unsigned K = pfb_rows(T, M);
            if (K < 1 || K > (unsigned)PFB_MAX_ROWS || K * M < T || (K - 1) * M >= T)
                return fail("rows", M, T, 0, 0, 0);
            std::vector<float> h(T);
            for (unsigned k = 0; k < T; k++)
                h[k] = (float)(k + 1);
            float *tab = (float *)malloc((size_t)K * M * sizeof(float)); // exactly its size: the sanitizer sees one float more
            if (!tab)
                return fail("out of memory", M, T, 0, 0, 0);
            pfb_build_taps(h.data(), T, M, tab);
            for (unsigned r = 0; r < K; r++)
                for (unsigned q = 0; q < M; q++)
                {
                    const unsigned t = M - 1 - q + r * M;
                    if (tab[(size_t)r * M + q] != (t < T ? (float)(t + 1) : 0.0f))
                    {
                        free(tab);
                        return fail("tap table", M, T, 0, r, q);
                    }
                }
            free(tab);
            for (unsigned D : Ds)
            {
                const unsigned long long uD = D;
                const unsigned long long cs[11] = {0, 1, uD - 1, uD, 4294967295ull, 4294967296ull, 4294967297ull, (1ull << 40) + 12345, 1ull << 63,
                                                   (1ull << 63) + uD - 1, ~0ull - 1000};
                const unsigned long long ns[8] = {0, 1, 2, uD - 1, uD, uD + 1, 1000, 1ull << 36};
                for (unsigned long long c : cs)
                    for (unsigned long long n : ns)
                    {
                        calls++;
                        PfbCall call;
                        const bool past = (u128)c + n > ~0ull;
                        if (pfb_call(c, n, M, D, T, &call) == past)
                            return fail(past ? "a position past 2^64 was accepted" : "pfb_call refused", M, T, D, c, n);
                        if (past)
                            continue;
                        const u128 first = ((u128)c + D - 1) / D, last = ((u128)c + n + D - 1) / D; // frames m with c <= m D < c + n
                        if ((u128)call.frames != last - first)
                            return fail("frames", M, T, D, c, n);
                        if (call.frames && (call.n0 >= D || ((u128)c + call.n0) % D != 0 || (u128)call.n0 != first * D - c))
                            return fail("n0", M, T, D, c, n);
                        if (call.groups != (call.frames + GF - 1) / GF || call.cmod != (unsigned)(c % M) || call.carry != T - 1)
                            return fail("groups, c mod M or carry", M, T, D, c, n);
                        // the first and the last frame of the call, the lanes at both ends, every row
                        const unsigned long long fs[2] = {0, call.frames ? call.frames - 1 : 0};
                        for (unsigned long long f : fs)
                        {
                            if (!call.frames)
                                break;
                            const unsigned long long a_rel = call.n0 + f * uD; // < n
                            if (a_rel >= n)
                                return fail("a frame beyond the call", M, T, D, c, n);
                            const unsigned qs[3] = {0, M / 2 + 1, M - 1};
                            for (unsigned q : qs)
                                for (unsigned r = 0; r < K; r++)
                                {
                                    const unsigned t = M - 1 - q + r * M;
                                    if (t >= T)
                                        continue;
                                    // not before the history: a_rel - t >= -(T - 1)
                                    if ((long long)a_rel - (long long)t < -(long long)(T - 1))
                                        return fail("a read before the history", M, T, D, c, n);
                                    const u128 a = (u128)c + a_rel;
                                    const unsigned slot = (unsigned)((a_rel + call.cmod + 1u + q) & (M - 1)); // the kernel's
                                    if ((u128)slot != ((a + ((u128)1 << 100)) - t) % M)
                                        return fail("slot", M, T, D, c, n);
                                }
                        }
                    }
            }
        }
    }
    PfbCall call;
    if (pfb_call(~0ull - 5, 10, 64, 3, 100, &call) || pfb_call(5, 10, 64, 0, 100, &call))
        return fail("a stream position past 2^64, or a zero hop, was accepted", 64, 100, 3, ~0ull - 5, 10);
    printf("%llu shapes, %llu calls checked: OK\n", shapes, calls);
    return 0;
}
