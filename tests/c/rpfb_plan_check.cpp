// rpfb_plan_check.cpp — walks qo-100-tools_amd/csrc/if_fir_rpfb_plan.h, the planning the real-input polyphase filter bank's shim
// and kernel use, with a plain host compiler (tests/test_rpfb_host.py builds it plain and with -fsanitize=address,undefined and
// runs it directly).
//
// Without arguments, every M of the list with T in {1, M-1, M, M+1, 3M-5, 16M-1, 16M} and D in {1, 17, M/2, 3M/4, M-1, M}: the
// batch fills the 256 lanes of the fold and of every transform pass, a workgroup's run is whole batches, the LDS fits; the tap
// table, built into a heap buffer of exactly its size, holds h[r M + M-1-q] at (r, q) and zeros from T on; for EVERY channel
// k = 0 .. M/2 (0, M/4 and M/2 among them) the place of Z[k] and the place of its partner Z[M/2 - k] are those of an M/2-point
// transform walked digit by digit here, the places of k < M/2 are a permutation, k and M/2 - k swap places with their partners,
// and the kernel's table packs the two; the untangling twiddles are e^{-j 2 pi k / M} with W^0 = (1, 0), W^{M/8} = (s, -s),
// W^{M/4} = (~0, -1) and W^{M/2} = (-1, ~0); and -- the index algebra of the kernel -- the sample of item (q, r) of a frame at a lies at a - t,
// t = M-1-q + r M, never before the T - 1 carried samples when t < T, and its slot (a + 1 + q) mod M is (a - t) mod M, at
// positions up to 2^64 - 1 (128-bit arithmetic here).  For stream positions c in {0, 1, D-1, D, 2^32-1, 2^32, 2^32+1,
// 2^40+12345, 2^63, 2^63+D-1, 2^64-1001} and N in {0, 1, 2, D-1, D, D+1, 1000, 2^36}: n0 < D, c + n0 = 0 mod D, frames = the m
// with c <= m D < c + N, groups, c mod M, carry; a position past 2^64 is refused.
//
// `rpfb_plan_check query` answers one request per line of standard input: `call c N M D T` -> frames groups n0 cmod carry (or
// `refused`), `shape M T` -> K batch group_frames lds_bytes groups_per_cu, `taps M T` -> the table of the taps k + 1, one row
// per line, `place M k` -> place partner_place, `span M first_bin bins` -> ok / refused, `size M` -> ok / refused.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "if_fir_rpfb_plan.h"

typedef unsigned __int128 u128;

static int fail(const char *what, unsigned M, unsigned T, unsigned D, unsigned long long c, unsigned long long n)
{
    printf("FAILED: %s at M=%u T=%u D=%u c=%llu N=%llu\n", what, M, T, D, c, n);
    return 1;
}

// where an N-point transform of radix-4 passes (and a last radix-2 one) leaves bin k: its digits reversed
static unsigned digit_reverse(unsigned k, unsigned N)
{
    unsigned pos = 0;
    for (unsigned len = N; len > 1;)
    {
        const unsigned r = len >= 4 ? 4 : 2;
        pos += (k % r) * (len / r);
        k /= r;
        len /= r;
    }
    return pos;
}

static int query()
{
    using namespace if_fir;
    char line[256], word[16];
    while (fgets(line, sizeof line, stdin))
    {
        unsigned long long c = 0, n = 0;
        unsigned M = 0, D = 0, T = 0;
        if (sscanf(line, "%15s", word) != 1)
            continue;
        if (!strcmp(word, "call") && sscanf(line, "%*s %llu %llu %u %u %u", &c, &n, &M, &D, &T) == 5)
        {
            RpfbCall call;
            if (!rpfb_call(c, n, M, D, T, &call))
                printf("refused\n");
            else
                printf("%llu %llu %u %u %u\n", (unsigned long long)call.frames, (unsigned long long)call.groups, call.n0, call.cmod, call.carry);
        }
        else if (!strcmp(word, "shape") && sscanf(line, "%*s %u %u", &M, &T) == 2 && rpfb_size_ok(M))
            printf("%u %u %u %zu %d\n", rpfb_rows(T, M), rpfb_batch(M), rpfb_group_frames(M), rpfb_lds_bytes(M), rpfb_groups_per_cu(M));
        else if (!strcmp(word, "taps") && sscanf(line, "%*s %u %u", &M, &T) == 2 && rpfb_size_ok(M) && T >= 1 && T <= RPFB_MAX_ROWS * M)
        {
            const unsigned K = rpfb_rows(T, M);
            std::vector<float> h(T), tab((size_t)K * M, -1.0f);
            for (unsigned k = 0; k < T; k++)
                h[k] = (float)(k + 1);
            rpfb_build_taps(h.data(), T, M, tab.data());
            for (unsigned r = 0; r < K; r++, printf("\n"))
                for (unsigned q = 0; q < M; q++)
                    printf("%g ", tab[(size_t)r * M + q]);
        }
        else if (!strcmp(word, "place") && sscanf(line, "%*s %u %u", &M, &D) == 2 && rpfb_size_ok(M) && D <= M / 2)
            printf("%u %u\n", rpfb_bin_place(D, M), rpfb_partner_place(D, M));
        else if (!strcmp(word, "span") && sscanf(line, "%*s %u %u %u", &M, &D, &T) == 3 && rpfb_size_ok(M))
            printf("%s\n", rpfb_span_ok(D, T, M) ? "ok" : "refused");
        else if (!strcmp(word, "size") && sscanf(line, "%*s %u", &M) == 1)
            printf("%s\n", rpfb_size_ok(M) ? "ok" : "refused");
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
    const unsigned Ms[7] = {128, 256, 512, 1024, 2048, 4096, 8192};
    if (rpfb_size_ok(64) || rpfb_size_ok(96) || rpfb_size_ok(16384) || rpfb_size_ok(0) || rpfb_size_ok(129) || rpfb_size_ok(1))
        return fail("a size outside the list was accepted", 0, 0, 0, 0, 0);
    for (unsigned M : Ms)
    {
        if (!rpfb_size_ok(M))
            return fail("size refused", M, 0, 0, 0, 0);
        const unsigned H = M / 2, B = rpfb_batch(M), GF = rpfb_group_frames(M);
        if (B < 1 || B * H < (unsigned)STREAM_BANK_POINTS || (B > 1 && B * H != (unsigned)STREAM_BANK_POINTS) || (B * M) % RPFB_THREADS ||
            (B * H / 4) % RPFB_THREADS || GF % B || GF < 8 || GF < 2 * B)
            return fail("batch", M, 0, 0, 0, 0);
        const int per_cu = rpfb_groups_per_cu(M);
        if (rpfb_lds_bytes(M) != (size_t)B * H * 8 + (size_t)H * 12 || per_cu < 1 || per_cu > 8 ||
            (size_t)per_cu * rpfb_lds_bytes(M) > (size_t)RPFB_LDS_PER_CU ||
            (per_cu < 8 && (size_t)(per_cu + 1) * rpfb_lds_bytes(M) <= (size_t)RPFB_LDS_PER_CU) || (M == 8192 && per_cu != 2))
            return fail("LDS", M, 0, 0, 0, 0);
        if (!rpfb_span_ok(0, H + 1, M) || !rpfb_span_ok(H, 1, M) || !rpfb_span_ok(0, 1, M) || rpfb_span_ok(0, H + 2, M) || rpfb_span_ok(H + 1, 1, M) ||
            rpfb_span_ok(1, H + 1, M) || rpfb_span_ok(0, 0, M) || rpfb_span_ok(4294967295u, 2, M) || rpfb_span_ok(2, 4294967295u, M))
            return fail("span", M, 0, 0, 0, 0);
        // the places of every channel and of its partner
        std::vector<char> seen(H, 0);
        std::vector<uint32_t> packed(H, ~0u);
        rpfb_build_places(M, packed.data());
        for (unsigned k = 0; k <= H; k++)
        {
            const unsigned p = rpfb_bin_place(k, M), pp = rpfb_partner_place(k, M);
            if (p >= H || pp >= H || p != digit_reverse(k % H, H) || pp != digit_reverse((H - k % H) % H, H))
                return fail("bin place", M, 0, 0, k, 0);
            if (rpfb_partner_place(H - k, M) != p || rpfb_bin_place(H - k, M) != pp)
                return fail("a channel and its partner do not swap places", M, 0, 0, k, 0);
            if (k < H)
            {
                if (seen[p] || packed[k] != (p | pp << 16))
                    return fail("the places are no permutation, or the packed table differs", M, 0, 0, k, 0);
                seen[p] = 1;
            }
        }
        if (rpfb_bin_place(0, M) != 0 || rpfb_partner_place(0, M) != 0 || rpfb_bin_place(H, M) != 0 || rpfb_partner_place(H, M) != 0 ||
            rpfb_bin_place(M / 4, M) != rpfb_partner_place(M / 4, M))
            return fail("the places of k = 0, M/4, M/2", M, 0, 0, 0, 0);
        // the untangling twiddles
        float *tw = (float *)malloc((size_t)(H + 1) * 2 * sizeof(float)); // exactly its size
        if (!tw)
            return fail("out of memory", M, 0, 0, 0, 0);
        rpfb_build_twiddles(M, tw);
        bool tw_ok = tw[0] == 1.0f && tw[1] == 0.0f && tw[2 * H] == -1.0f && fabsf(tw[2 * H + 1]) < 1e-15f &&
                     fabsf(tw[2 * (M / 4)]) < 1e-15f && tw[2 * (M / 4) + 1] == -1.0f && tw[2 * (M / 8)] == (float)sqrt(0.5) &&
                     tw[2 * (M / 8) + 1] == -(float)sqrt(0.5);
        for (unsigned k = 0; k <= H && tw_ok; k++)
        {
            const double a = -2.0 * M_PI * (double)k / (double)M;
            tw_ok = fabs((double)tw[2 * k] - cos(a)) <= 6e-8 && fabs((double)tw[2 * k + 1] - sin(a)) <= 6e-8;
        }
        free(tw);
        if (!tw_ok)
            return fail("untangling twiddles", M, 0, 0, 0, 0);
        const unsigned Ts[7] = {1, M - 1, M, M + 1, 3 * M - 5, 16 * M - 1, 16 * M};
        const unsigned Ds[6] = {1, 17, M / 2, 3 * M / 4, M - 1, M};
        for (unsigned T : Ts)
        {
            shapes++;
            const unsigned K = rpfb_rows(T, M);
            if (K < 1 || K > (unsigned)RPFB_MAX_ROWS || K * M < T || (K - 1) * M >= T)
                return fail("rows", M, T, 0, 0, 0);
            std::vector<float> h(T);
            for (unsigned k = 0; k < T; k++)
                h[k] = (float)(k + 1);
            float *tab = (float *)malloc((size_t)K * M * sizeof(float)); // exactly its size: the sanitizer sees one float more
            if (!tab)
                return fail("out of memory", M, T, 0, 0, 0);
            rpfb_build_taps(h.data(), T, M, tab);
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
                        RpfbCall call;
                        const bool past = (u128)c + n > ~0ull;
                        if (rpfb_call(c, n, M, D, T, &call) == past)
                            return fail(past ? "a position past 2^64 was accepted" : "rpfb_call refused", M, T, D, c, n);
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
    RpfbCall call;
    if (rpfb_call(~0ull - 5, 10, 128, 3, 100, &call) || rpfb_call(5, 10, 128, 0, 100, &call) || !rpfb_call(~0ull - 5, 5, 128, 3, 100, &call) ||
        call.frames != (unsigned long long)(((u128)~0ull + 2) / 3 - ((u128)(~0ull - 5) + 2) / 3))
        return fail("a stream position past 2^64, or a zero hop, was accepted; or a call up to 2^64 - 1 went wrong", 128, 100, 3, ~0ull - 5, 10);
    printf("%llu shapes, %llu calls checked: OK\n", shapes, calls);
    return 0;
}
