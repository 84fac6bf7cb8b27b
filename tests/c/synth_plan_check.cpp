// synth_plan_check.cpp — walks qo-100-tools_amd/csrc/if_fir_synth_plan.h, the planning the polyphase synthesis bank's shim and
// kernels use, with a plain host compiler (tests/test_synth_host.py builds it plain and with -fsanitize=address,undefined and
// runs it directly).
//
// Without arguments, every M of the list with T in {1, L, L+1, M-1, M, 3M-5, 16M-1, 16M, 32L, 32L+1} (those within 1..16M) and L in
// {1, 17, M/2, 3M/4, M-1, M}: J = ceil(T / L), accepted up to 32 and refused from 33; the batch fills the 256 lanes and the
// transform kernel's LDS fits; the one-kernel route's LDS bytes, whether two (it can run) and four (the plan prefers it) of them
// fit a CU, its runs of batches and the ring slot an output's term reads; the tap table, built into a
// heap buffer of exactly its size, holds h[t] at t and zeros from T on; the places are the mirrored permutation; for workspace
// budgets from 1 byte to the default the chunks cover every frame of a call once, in order, a chunk's rows fit the workspace,
// every row an output reads lies inside it, and a chunk's first output index modulo M is the absolute one (128-bit arithmetic
// here); for frame positions c in {0, 1, 2^32-1, 2^32, 2^40+12345, 2^63, floor((2^64-1)/L) - 1000, 2^64-1001} and F in {0, 1, 2,
// 999, 1000, 1001, 2^32}: a call is refused exactly when (c + F) L passes 2^64 - 1, outputs = F L, (c L) mod M, carry = J - 1.
//
// `synth_plan_check query` answers one request per line of standard input: `config M T L` -> J (or `refused`), `call c F M L T`
// -> outputs smod carry (or `refused`), `shape M T L` -> batch lds_bytes groups_per_cu lds_route_bytes fits route ring_groups_per_cu, `route M T L
// forced` -> route (0 = refused), `chunks F bytes M T L smod` -> count, then first frames smod per chunk, `taps T L` -> the table
// of the taps k + 1, `place M s` -> place.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "if_fir_synth_plan.h"

typedef unsigned __int128 u128;

static int fail(const char *what, unsigned M, unsigned T, unsigned L, unsigned long long c, unsigned long long n)
{
    printf("FAILED: %s at M=%u T=%u L=%u c=%llu F=%llu\n", what, M, T, L, c, n);
    return 1;
}

static int query()
{
    using namespace if_fir;
    char line[256], word[16];
    while (fgets(line, sizeof line, stdin))
    {
        unsigned long long c = 0, n = 0;
        unsigned M = 0, L = 0, T = 0, s = 0;
        if (sscanf(line, "%15s", word) != 1)
            continue;
        if (!strcmp(word, "config") && sscanf(line, "%*s %u %u %u", &M, &T, &L) == 3)
        {
            if (synth_config_ok(M, T, L))
                printf("%u\n", synth_terms(T, L));
            else
                printf("refused\n");
        }
        else if (!strcmp(word, "call") && sscanf(line, "%*s %llu %llu %u %u %u", &c, &n, &M, &L, &T) == 5)
        {
            SynthCall call;
            if (!synth_call(c, n, M, L, T, &call))
                printf("refused\n");
            else
                printf("%llu %u %u\n", (unsigned long long)call.outputs, call.smod, call.carry);
        }
        else if (!strcmp(word, "shape") && sscanf(line, "%*s %u %u %u", &M, &T, &L) == 3 && synth_config_ok(M, T, L))
        {
            const unsigned J = synth_terms(T, L);
            printf("%u %zu %d %zu %d %u %d\n", synth_batch(M), synth_lds_bytes(M), synth_groups_per_cu(M), synth_lds_route_bytes(M, J),
                   (int)synth_lds_route_fits(M, J), synth_route(M, J, SYNTH_ROUTE_PLAN), synth_lds_route_groups_per_cu(M, J));
        }
        else if (!strcmp(word, "route") && sscanf(line, "%*s %u %u %u %u", &M, &T, &L, &s) == 4 && synth_config_ok(M, T, L))
            printf("%u\n", synth_route(M, synth_terms(T, L), s));
        else if (!strcmp(word, "chunks") && sscanf(line, "%*s %llu %llu %u %u %u %u", &n, &c, &M, &T, &L, &s) == 6 && synth_config_ok(M, T, L))
        {
            const unsigned J = synth_terms(T, L);
            const unsigned long long most = synth_chunk_frames(synth_workspace_frames(c, M, J), J), per = synth_even_chunk_frames(n, most),
                                     count = synth_chunks(n, per);
            printf("%llu", count);
            for (unsigned long long i = 0; i < count; i++)
            {
                const SynthChunk ch = synth_chunk(i, n, per, M, L, s);
                printf(" %llu %llu %u", (unsigned long long)ch.first, (unsigned long long)ch.frames, ch.smod);
            }
            printf("\n");
        }
        else if (!strcmp(word, "taps") && sscanf(line, "%*s %u %u", &T, &L) == 2 && T >= 1 && L >= 1 && synth_terms(T, L) <= 32)
        {
            const unsigned J = synth_terms(T, L);
            std::vector<float> h(T), tab((size_t)J * L, -1.0f);
            for (unsigned k = 0; k < T; k++)
                h[k] = (float)(k + 1);
            synth_build_taps(h.data(), T, L, tab.data());
            for (size_t k = 0; k < tab.size(); k++)
                printf("%g ", tab[k]);
            printf("\n");
        }
        else if (!strcmp(word, "place") && sscanf(line, "%*s %u %u", &M, &s) == 2 && synth_size_ok(M) && s < M)
            printf("%u\n", synth_slot_place(s, M));
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
    unsigned long long shapes = 0, calls = 0, chunks = 0;
    const unsigned Ms[7] = {64, 128, 256, 512, 1024, 2048, 4096};
    if (synth_size_ok(32) || synth_size_ok(96) || synth_size_ok(8192) || synth_size_ok(0))
        return fail("a size outside the list was accepted", 0, 0, 0, 0, 0);
    for (unsigned M : Ms)
    {
        if (!synth_size_ok(M))
            return fail("size refused", M, 0, 0, 0, 0);
        const unsigned B = synth_batch(M);
        if (B < 1 || B * M < (unsigned)SYNTH_BATCH_POINTS || (B > 1 && B * M != (unsigned)SYNTH_BATCH_POINTS) || (B * M) % SYNTH_THREADS)
            return fail("batch", M, 0, 0, 0, 0);
        const int per_cu = synth_groups_per_cu(M);
        if (synth_lds_bytes(M) != (size_t)B * M * 8 + (size_t)M * 10 || per_cu < 1 || per_cu > 8 ||
            (size_t)per_cu * synth_lds_bytes(M) > (size_t)SYNTH_LDS_PER_CU ||
            (per_cu < 8 && (size_t)(per_cu + 1) * synth_lds_bytes(M) <= (size_t)SYNTH_LDS_PER_CU))
            return fail("LDS", M, 0, 0, 0, 0);
        // the places: the permutation of the shared transform, mirrored; slot 0 is bin 0
        std::vector<char> seen(M, 0);
        for (unsigned s = 0; s < M; s++)
        {
            const unsigned p = synth_slot_place(s, M);
            if (p >= M || seen[p] || p != psd_bin_position((M - s) % M, M))
                return fail("place", M, 0, 0, s, 0);
            seen[p] = 1;
        }
        if (synth_slot_place(0, M) != 0)
            return fail("place of slot 0", M, 0, 0, 0, 0);
        // the element of a channel in a frame of a span (what the kernels call): element j holds channel (first + j) mod M
        for (unsigned k = 0; k < M; k++)
        {
            const int firsts[5] = {0, -(int)(M / 2), (int)M - 1, -3, 77 % (int)M};
            for (int first : firsts)
            {
                const unsigned j = synth_channel_index(first, k, M);
                if (j >= M || (unsigned)(((long long)first + j + M) % M) != k)
                    return fail("channel index", M, 0, 0, k, 0);
            }
        }
        const unsigned Ls[6] = {1, 17, M / 2, 3 * M / 4, M - 1, M};
        for (unsigned L : Ls)
        {
            const unsigned Ts[10] = {1, L, L + 1, M - 1, M, 3 * M - 5, 16 * M - 1, 16 * M, 32 * L, 32 * L + 1};
            for (unsigned T : Ts)
            {
                if (T < 1 || T > 16 * M)
                {
                    if (synth_config_ok(M, T, L))
                        return fail("taps outside 1..16 M accepted", M, T, L, 0, 0);
                    continue;
                }
                const unsigned J = synth_terms(T, L);
                if (J < 1 || (unsigned long long)J * L < T || (unsigned long long)(J - 1) * L >= T)
                    return fail("terms", M, T, L, 0, 0);
                if (synth_config_ok(M, T, L) != (J <= 32))
                    return fail(J <= 32 ? "a configuration with J <= 32 was refused" : "J = 33 or more was accepted", M, T, L, 0, 0);
                if (J > 32)
                    continue;
                shapes++;
                if (synth_config_ok(M, T, 0) || synth_config_ok(M, T, M + 1) || synth_config_ok(M, 0, L) || synth_config_ok(M, 16 * M + 1, L))
                    return fail("a hop or a tap count outside its range was accepted", M, T, L, 0, 0);
                const size_t ring = (size_t)((J - 1 + B - 1) / B + 1) * B * M * 8 + (size_t)M * 10;
                const bool fits = 2 * ring <= 160 * 1024;
                if (synth_lds_route_bytes(M, J) != ring || synth_lds_route_fits(M, J) != fits ||
                    synth_lds_route_preferred(M, J) != (4 * ring <= 160 * 1024) ||
                    synth_route(M, J, SYNTH_ROUTE_PLAN) != (unsigned)(4 * ring <= 160 * 1024 ? SYNTH_ROUTE_LDS : SYNTH_ROUTE_WORKSPACE) ||
                    synth_route(M, J, SYNTH_ROUTE_WORKSPACE) != SYNTH_ROUTE_WORKSPACE ||
                    synth_route(M, J, SYNTH_ROUTE_LDS) != (unsigned)(fits ? SYNTH_ROUTE_LDS : 0) || synth_route(M, J, 3) != 0 ||
                    (fits && (synth_lds_route_groups_per_cu(M, J) < 2 || synth_lds_route_groups_per_cu(M, J) > 8 ||
                              (size_t)synth_lds_route_groups_per_cu(M, J) * ring > 160 * 1024)))
                    return fail("route", M, T, L, 0, 0);
                // the ring route: runs of batches cover the call once; term j of the output of frame fbi of a batch reads frame
                // (fbi - j) mod B of the batch `back` batches ago, inside the ring of NB = ceil((J-1)/B) + 1 batches
                {
                    const unsigned NB = (J - 1 + B - 1) / B + 1;
                    for (unsigned fbi = 0; fbi < B; fbi++)
                        for (unsigned j = 0; j < J; j++)
                        {
                            const int back = j > fbi ? (int)((j - fbi + B - 1) / B) : 0, fb = ((int)fbi - (int)j) & (int)(B - 1);
                            const long long frame = 1000ll * B + fbi - j; // batch 1000
                            if (back < 0 || (unsigned)back > NB - 1 || frame != (1000ll - back) * B + fb)
                                return fail("ring slot", M, T, L, fbi, j);
                        }
                    const unsigned long long bs[5] = {1, 2, 7, 1000, 65536}, gs[4] = {1, 2, 3, 512};
                    for (unsigned long long nbat : bs)
                        for (unsigned long long g : gs)
                        {
                            const unsigned long long len = synth_run_batches(nbat, g < nbat ? g : nbat), runs = (nbat + len - 1) / len;
                            if (len < 1 || runs > g || runs * len < nbat || (runs - 1) * len >= nbat)
                                return fail("runs of batches", M, T, L, nbat, g);
                        }
                }
                std::vector<float> h(T);
                for (unsigned k = 0; k < T; k++)
                    h[k] = (float)(k + 1);
                float *tab = (float *)malloc((size_t)J * L * sizeof(float)); // exactly its size: the sanitizer sees one float more
                if (!tab)
                    return fail("out of memory", M, T, L, 0, 0);
                synth_build_taps(h.data(), T, L, tab);
                for (unsigned t = 0; t < J * L; t++)
                    if (tab[t] != (t < T ? (float)(t + 1) : 0.0f))
                    {
                        free(tab);
                        return fail("tap table", M, T, L, t, 0);
                    }
                free(tab);
                // chunking: budgets from nothing to the default, calls of 1 frame to many
                const unsigned long long budgets[5] = {1, (unsigned long long)M * 8 * (J + 1), (unsigned long long)M * 8 * (J + 6), 1ull << 20,
                                                       SYNTH_WORKSPACE_DEFAULT};
                const unsigned long long Fs[5] = {1, 2, J, 3ull * J + 7, 1000};
                const unsigned long long cs[3] = {0, (1ull << 40) + 12345, (~0ull / L) - 1000};
                for (unsigned long long bytes : budgets)
                {
                    const unsigned long long rows = synth_workspace_frames(bytes, M, J), most = synth_chunk_frames(rows, J);
                    if (rows < J || most < 1 || (rows > J && rows * M * 8 > bytes) || rows * M * 8 > SYNTH_WORKSPACE_MAX)
                        return fail("workspace", M, T, L, bytes, 0);
                    for (unsigned long long F : Fs)
                        for (unsigned long long c : cs)
                        {
                            SynthCall call;
                            if (!synth_call(c, F, M, L, T, &call))
                                return fail("synth_call refused", M, T, L, c, F);
                            const unsigned long long per = synth_even_chunk_frames(F, most), count = synth_chunks(F, per);
                            unsigned long long next = 0, shortest = ~0ull;
                            if (per < 1 || per > most || count != synth_chunks(F, most))
                                return fail("even chunks", M, T, L, c, F);
                            for (unsigned long long i = 0; i < count; i++)
                            {
                                chunks++;
                                const SynthChunk ch = synth_chunk(i, F, per, M, L, call.smod);
                                if (ch.first != next || ch.frames < 1 || ch.frames > per || ch.frames + J - 1 > rows)
                                    return fail("chunk", M, T, L, c, F);
                                if ((u128)ch.smod != (((u128)c + ch.first) * L) % M)
                                    return fail("chunk position mod M", M, T, L, c, F);
                                if (ch.frames * L >= (1ull << 31))
                                    return fail("a chunk's outputs do not fit 32 bits", M, T, L, c, F);
                                // the emit kernel's rows: output i of the chunk, term j reads row i / L + J - 1 - j
                                const unsigned long long last = ch.frames * L - 1;
                                if (last / L + J - 1 >= ch.frames + J - 1)
                                    return fail("a row beyond the chunk's", M, T, L, c, F);
                                next = ch.first + ch.frames;
                                shortest = ch.frames < shortest ? ch.frames : shortest;
                            }
                            if (per - shortest >= count)
                                return fail("a chunk much shorter than the others", M, T, L, c, F);
                            if (next != F)
                                return fail("chunks do not cover the call", M, T, L, c, F);
                        }
                }
                // calls at positions up to 2^64
                const unsigned long long ps[8] = {0, 1, 4294967295ull, 4294967296ull, (1ull << 40) + 12345, 1ull << 63, (~0ull / L) - 1000, ~0ull - 1000};
                const unsigned long long ns[7] = {0, 1, 2, 999, 1000, 1001, 1ull << 32};
                for (unsigned long long c : ps)
                    for (unsigned long long F : ns)
                    {
                        calls++;
                        SynthCall call;
                        const bool past = ((u128)c + F) * L > (u128)~0ull;
                        if (synth_call(c, F, M, L, T, &call) == past)
                            return fail(past ? "a position past 2^64 was accepted" : "synth_call refused", M, T, L, c, F);
                        if (past)
                            continue;
                        if ((u128)call.outputs != (u128)F * L || (u128)call.smod != ((u128)c * L) % M || call.carry != J - 1)
                            return fail("outputs, (c L) mod M or carry", M, T, L, c, F);
                    }
            }
        }
    }
    SynthCall call;
    if (synth_call(~0ull - 5, 10, 64, 3, 100, &call) || synth_call(5, 10, 64, 0, 100, &call) || synth_call(~0ull / 3, 1, 64, 3, 100, &call))
        return fail("a position past 2^64, or a zero hop, was accepted", 64, 100, 3, ~0ull - 5, 10);
    printf("%llu shapes, %llu calls, %llu chunks checked: OK\n", shapes, calls, chunks);
    return 0;
}
