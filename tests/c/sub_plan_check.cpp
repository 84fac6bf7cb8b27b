// sub_plan_check.cpp — walks qo-100-tools_amd/csrc/if_fir_sub_plan.h, the planning the per-channel FIR stage's shim and kernel
// use, with a plain host compiler (tests/test_sub_host.py builds it with -fsanitize=address,undefined and runs it directly).
//
// Without arguments:
//  - the call plan for every R = 1 .. 64 at positions c in {0, 1, R-1, R, 2^32-1, 2^32, 2^32+1, 2^63, 2^64-1001} and F in {0, 1,
//    2, R-1, R, R+1, 701, 1000, 2^32}: n0 < R, c + n0 = 0 mod R, count = the a with c <= a < c + F and a mod R = 0, a0 = the low
//    32 bits of c + n0; a position past 2^64 is refused (128-bit arithmetic here);
//  - the tile plan for B in {1, 63, 64, 65, 4095, 4096} and output counts around every edge of SUB_OUT and of a tile: every
//    (output, bin) of the call belongs to exactly one item, item = run B + j, the items of a tile are consecutive, the tiles
//    cover the items and only the last one is ragged; the index algebra of the kernel: the element under output o, tap k of bin
//    j is (n0 + o R - k) B + j, never before the (T - 1) B carried elements, and an item the kernel takes for interior reads
//    nothing outside the call; the largest offsets fit 63 bits;
//  - the tap-major table built into a heap buffer of exactly its size: g_j[k] at k B + j, one row for all bins or a row per bin,
//    word 0 giving the taps as they are and a word giving stream_mix_taps' values;
//  - the size rules with their messages.
//
// `sub_plan_check query` answers one request per line of standard input: `call c F R` -> count n0 a0 (or `refused`), `tiles B
// count` -> runs items tiles, `item B item` -> first output, bin, `config B T rows R max have_taps` -> ok or the message, `table
// B T rows` -> the table of the taps 1000 r + k + 1 with all words 0, one tap per line.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "if_fir_sub_plan.h"

typedef unsigned __int128 u128;

static int fail(const char *what, unsigned long long a, unsigned long long b, unsigned long long c, unsigned long long d)
{
    printf("FAILED: %s at %llu %llu %llu %llu\n", what, a, b, c, d);
    return 1;
}

static int query()
{
    using namespace if_fir;
    char line[256], word[16];
    while (fgets(line, sizeof line, stdin))
    {
        unsigned long long c = 0, F = 0, mx = 0;
        unsigned B = 0, T = 0, rows = 0, R = 0, have = 0;
        if (sscanf(line, "%15s", word) != 1)
            continue;
        if (!strcmp(word, "call") && sscanf(line, "%*s %llu %llu %u", &c, &F, &R) == 3 && R >= 1)
        {
            SubCall call;
            if (!sub_call(c, F, R, &call))
                printf("refused\n");
            else
                printf("%llu %u %u\n", (unsigned long long)call.count, call.n0, call.a0);
        }
        else if (!strcmp(word, "tiles") && sscanf(line, "%*s %u %llu", &B, &c) == 2)
        {
            const SubTiles t = sub_tiles(B, c);
            printf("%llu %llu %llu\n", (unsigned long long)t.runs, (unsigned long long)t.items, (unsigned long long)t.tiles);
        }
        else if (!strcmp(word, "item") && sscanf(line, "%*s %u %llu", &B, &c) == 2 && B >= 1)
        {
            uint64_t o0;
            uint32_t j;
            sub_item_place(c, B, &o0, &j);
            printf("%llu %u\n", (unsigned long long)o0, j);
        }
        else if (!strcmp(word, "config") && sscanf(line, "%*s %u %u %u %u %llu %u", &B, &T, &rows, &R, &mx, &have) == 6)
        {
            char msg[256];
            printf("%s\n", sub_config_ok(B, T, rows, R, mx, have != 0, msg) ? "ok" : msg);
        }
        else if (!strcmp(word, "table") && sscanf(line, "%*s %u %u %u", &B, &T, &rows) == 3 && B >= 1 && T >= 1 && (rows == 1 || rows == B))
        {
            std::vector<float> h((size_t)rows * T), row(2 * (size_t)T), tab(2 * (size_t)T * B, -1.0f);
            std::vector<uint32_t> words(B, 0u);
            for (unsigned r = 0; r < rows; r++)
                for (unsigned k = 0; k < T; k++)
                    h[(size_t)r * T + k] = (float)(1000 * r + k + 1);
            sub_build_table(h.data(), T, rows, B, words.data(), row.data(), tab.data());
            for (size_t e = 0; e < (size_t)T * B; e++)
                printf("%g %g\n", tab[2 * e], tab[2 * e + 1]);
        }
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
    unsigned long long calls = 0, shapes = 0, tables = 0;
    // ---- the call plan
    for (unsigned R = 1; R <= SUB_MAX_DECIMATION; R++)
    {
        const unsigned long long uR = R;
        const unsigned long long cs[9] = {0, 1, uR - 1, uR, 4294967295ull, 4294967296ull, 4294967297ull, 1ull << 63, ~0ull - 1000};
        const unsigned long long Fs[9] = {0, 1, 2, uR - 1, uR, uR + 1, 701, 1000, 1ull << 32};
        for (unsigned long long c : cs)
            for (unsigned long long F : Fs)
            {
                calls++;
                SubCall call;
                const bool past = (u128)c + F > ~0ull;
                if (sub_call(c, F, R, &call) == past)
                    return fail(past ? "a position past 2^64 was accepted" : "sub_call refused", c, F, R, 0);
                if (past)
                    continue;
                const u128 first = ((u128)c + R - 1) / R, last = ((u128)c + F + R - 1) / R;
                if ((u128)call.count != last - first)
                    return fail("count", c, F, R, call.count);
                if (call.count && (call.n0 >= R || ((u128)c + call.n0) % R != 0 || (u128)call.n0 != first * R - c ||
                                   call.a0 != (uint32_t)(unsigned long long)((u128)c + call.n0) || call.n0 + (call.count - 1) * uR >= F))
                    return fail("n0 or a0", c, F, R, call.n0);
            }
    }
    SubCall refused;
    if (sub_call(~0ull - 5, 10, 3, &refused) || sub_call(~0ull, 1, 1, &refused) || !sub_call(~0ull - 1, 1, 1, &refused))
        return fail("the edge of 2^64", 0, 0, 0, 0);
    // ---- the tile plan and the kernel's index algebra
    const unsigned Bs[6] = {1, 63, 64, 65, 4095, 4096};
    for (unsigned B : Bs)
    {
        const unsigned long long per_tile = (unsigned long long)SUB_THREADS * SUB_OUT; // (output, bin) values of a tile
        const unsigned long long edge = (per_tile + B - 1) / B;                         // outputs that fill about one tile
        const unsigned long long counts[14] = {0, 1, 2, 3, 4, 5, 7, 8, 9, edge > 1 ? edge - 1 : 1, edge, edge + 1, 4 * edge + 3, 1ull << 32};
        for (unsigned long long count : counts)
        {
            shapes++;
            const SubTiles t = sub_tiles(B, count);
            if ((u128)t.runs * SUB_OUT < count || (t.runs && (u128)(t.runs - 1) * SUB_OUT >= count) || (u128)t.items != (u128)t.runs * B ||
                (u128)t.tiles * SUB_THREADS < t.items || (t.tiles && (u128)(t.tiles - 1) * SUB_THREADS >= t.items) || (!count && (t.runs || t.tiles)))
                return fail("tiles", B, count, t.items, t.tiles);
            if ((u128)t.items * SUB_OUT >= ((u128)1 << 62))
                return fail("an item count beyond 62 bits", B, count, t.items, 0);
            // every (output, bin) at the edges belongs to the item run B + j and to no other
            const unsigned long long os[6] = {0, 1, count / 2, count > 2 ? count - 2 : 0, count ? count - 1 : 0, 3};
            const unsigned js[4] = {0, B / 2, B > 1 ? B - 2 : 0, B - 1};
            for (unsigned long long o : os)
                for (unsigned j : js)
                {
                    if (o >= count)
                        continue;
                    const unsigned long long item = (o / SUB_OUT) * B + j;
                    uint64_t o0;
                    uint32_t jj;
                    sub_item_place(item, B, &o0, &jj);
                    if (item >= t.items || jj != j || o0 > o || o >= o0 + SUB_OUT || o0 % SUB_OUT)
                        return fail("item", B, count, o, j);
                }
            // the items at both ends of the first, a middle and the last tile: consecutive items, the bin fastest
            const unsigned long long tiles[3] = {0, t.tiles / 2, t.tiles ? t.tiles - 1 : 0};
            for (unsigned long long tile : tiles)
            {
                if (!t.tiles)
                    break;
                unsigned long long prev_o = 0;
                unsigned prev_j = 0;
                for (int lane = 0; lane < SUB_THREADS; lane++)
                {
                    const unsigned long long item = tile * SUB_THREADS + lane;
                    if (item >= t.items)
                    {
                        if (tile != t.tiles - 1)
                            return fail("an idle lane before the last tile", B, count, tile, lane);
                        break;
                    }
                    uint64_t o0;
                    uint32_t j;
                    sub_item_place(item, B, &o0, &j);
                    if (j >= B || o0 >= t.runs * SUB_OUT)
                        return fail("a lane outside the plane", B, count, tile, lane);
                    if (lane && !((j == prev_j + 1 && o0 == prev_o) || (j == 0 && prev_j == B - 1 && o0 == prev_o + SUB_OUT)))
                        return fail("lanes not along the bins", B, count, tile, lane);
                    prev_o = o0;
                    prev_j = j;
                }
            }
            // the reads of the first and the last item, for a few (T, R, n0): inside [-(T-1) B, F B) wherever the tap counts,
            // and inside [0, F B) for an item the kernel takes for interior
            const unsigned Ts[4] = {1, 2, 17, SUB_MAX_TAPS}, Rs[4] = {1, 3, 7, SUB_MAX_DECIMATION};
            for (unsigned T : Ts)
                for (unsigned R : Rs)
                {
                    if (!count)
                        continue;
                    const unsigned n0 = R - 1;
                    const u128 F = (u128)n0 + (u128)(count - 1) * R + 1; // the shortest call with these outputs
                    const unsigned long long items[2] = {0, t.items - 1};
                    for (unsigned long long item : items)
                    {
                        uint64_t o0;
                        uint32_t j;
                        sub_item_place(item, B, &o0, &j);
                        const __int128 row0 = (__int128)n0 + (__int128)o0 * R;
                        const bool interior = row0 - (T - 1) >= 0 && row0 + (__int128)(SUB_OUT - 1) * R < (__int128)F;
                        for (int i = 0; i < SUB_OUT; i++)
                            for (unsigned k = 0; k < T; k += (T > 1 ? T - 1 : 1))
                            {
                                const __int128 e = (row0 + (__int128)i * R - k) * B + j;
                                if (e >= ((__int128)1 << 62) || e <= -((__int128)1 << 62))
                                    return fail("an offset beyond 62 bits", B, count, T, R);
                                if (interior && (e < 0 || e >= (__int128)F * B))
                                    return fail("an interior item reads outside the call", B, count, T, R);
                                if (o0 + i < count && e < -(__int128)(T - 1) * B)
                                    return fail("a read before the history", B, count, T, R);
                                if (o0 + i < count && row0 + (__int128)i * R >= (__int128)F)
                                    return fail("an output beyond the call", B, count, T, R);
                            }
                    }
                }
        }
    }
    // ---- the tap-major table
    const unsigned TBs[5][2] = {{1, 1}, {63, 16}, {65, 17}, {4096, 2}, {200, SUB_MAX_TAPS}};
    for (const auto &tb : TBs)
        for (unsigned rows_all = 0; rows_all < 2; rows_all++)
        {
            tables++;
            const unsigned B = tb[0], T = tb[1], rows = rows_all ? B : 1;
            std::vector<float> h((size_t)rows * T), row(2 * (size_t)T), mixed(2 * (size_t)T);
            std::vector<uint32_t> words(B);
            for (unsigned r = 0; r < rows; r++)
                for (unsigned k = 0; k < T; k++)
                    h[(size_t)r * T + k] = (float)(1000 * r + k + 1);
            for (unsigned j = 0; j < B; j++)
                words[j] = j % 3 == 0 ? 0u : 0x9e3779b9u * j;
            float *tab = (float *)malloc(2 * (size_t)T * B * sizeof(float)); // exactly its size: the sanitizer sees one float more
            if (!tab)
                return fail("out of memory", B, T, rows, 0);
            sub_build_table(h.data(), T, rows, B, words.data(), row.data(), tab);
            for (unsigned j = 0; j < B; j++)
            {
                const float *hr = h.data() + (rows == 1 ? 0 : (size_t)j * T);
                stream_mix_taps(hr, (int)T, 0, words[j], mixed.data());
                for (unsigned k = 0; k < T; k++)
                {
                    const size_t at = sub_table_place(k, j, B);
                    if (at != (size_t)k * B + j || at >= (size_t)T * B || tab[2 * at] != mixed[2 * k] || tab[2 * at + 1] != mixed[2 * k + 1] ||
                        (words[j] == 0 && (tab[2 * at] != hr[k] || tab[2 * at + 1] != 0.0f)))
                    {
                        free(tab);
                        return fail("tap table", B, T, j, k);
                    }
                }
            }
            free(tab);
        }
    // ---- the size rules
    char msg[256];
    const struct
    {
        unsigned B, T, rows, R;
        unsigned long long mx;
        bool have;
        const char *want;
    } rules[] = {
        {24, 33, 1, 2, 4096, true, nullptr},
        {24, 33, 24, 2, 1ull << 32, true, nullptr},
        {1, 1, 1, 1, 1, true, nullptr},
        {4096, 128, 4096, 64, 1, true, nullptr},
        {0, 33, 1, 2, 4096, true, "bins must be 1..4096 (got 0)"},
        {4097, 33, 1, 2, 4096, true, "bins must be 1..4096 (got 4097)"},
        {24, 0, 1, 2, 4096, true, "taps must be 1..128 (got 0)"},
        {24, 129, 1, 2, 4096, true, "taps must be 1..128 (got 129)"},
        {24, 33, 1, 2, 4096, false, "taps must be 1..128 (got 33), pfTaps is NULL"},
        {24, 33, 0, 2, 4096, true, "tap rows must be 1 or the 24 bins (got 0)"},
        {24, 33, 2, 2, 4096, true, "tap rows must be 1 or the 24 bins (got 2)"},
        {24, 33, 1, 0, 4096, true, "decimation must be 1..64 (got 0)"},
        {24, 33, 1, 65, 4096, true, "decimation must be 1..64 (got 65)"},
        {24, 33, 1, 2, 0, true, "ullMaxFrames must be 1..2^32 (got 0)"},
        {24, 33, 1, 2, (1ull << 32) + 1, true, "ullMaxFrames must be 1..2^32 (got 4294967297)"},
        {0, 0, 0, 0, 0, false, "bins must be 1..4096 (got 0)"},
    };
    for (const auto &r : rules)
    {
        const bool ok = sub_config_ok(r.B, r.T, r.rows, r.R, r.mx, r.have, msg);
        if (ok != (r.want == nullptr) || (!ok && strcmp(msg, r.want)))
            return fail(ok ? "a broken rule was accepted" : msg, r.B, r.T, r.rows, r.R);
    }
    printf("%llu calls, %llu tile plans, %llu tables checked: OK\n", calls, shapes, tables);
    return 0;
}
