// subup_plan_check.cpp — walks qo-100-tools_amd/csrc/if_fir_subup_plan.h, the planning the per-bin interpolating FIR stage's shim
// and kernel use, with a plain host compiler (tests/test_subup_host.py builds it with -fsanitize=address,undefined and runs it
// directly).
//
// Without arguments:
//  - the call plan for every R = 1 .. 64 at positions c in {0, 1, 2^32-1, 2^32, 2^32+1, 2^63 / R, E - 1001, E - 1, E} with
//    E = floor((2^64 - 1) / R) and F in {0, 1, 2, 31, 32, 33, 701, 1000, 2^32}: accepted exactly when (c + F) R <= 2^64 - 1 (128-bit
//    arithmetic here), count = F R, n0 = the low 32 bits of c R;
//  - the tile plan for B in {1, 63, 64, 65, 4095, 4096}, R in {1, 3, 64} and frame counts around every edge of a run and of a
//    tile: every (frame, phase, bin) of the call belongs to exactly one item, item = (run R + p) B + j, the items of a tile are
//    consecutive with the bin fastest, the tiles cover the items and only the last one is ragged; the index algebra of the
//    kernel: the element under frame m - i of bin j is (m - i) B + j, never before the (J - 1) B carried elements, an item the
//    kernel takes for interior reads and writes nothing outside the call, and the largest offsets (F R B reaches 2^50) fit 62
//    bits;
//  - the zero-padded tap-major table built into a heap buffer of exactly its size: h_r[k] at k rows + r, 0 from T to J R, and
//    every entry p + i R a lane reads inside it;
//  - the size rules with their messages.
//
// `subup_plan_check query` answers one request per line of standard input: `call c F R` -> count n0 (or `refused`), `tiles B R
// F` -> runs items tiles, `item B R item` -> first frame, phase, bin, `config B T rows R max have_taps` -> ok or the message,
// `table B T rows R` -> the table of the taps 1000 r + k + 1, one entry per line.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "if_fir_subup_plan.h"

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
            SubUpCall call;
            if (!subup_call(c, F, R, &call))
                printf("refused\n");
            else
                printf("%llu %u\n", (unsigned long long)call.count, call.n0);
        }
        else if (!strcmp(word, "tiles") && sscanf(line, "%*s %u %u %llu", &B, &R, &F) == 3)
        {
            const SubUpTiles t = subup_tiles(B, R, F);
            printf("%llu %llu %llu\n", (unsigned long long)t.runs, (unsigned long long)t.items, (unsigned long long)t.tiles);
        }
        else if (!strcmp(word, "item") && sscanf(line, "%*s %u %u %llu", &B, &R, &c) == 3 && B >= 1 && R >= 1)
        {
            uint64_t m0;
            uint32_t p, j;
            subup_item_place(c, B, R, &m0, &p, &j);
            printf("%llu %u %u\n", (unsigned long long)m0, p, j);
        }
        else if (!strcmp(word, "config") && sscanf(line, "%*s %u %u %u %u %llu %u", &B, &T, &rows, &R, &mx, &have) == 6)
        {
            char msg[256];
            printf("%s\n", subup_config_ok(B, T, rows, R, mx, have != 0, msg) ? "ok" : msg);
        }
        else if (!strcmp(word, "table") && sscanf(line, "%*s %u %u %u %u", &B, &T, &rows, &R) == 4 && B >= 1 && T >= 1 && R >= 1 &&
                 (rows == 1 || rows == B))
        {
            std::vector<float> h((size_t)rows * T), tab(subup_table_floats(T, rows, R), -1.0f);
            for (unsigned r = 0; r < rows; r++)
                for (unsigned k = 0; k < T; k++)
                    h[(size_t)r * T + k] = (float)(1000 * r + k + 1);
            subup_build_table(h.data(), T, rows, R, tab.data());
            for (size_t e = 0; e < tab.size(); e++)
                printf("%g\n", tab[e]);
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
    for (unsigned R = 1; R <= SUBUP_MAX_INTERPOLATION; R++)
    {
        const unsigned long long E = ~0ull / R; // the last position a stream has
        const unsigned long long cs[9] = {0, 1, 4294967295ull, 4294967296ull, 4294967297ull, (1ull << 63) / R, E - 1001, E - 1, E};
        const unsigned long long Fs[9] = {0, 1, 2, 31, 32, 33, 701, 1000, 1ull << 32};
        for (unsigned long long c : cs)
            for (unsigned long long F : Fs)
            {
                calls++;
                SubUpCall call;
                const bool past = ((u128)c + F) * R > (u128)~0ull;
                if (subup_call(c, F, R, &call) == past)
                    return fail(past ? "an output index past 2^64 - 1 was accepted" : "subup_call refused", c, F, R, 0);
                if (past)
                    continue;
                if ((u128)call.count != (u128)F * R || call.n0 != (uint32_t)(unsigned long long)(((u128)c * R) & 0xffffffffu))
                    return fail("count or n0", c, F, R, call.count);
            }
    }
    SubUpCall refused;
    if (subup_call(~0ull, 1, 1, &refused) || !subup_call(~0ull - 1, 1, 1, &refused) || subup_call(~0ull / 3, 1, 3, &refused) ||
        !subup_call(~0ull / 3 - 1, 1, 3, &refused) || subup_call(~0ull - 5, 10, 1, &refused))
        return fail("the edge of 2^64", 0, 0, 0, 0);
    // ---- the tile plan and the kernel's index algebra
    const unsigned Bs[6] = {1, 63, 64, 65, 4095, 4096}, Rs[3] = {1, 3, SUBUP_MAX_INTERPOLATION};
    for (unsigned B : Bs)
        for (unsigned R : Rs)
        {
            const unsigned long long per_tile = (unsigned long long)SUBUP_THREADS * SUBUP_Q; // (frame, phase, bin) values of a tile
            const unsigned long long edge = (per_tile + (unsigned long long)B * R - 1) / ((unsigned long long)B * R); // frames that fill about one tile
            const unsigned long long Fs[12] = {0, 1, 31, 32, 33, 64, 97, edge > 1 ? edge - 1 : 1, edge, edge + 1, 4 * edge + 3, 1ull << 32};
            for (unsigned long long F : Fs)
            {
                shapes++;
                const SubUpTiles t = subup_tiles(B, R, F);
                if ((u128)t.runs * SUBUP_Q < F || (t.runs && (u128)(t.runs - 1) * SUBUP_Q >= F) || (u128)t.items != (u128)t.runs * R * B ||
                    (u128)t.tiles * SUBUP_THREADS < t.items || (t.tiles && (u128)(t.tiles - 1) * SUBUP_THREADS >= t.items) ||
                    (!F && (t.runs || t.tiles)))
                    return fail("tiles", B, R, F, t.tiles);
                if ((u128)t.items * SUBUP_Q >= ((u128)1 << 62))
                    return fail("an item count beyond 62 bits", B, R, F, t.items);
                // every (frame, phase, bin) at the edges belongs to the item (run R + p) B + j and to no other
                const unsigned long long ms[6] = {0, 1, F / 2, F > 2 ? F - 2 : 0, F ? F - 1 : 0, 33};
                const unsigned ps[3] = {0, R / 2, R - 1}, js[4] = {0, B / 2, B > 1 ? B - 2 : 0, B - 1};
                for (unsigned long long m : ms)
                    for (unsigned p : ps)
                        for (unsigned j : js)
                        {
                            if (m >= F)
                                continue;
                            const unsigned long long item = ((m / SUBUP_Q) * R + p) * B + j;
                            uint64_t m0;
                            uint32_t pp, jj;
                            subup_item_place(item, B, R, &m0, &pp, &jj);
                            if (item >= t.items || jj != j || pp != p || m0 > m || m >= m0 + SUBUP_Q || m0 % SUBUP_Q)
                                return fail("item", B, R, m, j);
                        }
                // the items at both ends of the first, a middle and the last tile: consecutive items, the bin fastest, then the
                // phase: a wave's stores of one step are consecutive elements of the output
                const unsigned long long tiles[3] = {0, t.tiles / 2, t.tiles ? t.tiles - 1 : 0};
                for (unsigned long long tile : tiles)
                {
                    if (!t.tiles)
                        break;
                    u128 prev_out = 0;
                    uint64_t prev_m0 = 0;
                    for (int lane = 0; lane < SUBUP_THREADS; lane++)
                    {
                        const unsigned long long item = tile * SUBUP_THREADS + lane;
                        if (item >= t.items)
                        {
                            if (tile != t.tiles - 1)
                                return fail("an idle lane before the last tile", B, R, tile, lane);
                            break;
                        }
                        uint64_t m0;
                        uint32_t p, j;
                        subup_item_place(item, B, R, &m0, &p, &j);
                        if (j >= B || p >= R || m0 >= t.runs * SUBUP_Q)
                            return fail("a lane outside the space", B, R, tile, lane);
                        const u128 out = ((u128)m0 * R + p) * B + j; // the element of the lane's first output
                        if (lane && !((m0 == prev_m0 && out == prev_out + 1) || (m0 == prev_m0 + SUBUP_Q && p == 0 && j == 0)))
                            return fail("lanes not along the output", B, R, tile, lane);
                        prev_out = out;
                        prev_m0 = m0;
                    }
                }
                // the reads and writes of the first and the last item, for a few J: reads inside [-(J-1) B, F B) wherever a
                // frame of the call is under way, and inside [0, F B) with every write inside [0, F R B) for an item the kernel
                // takes for interior
                const unsigned Js[4] = {1, 2, 6, SUBUP_MAX_J};
                for (unsigned J : Js)
                {
                    if (!F)
                        continue;
                    const unsigned long long items[2] = {0, t.items - 1};
                    for (unsigned long long item : items)
                    {
                        uint64_t m0;
                        uint32_t p, j;
                        subup_item_place(item, B, R, &m0, &p, &j);
                        const bool interior = (__int128)m0 - (J - 1) >= 0 && (u128)m0 + SUBUP_Q <= F;
                        for (int s = 0; s < SUBUP_Q; s += SUBUP_Q - 1)
                            for (unsigned i = 0; i < J; i += (J > 1 ? J - 1 : 1))
                            {
                                const __int128 m = (__int128)m0 + s;
                                const __int128 e = (m - i) * B + j, o = (m * R + p) * B + j;
                                if (e >= ((__int128)1 << 62) || e <= -((__int128)1 << 62) || o >= ((__int128)1 << 62))
                                    return fail("an offset beyond 62 bits", B, R, F, J);
                                if (interior && (e < 0 || e >= (__int128)F * B || o < 0 || o >= (__int128)F * R * B))
                                    return fail("an interior item reads or writes outside the call", B, R, F, J);
                                if (m < (__int128)F && e < -(__int128)(J - 1) * B)
                                    return fail("a read before the history", B, R, F, J);
                                if (m < (__int128)F && o >= (__int128)F * R * B)
                                    return fail("an output beyond the call", B, R, F, J);
                            }
                    }
                }
            }
        }
    if (subup_tiles(4096, 64, 1ull << 32).runs * SUBUP_Q * 64 * 4096 != 1ull << 50)
        return fail("the largest call", 0, 0, 0, 0);
    // ---- the zero-padded tap-major table
    const unsigned TBs[6][3] = {{1, 1, 1}, {63, 16, 2}, {65, 17, 3}, {64, 33, 64}, {4096, 2, 1}, {3, SUBUP_MAX_TAPS, 64}};
    for (const auto &tb : TBs)
        for (unsigned rows_all = 0; rows_all < 2; rows_all++)
        {
            tables++;
            const unsigned B = tb[0], T = tb[1], R = tb[2], rows = rows_all ? B : 1, J = subup_j(T, R);
            std::vector<float> h((size_t)rows * T);
            for (unsigned r = 0; r < rows; r++)
                for (unsigned k = 0; k < T; k++)
                    h[(size_t)r * T + k] = (float)(1000 * r + k + 1);
            const size_t n = subup_table_floats(T, rows, R);
            float *tab = (float *)malloc(n * sizeof(float)); // exactly its size: the sanitizer sees one float more
            if (!tab)
                return fail("out of memory", B, T, rows, 0);
            subup_build_table(h.data(), T, rows, R, tab);
            bool ok = n == (size_t)J * R * rows && J >= 1 && (size_t)J * R >= T && (size_t)(J - 1) * R < T && subup_bucket(J) >= (int)J &&
                      subup_bucket(J) < 2 * (int)J && (subup_bucket(J) & (subup_bucket(J) - 1)) == 0;
            for (unsigned r = 0; ok && r < rows; r++)
                for (unsigned p = 0; ok && p < R; p++)
                    for (unsigned i = 0; ok && i < J; i++)
                    {
                        const unsigned k = p + i * R;
                        const size_t at = subup_table_place(k, r, rows);
                        ok = at == (size_t)k * rows + r && at < n && tab[at] == (k < T ? h[(size_t)r * T + k] : 0.0f);
                    }
            free(tab);
            if (!ok)
                return fail("tap table", B, T, R, rows);
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
        {4096, 2048, 4096, 64, 1, true, nullptr},
        {24, 32, 1, 1, 4096, true, nullptr},
        {0, 33, 1, 2, 4096, true, "bins must be 1..4096 (got 0)"},
        {4097, 33, 1, 2, 4096, true, "bins must be 1..4096 (got 4097)"},
        {24, 0, 1, 2, 4096, true, "taps must be 1..2048 (got 0)"},
        {24, 2049, 1, 64, 4096, true, "taps must be 1..2048 (got 2049)"},
        {24, 33, 1, 2, 4096, false, "taps must be 1..2048 (got 33), pfTaps is NULL"},
        {24, 33, 0, 2, 4096, true, "tap rows must be 1 or the 24 bins (got 0)"},
        {24, 33, 2, 2, 4096, true, "tap rows must be 1 or the 24 bins (got 2)"},
        {24, 33, 1, 0, 4096, true, "interpolation must be 1..64 (got 0)"},
        {24, 33, 1, 65, 4096, true, "interpolation must be 1..64 (got 65)"},
        {24, 33, 1, 1, 4096, true, "taps per phase J = ceil(33 / 1) = 33 exceed 32"},
        {24, 2048, 1, 63, 4096, true, "taps per phase J = ceil(2048 / 63) = 33 exceed 32"},
        {24, 33, 1, 2, 0, true, "ullMaxFrames must be 1..2^32 (got 0)"},
        {24, 33, 1, 2, (1ull << 32) + 1, true, "ullMaxFrames must be 1..2^32 (got 4294967297)"},
        {0, 0, 0, 0, 0, false, "bins must be 1..4096 (got 0)"},
    };
    for (const auto &r : rules)
    {
        const bool ok = subup_config_ok(r.B, r.T, r.rows, r.R, r.mx, r.have, msg);
        if (ok != (r.want == nullptr) || (!ok && strcmp(msg, r.want)))
            return fail(ok ? "a broken rule was accepted" : msg, r.B, r.T, r.rows, r.R);
    }
    printf("%llu calls, %llu tile plans, %llu tables checked: OK\n", calls, shapes, tables);
    return 0;
}
