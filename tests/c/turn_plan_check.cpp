// turn_plan_check.cpp — the corner turn's plan header (qo-100-tools_amd/csrc/if_fir_turn_plan.h) played on the host.  Stand-alone:
// built with plain g++ under the address and undefined-behaviour sanitizers and run directly (tests/test_turn_host.py).
//
// Without arguments it walks the tile map exactly as turn_kernel does -- the grid-stride loop over the tiles on 1 and on 3
// workgroups, both phases of a tile, 256 threads of 16 items -- over frame counts, channel counts, frame sizes and four
// selections, with an LDS tile of exactly the planned size, and checks that
//   TO_STREAMS writes every (c, a), a < F, exactly once, nothing at a >= F, and the element SPEC §20 names;
//   TO_FRAMES writes every one of the F B elements exactly once, the listed ones from their rows, the others zero;
//   no LDS index leaves the tile and a phase reads only what the other phase wrote;
//   the offsets of the first and the last tile at P = 2^32 and F = 2^32 (and at the largest legal pitch) equal 128-bit arithmetic;
//   the init and call rules give their messages in order.
// "query" answers request lines from stdin: config / call / tile.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "if_fir_turn_plan.h"

using namespace if_fir;
typedef unsigned __int128 u128;

static long g_fail = 0;
#define CHECK(cond, ...)                   \
    do                                     \
    {                                      \
        if (!(cond))                       \
        {                                  \
            if (g_fail++ < 20)             \
            {                              \
                printf("FAIL %s: ", #cond); \
                printf(__VA_ARGS__);       \
                printf("\n");              \
            }                              \
        }                                  \
    } while (0)

static const uint32_t EMPTY = 0xffffffffu;

// the four selections (tests/turn_ref.py builds the same kinds for the GPU tests; the two need not agree element for element)
static std::vector<uint32_t> selection(int kind, uint32_t B, uint32_t C)
{
    std::vector<uint32_t> s;
    const uint32_t first = B - C < 3 ? B - C : 3;
    if (kind == 0)
        for (uint32_t c = 0; c < C; c++)
            s.push_back(first + c);
    else if (kind == 1)
        for (uint32_t c = 0; c < C; c++)
            s.push_back(first + C - 1 - c);
    else if (kind == 2)
    {
        // scattered: a fixed permutation of the frame's bins by a linear congruential walk, its first C
        std::vector<uint32_t> perm(B);
        for (uint32_t i = 0; i < B; i++)
            perm[i] = i;
        uint64_t x = 88172645463325252ull + B * 977u + C;
        for (uint32_t i = B; i > 1; i--)
        {
            x = x * 6364136223846793005ull + 1442695040888963407ull;
            const uint32_t k = (uint32_t)((x >> 33) % i);
            const uint32_t t = perm[i - 1];
            perm[i - 1] = perm[k];
            perm[k] = t;
        }
        s.assign(perm.begin(), perm.begin() + C);
    }
    else
    {
        // straddle: the bins on either side of every multiple of 64 (the frame side's tile edges), filled up from the top,
        // rotated by one so that a pair also lies across the channel side's tile edges
        std::vector<uint8_t> taken(B, 0);
        std::vector<uint32_t> pool;
        for (uint32_t e = 64; e < B; e += 64)
        {
            pool.push_back(e - 1);
            pool.push_back(e);
            taken[e - 1] = taken[e] = 1;
        }
        for (uint32_t b = B; b-- > 0;)
            if (!taken[b])
                pool.push_back(b);
        pool.resize(C);
        s.push_back(pool[C - 1]);
        s.insert(s.end(), pool.begin(), pool.end() - 1);
    }
    return s;
}

// one launch played: `groups` workgroups, each its tiles in order.  Elements are numbered: the input element at offset e holds
// the value e + 1; 0 is the zero a TO_FRAMES call writes; EMPTY marks what nobody wrote.
struct Play
{
    uint32_t B, C;
    uint64_t F, P;
    std::vector<uint16_t> sel, inv;
    std::vector<uint32_t> out;     // the output's values, by offset
    std::vector<uint8_t> count;    // writes per output offset
    long tiles_walked = 0;
};

static void play(Play &p, int direction, int groups)
{
    const uint32_t cols = direction == (int)TURN_TO_STREAMS ? p.C : p.B;
    const int xs = turn_tile_shift(cols);
    const int lds_n = turn_lds_elements(xs);
    int64_t tiles_x;
    const int64_t tiles = turn_tiles(cols, p.F, xs, &tiles_x);
    CHECK(turn_tile_frames(xs) >= 64 && (1 << xs) <= TURN_MAX_COLS && ((1u << xs) >= cols || (1 << xs) == TURN_MAX_COLS), "xs %d cols %u", xs, cols);
    CHECK((turn_lds_pitch(xs) & 1) == 1 && lds_n <= 6144, "pitch %d elements %d", turn_lds_pitch(xs), lds_n);
    for (int g = 0; g < groups; g++)
    {
        // exactly the planned size: the sanitizer sees an index past it
        std::vector<uint32_t> lds((size_t)lds_n);
        for (int64_t t = g; t < tiles; t += groups)
        {
            p.tiles_walked++;
            uint32_t x0;
            uint64_t a0;
            turn_tile_origin(t, tiles_x, xs, &x0, &a0);
            CHECK(x0 < cols && a0 < p.F, "tile %lld origin (%u, %llu)", (long long)t, x0, (unsigned long long)a0);
            std::fill(lds.begin(), lds.end(), EMPTY);
            int j, f;
            if (direction == (int)TURN_TO_STREAMS)
            {
                for (int tid = 0; tid < TURN_THREADS; tid++)
                    for (int k = 0; k < TURN_ITEMS; k++)
                    {
                        turn_item_along_frame(k, tid, xs, &j, &f);
                        const uint32_t c = x0 + (uint32_t)j;
                        const uint64_t a = a0 + (uint64_t)f;
                        uint32_t v = 0;
                        if (c < p.C && a < p.F)
                            v = (uint32_t)turn_frame_offset(a, p.B, p.sel[c]) + 1;
                        uint32_t &slot = lds.at((size_t)turn_lds_index(j, f, xs));
                        CHECK(slot == EMPTY, "LDS slot written twice");
                        slot = v;
                    }
                for (int tid = 0; tid < TURN_THREADS; tid++)
                    for (int k = 0; k < TURN_ITEMS; k++)
                    {
                        int jw, fw;
                        turn_item_along_row(k, tid & ~63, xs, &jw, &fw);
                        turn_item_along_row(k, tid, xs, &j, &f);
                        CHECK(j == jw && f == fw + (tid & 63), "a wave of the row phase is not 64 consecutive frames of one column");
                        const uint32_t v = lds.at((size_t)turn_lds_index(j, f, xs));
                        CHECK(v != EMPTY, "LDS slot read that nobody wrote");
                        const uint32_t c = x0 + (uint32_t)j;
                        const uint64_t a = a0 + (uint64_t)f;
                        if (c < p.C && a < p.F)
                        {
                            const uint64_t o = turn_row_offset(c, p.P, a);
                            p.out.at((size_t)o) = v;
                            p.count.at((size_t)o)++;
                        }
                    }
            }
            else
            {
                bool any = false;
                for (int tid = 0; tid < TURN_THREADS; tid++)
                {
                    turn_item_along_frame(0, tid, xs, &j, &f);
                    const uint32_t bin = x0 + (uint32_t)j;
                    any = any || (bin < p.B && p.inv[bin] != TURN_NONE);
                }
                if (any)
                    for (int tid = 0; tid < TURN_THREADS; tid++)
                        for (int k = 0; k < TURN_ITEMS; k++)
                        {
                            turn_item_along_row(k, tid, xs, &j, &f);
                            const uint32_t i = x0 + (uint32_t)j;
                            const uint32_t cr = i < p.B ? p.inv[i] : (uint32_t)TURN_NONE;
                            const uint64_t a = a0 + (uint64_t)f;
                            uint32_t v = 0;
                            if (cr != (uint32_t)TURN_NONE && a < p.F)
                                v = (uint32_t)turn_row_offset(cr, p.P, a) + 1;
                            uint32_t &slot = lds.at((size_t)turn_lds_index(j, f, xs));
                            CHECK(slot == EMPTY, "LDS slot written twice");
                            slot = v;
                        }
                for (int tid = 0; tid < TURN_THREADS; tid++)
                {
                    turn_item_along_frame(0, tid, xs, &j, &f);
                    const int j0 = j;
                    for (int k = 0; k < TURN_ITEMS; k++)
                    {
                        turn_item_along_frame(k, tid, xs, &j, &f);
                        CHECK(j == j0, "a thread's column moves with k");
                        uint32_t v = 0;
                        if (any)
                        {
                            v = lds.at((size_t)turn_lds_index(j, f, xs));
                            CHECK(v != EMPTY, "LDS slot read that nobody wrote");
                        }
                        const uint32_t bin = x0 + (uint32_t)j;
                        const uint64_t a = a0 + (uint64_t)f;
                        if (bin < p.B && a < p.F)
                        {
                            const uint64_t o = turn_frame_offset(a, p.B, bin);
                            p.out.at((size_t)o) = v;
                            p.count.at((size_t)o)++;
                        }
                    }
                }
            }
        }
    }
}

static long g_cases = 0, g_tiles = 0;

static void walk_case(uint32_t B, uint32_t C, uint64_t F, int kind, int groups)
{
    const std::vector<uint32_t> list = selection(kind, B, C);
    char msg[256];
    // the span kind goes in as a span (no list), the others as lists
    const uint32_t first = kind == 0 ? list[0] : 0;
    if (!turn_config_ok(TURN_TO_STREAMS, B, C, first, 0, 0, kind == 0 ? nullptr : list.data(), 4096, msg))
    {
        CHECK(false, "selection %d B %u C %u refused: %s", kind, B, C, msg);
        return;
    }
    Play p;
    p.B = B;
    p.C = C;
    p.F = F;
    p.P = F + (F % 3 == 0 ? 0 : 5); // a pitch with a tail on two frame counts of three
    p.sel.resize(C);
    p.inv.resize(B);
    turn_maps(B, C, first, kind == 0 ? nullptr : list.data(), p.sel.data(), p.inv.data());
    for (uint32_t c = 0; c < C; c++)
        CHECK(p.sel[c] == list[c] && p.inv[list[c]] == c, "maps at channel %u", c);
    // TO_STREAMS
    p.out.assign((size_t)(C * p.P), EMPTY);
    p.count.assign((size_t)(C * p.P), 0);
    play(p, TURN_TO_STREAMS, groups);
    for (uint32_t c = 0; c < C; c++)
        for (uint64_t a = 0; a < p.P; a++)
        {
            const size_t o = (size_t)(c * p.P + a);
            if (a < F)
                CHECK(p.count[o] == 1 && p.out[o] == (uint32_t)(a * B + list[c]) + 1, "TO_STREAMS (%u, %llu): %u writes, value %u", c, (unsigned long long)a, p.count[o], p.out[o]);
            else
                CHECK(p.count[o] == 0, "TO_STREAMS wrote a row's tail at (%u, %llu)", c, (unsigned long long)a);
        }
    // TO_FRAMES
    p.out.assign((size_t)(F * B), EMPTY);
    p.count.assign((size_t)(F * B), 0);
    play(p, TURN_TO_FRAMES, groups);
    for (uint64_t a = 0; a < F; a++)
        for (uint32_t i = 0; i < B; i++)
        {
            const size_t o = (size_t)(a * B + i);
            const uint32_t want = p.inv[i] == TURN_NONE ? 0u : (uint32_t)(p.inv[i] * p.P + a) + 1;
            CHECK(p.count[o] == 1 && p.out[o] == want, "TO_FRAMES (%llu, %u): %u writes, value %u, wanted %u", (unsigned long long)a, i, p.count[o], p.out[o], want);
        }
    g_cases++;
    g_tiles += p.tiles_walked;
}

// the offsets of every item of the first and the last tile at the largest sizes against 128-bit arithmetic
static long check_offsets()
{
    long n = 0;
    const uint64_t Fs[] = {(uint64_t)1 << 32, ((uint64_t)1 << 32) - 1, ((uint64_t)1 << 31) + 7};
    const uint64_t Ps[] = {(uint64_t)1 << 32, ((uint64_t)1 << 32) + 1, TURN_MAX_PITCH};
    const uint32_t Bs[] = {8192, 4097, 65, 1};
    for (uint64_t F : Fs)
        for (uint64_t P : Ps)
            for (uint32_t B : Bs)
                for (int direction = 0; direction < 2; direction++)
                {
                    const uint32_t C = B;
                    const uint32_t cols = direction == (int)TURN_TO_STREAMS ? C : B;
                    const int xs = turn_tile_shift(cols);
                    int64_t tiles_x;
                    const int64_t tiles = turn_tiles(cols, F, xs, &tiles_x);
                    const u128 want_tiles = (u128)((cols + (1u << xs) - 1) >> xs) * (((u128)F + (u128)turn_tile_frames(xs) - 1) / (u128)turn_tile_frames(xs));
                    CHECK((u128)tiles == want_tiles && tiles > 0, "tiles of F %llu cols %u", (unsigned long long)F, cols);
                    uint64_t covered_hi = 0;
                    for (int64_t t : {(int64_t)0, tiles_x - 1, tiles - tiles_x, tiles - 1})
                    {
                        uint32_t x0;
                        uint64_t a0;
                        turn_tile_origin(t, tiles_x, xs, &x0, &a0);
                        CHECK((u128)a0 == (u128)(t / tiles_x) * (u128)turn_tile_frames(xs) && x0 == (uint32_t)(t % tiles_x) << xs, "origin of tile %lld", (long long)t);
                        for (int tid = 0; tid < TURN_THREADS; tid++)
                            for (int k = 0; k < TURN_ITEMS; k++)
                            {
                                int j, f;
                                turn_item_along_row(k, tid, xs, &j, &f);
                                const uint32_t x = x0 + (uint32_t)j;
                                const uint64_t a = a0 + (uint64_t)f;
                                if (x >= cols || a >= F)
                                    continue;
                                if (a > covered_hi)
                                    covered_hi = a;
                                const u128 row = (u128)x * (u128)P + (u128)a, frame = (u128)a * (u128)B + (u128)x;
                                CHECK((u128)turn_row_offset(x, P, a) == row && (row * 8) >> 63 == 0, "row offset (%u, %llu) at P %llu", x, (unsigned long long)a, (unsigned long long)P);
                                CHECK((u128)turn_frame_offset(a, B, x) == frame && (frame * 8) >> 63 == 0, "frame offset (%llu, %u)", (unsigned long long)a, x);
                                n++;
                            }
                    }
                    CHECK(covered_hi == F - 1, "the last tile ends at frame %llu of %llu", (unsigned long long)covered_hi, (unsigned long long)F);
                }
    return n;
}

static long g_rules = 0;
static void rule(uint32_t d, uint32_t B, uint32_t C, uint32_t first, uint32_t fi, uint32_t fo, const std::vector<uint32_t> *sel, uint64_t mf, const char *want)
{
    char msg[256] = "";
    const bool ok = turn_config_ok(d, B, C, first, fi, fo, sel ? sel->data() : nullptr, mf, msg);
    if (!want)
        CHECK(ok, "refused: %s", msg);
    else
        CHECK(!ok && !strcmp(msg, want), "got \"%s\", wanted \"%s\"", ok ? "ok" : msg, want);
    g_rules++;
}

static void check_rules()
{
    const std::vector<uint32_t> good = {5, 0, 7}, twice = {5, 0, 5}, outside = {5, 8, 9}, both = {9, 9, 9};
    rule(0, 8, 3, 2, 0, 0, nullptr, 4096, nullptr);
    rule(1, 8, 3, 0, 1, 1, &good, (uint64_t)1 << 32, nullptr);
    rule(0, 8192, 8192, 0, 0, 1, nullptr, 1, nullptr);
    // the table's order, then the list, then ullMaxFrames: each case breaks its rule and every later one
    rule(2, 0, 0, 9, 2, 2, &both, 0, "unknown direction 2");
    rule(1, 0, 0, 9, 2, 2, &both, 0, "bins must be 1..8192 (got 0)");
    rule(1, 8193, 0, 9, 2, 2, &both, 0, "bins must be 1..8192 (got 8193)");
    rule(1, 8, 0, 9, 2, 2, &both, 0, "channels must be 1..8, the frame's bins (got 0)");
    rule(1, 8, 9, 9, 2, 2, &both, 0, "channels must be 1..8, the frame's bins (got 9)");
    rule(1, 8, 3, 6, 2, 2, &both, 0, "bins [6, 9) of the span are outside the frame's 8");
    rule(1, 8, 3, 4294967295u, 2, 2, &both, 0, "bins [4294967295, 4294967298) of the span are outside the frame's 8");
    rule(1, 8, 3, 5, 2, 2, &both, 0, "unknown input format 2");
    rule(1, 8, 3, 5, 1, 2, &both, 0, "unknown output format 2");
    rule(1, 8, 3, 5, 1, 1, &both, 0, "ulFirst must be 0 beside a list of bins (got 5)");
    rule(1, 8, 3, 0, 1, 1, &both, 0, "bin 9 at place 0 of the list is outside the frame's 8");
    rule(1, 8, 3, 0, 1, 1, &outside, 0, "bin 8 at place 1 of the list is outside the frame's 8");
    rule(1, 8, 3, 0, 1, 1, &twice, 0, "bin 5 is listed twice (places 0 and 2)");
    rule(1, 8, 3, 0, 1, 1, &good, 0, "ullMaxFrames must be 1..2^32 (got 0)");
    rule(0, 8, 3, 5, 0, 0, nullptr, ((uint64_t)1 << 32) + 1, "ullMaxFrames must be 1..2^32 (got 4294967297)");
    char msg[256];
    CHECK(turn_call_ok(0, 0, 1, msg) && turn_call_ok(7, 7, 7, msg) && turn_call_ok(7, TURN_MAX_PITCH, 7, msg), "legal calls refused: %s", msg);
    CHECK(!turn_call_ok(8, 7, 4, msg) && !strcmp(msg, "a row pitch of 7 elements is below the call's 8 frames"), "%s", msg);
    CHECK(!turn_call_ok(8, TURN_MAX_PITCH + 1, 4, msg) && !strcmp(msg, "a row pitch of 1099511627777 elements is above 2^40"), "%s", msg);
    CHECK(!turn_call_ok(8, 8, 7, msg) && !strcmp(msg, "8 frames exceed ullMaxFrames 7 of init"), "%s", msg);
    g_rules += 4;
}

static int query()
{
    char line[1 << 17];
    while (fgets(line, sizeof line, stdin))
    {
        char *s = line;
        char word[32];
        int used = 0;
        if (sscanf(s, "%31s%n", word, &used) != 1)
            continue;
        s += used;
        std::vector<unsigned long long> v;
        char *end;
        for (;;)
        {
            const unsigned long long x = strtoull(s, &end, 10);
            if (end == s)
                break;
            v.push_back(x);
            s = end;
        }
        char msg[256] = "";
        if (!strcmp(word, "config") && v.size() >= 8 && v.size() == 8 + (v[7] == (unsigned long long)-1 ? 0 : v[7]))
        {
            // config direction B C first in out max_frames n s0 .. s(n-1);  n = 18446744073709551615: no list
            std::vector<uint32_t> sel;
            for (size_t i = 8; i < v.size(); i++)
                sel.push_back((uint32_t)v[i]);
            sel.resize(sel.size() < v[2] && v[2] <= TURN_MAX_BINS ? (size_t)v[2] : sel.size(), 0); // (a short list reads as zeros, never past the end)
            const bool ok = turn_config_ok((uint32_t)v[0], (uint32_t)v[1], (uint32_t)v[2], (uint32_t)v[3], (uint32_t)v[4], (uint32_t)v[5],
                                           v[7] == (unsigned long long)-1 ? nullptr : sel.data(), v[6], msg);
            printf("%s\n", ok ? "ok" : msg);
        }
        else if (!strcmp(word, "call") && v.size() == 3)
            printf("%s\n", turn_call_ok(v[0], v[1], v[2], msg) ? "ok" : msg);
        else if (!strcmp(word, "tile") && v.size() == 2)
        {
            // tile cols F: columns and frames of a tile, LDS pitch and elements, tiles of the call
            const int xs = turn_tile_shift((uint32_t)v[0]);
            int64_t tiles_x;
            const int64_t tiles = turn_tiles((uint32_t)v[0], v[1], xs, &tiles_x);
            printf("%d %d %d %d %lld %lld\n", 1 << xs, turn_tile_frames(xs), turn_lds_pitch(xs), turn_lds_elements(xs), (long long)tiles_x, (long long)tiles);
        }
        else
        {
            printf("bad request\n");
            return 2;
        }
    }
    return 0;
}

int main(int argc, char **argv)
{
    if (argc > 1 && !strcmp(argv[1], "query"))
        return query();
    const uint64_t Fs[] = {0, 1, 2, 63, 64, 65, 127, 129, 1000};
    const uint32_t Cs[] = {1, 2, 3, 63, 64, 65, 200, 0 /* = B */};
    const uint32_t Bs[] = {1, 64, 65, 918, 4097, 8192};
    // Every F x C x B x selection x grid where the frames are small; a large F B is walked for one in eight of its
    // combinations, counted so that every value of every set is walked at every large frame size
    int combo = 0;
    bool seen_f[9] = {}, seen_c[8] = {};
    for (uint32_t B : Bs)
    {
        memset(seen_f, 0, sizeof seen_f);
        memset(seen_c, 0, sizeof seen_c);
        for (int fi = 0; fi < 9; fi++)
            for (int ci = 0; ci < 8; ci++)
                for (int kind = 0; kind < 4; kind++)
                    for (int groups : {1, 3})
                    {
                        const uint32_t C = Cs[ci] ? Cs[ci] : B;
                        if (C > B)
                            continue;
                        const bool small = Fs[fi] * B <= 70000;
                        combo++;
                        if (!small && (fi + ci + kind + (groups == 3)) % 8 != 0 && seen_f[fi] && seen_c[ci])
                            continue;
                        seen_f[fi] = seen_c[ci] = true;
                        walk_case(B, C, Fs[fi], kind, groups);
                    }
    }
    const long offsets = check_offsets();
    check_rules();
    if (g_fail)
    {
        printf("%ld checks failed\n", g_fail);
        return 1;
    }
    printf("%ld cases of %d, %ld tiles, %ld offsets, %ld rules checked: OK\n", g_cases, combo, g_tiles, offsets, g_rules);
    return 0;
}
