// fpow_plan_check.cpp — stand-alone checker of qo-100-tools_amd/csrc/if_fir_fpow_plan.h (docs/SPEC.md §19), the header the frame
// power stage's shim and kernel unit use.  Plain g++, its own main; tests/test_fpow_host.py builds it with
// -fsanitize=address,undefined and runs it.
//
// Without arguments, the self-check:
//   - for every K in 1..20 and K = 65535, at positions around 0, 2^32 and 2^64 - 1 and at every position of a frame, calls of
//     0, 1, 7, 8, 9, K - 1, K, K + 1, 3 K + 5 frames: fpow_plan, fpow_chunk_entry and fpow_frame_entry against a walk of the
//     definition frame by frame; every row a chunk reads lies inside the call; the chunks fit fpow_max_chunks;
//   - calls of 2^32 frames and positions up to 2^64 - 1 against 128-bit arithmetic, the refusal when c + F passes 2^64;
//   - every cut of a 3 K-frame stream into two and into three calls (K in 1..20; K = 65535: the cuts around every chunk and
//     frame edge of the first frame and a half): the two kernels' arithmetic, played here in float32 through the same plan
//     functions with a workspace of exactly plan.chunks values on the heap, gives the bits of the definition summed in one go;
//   - workspace sizing: the most chunks any position gives never passes fpow_max_chunks, which never decreases in F;
//   - the init rules, each with its message.
// With `query`, it answers request lines on stdin ("plan c F K", "config ...", "work F K").
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "if_fir_fpow_plan.h"

using namespace if_fir;

static unsigned long long g_calls = 0, g_cuts = 0, g_rules = 0;

#define CHECK(cond, ...)                     \
    do                                       \
    {                                        \
        if (!(cond))                         \
        {                                    \
            std::printf("FAIL %s: ", #cond); \
            std::printf(__VA_ARGS__);        \
            std::printf("\n");               \
            std::exit(1);                    \
        }                                    \
    } while (0)

struct WalkChunk
{
    uint64_t row0;   // first row of the call in it
    uint32_t count;  // rows of the call in it
    bool from_partial, finished;
    uint64_t frame;  // output frame counted from the open one
};

// the definition, frame by frame: frame a belongs to output frame a / K, chunk (a mod K) / 8 of it
static void walk(uint64_t c, uint64_t F, uint32_t K, std::vector<WalkChunk> *chunks, uint64_t *frames)
{
    chunks->clear();
    *frames = 0;
    const uint64_t f0 = c / K;
    for (uint64_t i = 0; i < F; i++)
    {
        const uint64_t a = c + i, r = a % K;
        const bool first_of_chunk = r % FPOW_CHUNK == 0;
        if (i == 0 || first_of_chunk)
            chunks->push_back(WalkChunk{i, 0, !first_of_chunk, false, a / K - f0});
        chunks->back().count++;
        if (r % FPOW_CHUNK == FPOW_CHUNK - 1 || r == K - 1)
            chunks->back().finished = true;
        if (r == K - 1)
            ++*frames;
    }
}

static void one_call(uint64_t c, uint64_t F, uint32_t K)
{
    FpowPlan p;
    CHECK(fpow_plan(c, F, K, &p), "plan refused c=%" PRIu64 " F=%" PRIu64, c, F);
    std::vector<WalkChunk> w;
    uint64_t frames;
    walk(c, F, K, &w, &frames);
    uint64_t done = 0;
    for (const WalkChunk &ch : w)
        done += ch.finished;
    const uint32_t r = (uint32_t)(c % K), re = (uint32_t)((c % K + F % K) % K);
    CHECK(p.chunks == w.size() && p.done == done && p.frames == frames, "K=%u c=%" PRIu64 " F=%" PRIu64 ": plan (%" PRIu64 " %" PRIu64 " %" PRIu64
          ") walk (%zu %" PRIu64 " %" PRIu64 ")", K, c, F, p.chunks, p.done, p.frames, w.size(), done, frames);
    CHECK(p.chunk0 == r / FPOW_CHUNK && p.skip == r % FPOW_CHUNK && p.open_chunks == re / FPOW_CHUNK && p.open_frames == re % FPOW_CHUNK,
          "state K=%u c=%" PRIu64 " F=%" PRIu64, K, c, F);
    CHECK(p.touched == (F ? w.back().frame + 1 : 0), "touched");
    CHECK(p.chunks <= fpow_max_chunks(F, K), "K=%u F=%" PRIu64 ": %" PRIu64 " chunks, at most %" PRIu64, K, F, p.chunks, fpow_max_chunks(F, K));
    // finished chunks come first
    for (size_t q = 0; q < w.size(); q++)
    {
        CHECK(w[q].finished == (q < p.done), "chunk %zu finished out of order", q);
        uint64_t row0;
        uint32_t count;
        bool from_partial;
        fpow_chunk_entry(p.chunk0, p.skip, (uint32_t)q, K, F, &row0, &count, &from_partial);
        CHECK(row0 == w[q].row0 && count == w[q].count && from_partial == w[q].from_partial,
              "K=%u c=%" PRIu64 " F=%" PRIu64 " chunk %zu: entry (%" PRIu64 " %u %d) walk (%" PRIu64 " %u %d)", K, c, F, q, row0, count, from_partial,
              w[q].row0, w[q].count, w[q].from_partial);
        CHECK(count >= 1 && row0 + count <= F, "chunk %zu reads rows outside the call", q);
    }
    for (uint64_t t = 0; t < p.touched; t++)
    {
        uint64_t lo, hi;
        bool complete;
        fpow_frame_entry(p.chunk0, p.done, (uint32_t)t, K, &lo, &hi, &complete);
        uint64_t wlo = UINT64_MAX, whi = 0;
        for (size_t q = 0; q < w.size(); q++)
            if (w[q].frame == t && w[q].finished)
            {
                wlo = wlo == UINT64_MAX ? q : wlo;
                whi = q + 1;
            }
        if (wlo == UINT64_MAX)
            CHECK(lo == hi, "frame %" PRIu64 " has no finished chunk, entry [%" PRIu64 ", %" PRIu64 ")", t, lo, hi);
        else
            CHECK(lo == wlo && hi == whi, "frame %" PRIu64 ": entry [%" PRIu64 ", %" PRIu64 ") walk [%" PRIu64 ", %" PRIu64 ")", t, lo, hi, wlo, whi);
        CHECK(complete == (t < frames), "frame %" PRIu64 " complete", t);
        CHECK(hi <= p.done, "frame %" PRIu64 " reads unfinished chunks", t);
    }
    g_calls++;
}

// big counts and positions: 128-bit arithmetic
static void big_call(uint64_t c, uint64_t F, uint32_t K)
{
    FpowPlan p;
    const unsigned __int128 end = (unsigned __int128)c + F;
    const bool ok = fpow_plan(c, F, K, &p);
    if (end >> 64)
    {
        CHECK(!ok, "c + F past 2^64 was not refused");
        g_calls++;
        return;
    }
    CHECK(ok, "refused c=%" PRIu64 " F=%" PRIu64, c, F);
    const uint64_t cpf = (K + 7) / 8;
    const unsigned __int128 frames = end / K - c / K;
    // chunks begun before `end`, minus chunks finished before c ... counted from chunk indices: chunk id of frame a = (a / K) cpf + (a mod K) / 8
    const unsigned __int128 first_id = (unsigned __int128)(c / K) * cpf + (c % K) / 8;
    const unsigned __int128 last_id = F ? (unsigned __int128)((uint64_t)((end - 1) / K)) * cpf + (uint64_t)((end - 1) % K) / 8 : first_id;
    CHECK((unsigned __int128)p.frames == frames, "frames");
    CHECK((unsigned __int128)p.chunks == (F ? last_id - first_id + 1 : 0), "chunks c=%" PRIu64 " F=%" PRIu64 " K=%u", c, F, K);
    CHECK(p.chunks <= fpow_max_chunks(F, K), "max chunks");
    g_calls++;
}

// ---- the two kernels' arithmetic, played on the host through the plan functions ------------------------------------------------
struct State
{
    uint64_t pos;
    float acc, partial;
};

static void play_call(State &st, const float *e, uint64_t F, uint32_t K, float scale, std::vector<float> *out)
{
    FpowPlan p;
    CHECK(fpow_plan(st.pos, F, K, &p), "plan");
    if (F == 0)
        return;
    float *work = new float[p.chunks]; // exactly its size: the sanitizer sees a chunk too many
    for (uint64_t q = 0; q < p.chunks; q++)
    {
        uint64_t row0;
        uint32_t count;
        bool from_partial;
        fpow_chunk_entry(p.chunk0, p.skip, (uint32_t)q, K, F, &row0, &count, &from_partial);
        float s = from_partial ? st.partial : 0.f;
        for (uint32_t u = 0; u < count; u++)
        {
            CHECK(row0 + u < F, "row");
            s = s + e[row0 + u];
        }
        work[q] = s;
    }
    float acc_out = st.acc, partial_out = st.partial;
    for (uint64_t t = 0; t < p.touched; t++)
    {
        uint64_t lo, hi;
        bool complete;
        fpow_frame_entry(p.chunk0, p.done, (uint32_t)t, K, &lo, &hi, &complete);
        float a = (t == 0 && p.chunk0 > 0) ? st.acc : 0.f;
        for (uint64_t q = lo; q < hi; q++)
            a = a + work[q];
        if (complete)
            out->push_back(a * scale);
        else
        {
            acc_out = a;
            if (p.done < p.chunks)
                partial_out = work[p.done];
        }
    }
    delete[] work;
    st.acc = acc_out;
    st.partial = partial_out;
    st.pos += F;
}

static std::vector<float> definition(const float *e, uint64_t F, uint32_t K, float scale)
{
    std::vector<float> out;
    for (uint64_t f = 0; (f + 1) * K <= F; f++)
    {
        float acc = 0.f;
        for (uint32_t c = 0; c < K; c += FPOW_CHUNK)
        {
            float part = 0.f;
            for (uint32_t s = c; s < K && s < c + FPOW_CHUNK; s++)
                part = part + e[f * K + s];
            acc = acc + part;
        }
        out.push_back(acc * scale);
    }
    return out;
}

static void cuts(uint32_t K, const std::vector<float> &e, const std::vector<uint64_t> &at, bool three)
{
    const uint64_t F = e.size();
    const float scale = fpow_scale(K, 1, 0.8125f);
    const std::vector<float> want = definition(e.data(), F, K, scale);
    for (uint64_t a : at)
        for (uint64_t b : at)
        {
            if (b < a || (!three && b != a))
                continue;
            State st{0, -1.f, -1.f}; // what nothing may read: a sum that took it in would not match
            std::vector<float> got;
            play_call(st, e.data(), a, K, scale, &got);
            play_call(st, e.data() + a, b - a, K, scale, &got);
            play_call(st, e.data() + b, F - b, K, scale, &got);
            CHECK(got.size() == want.size() && (got.empty() || !std::memcmp(got.data(), want.data(), got.size() * sizeof(float))),
                  "K=%u cuts %" PRIu64 " %" PRIu64 ": the bits differ", K, a, b);
            g_cuts++;
        }
}

static void rule(uint32_t B, uint32_t first, uint32_t G, uint32_t Bo, uint32_t K, bool norm_ok, bool ref_ok, uint32_t format, uint64_t max_frames,
                 const char *want)
{
    char msg[256] = "ok";
    const bool ok = fpow_config_ok(B, first, G, Bo, K, norm_ok, ref_ok, format, max_frames, msg);
    CHECK(ok == !std::strcmp(want, "ok") && !std::strcmp(msg, want), "rule: got \"%s\", want \"%s\"", msg, want);
    g_rules++;
}

static int query()
{
    char line[512];
    while (std::fgets(line, sizeof line, stdin))
    {
        unsigned long long c, F, mf;
        unsigned K, B, first, G, Bo, nok, rok, fmt;
        if (std::sscanf(line, "plan %llu %llu %u", &c, &F, &K) == 3)
        {
            FpowPlan p;
            if (!fpow_plan(c, F, K, &p))
                std::printf("refused\n");
            else
                std::printf("%" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %u %u %u %u\n", p.chunks, p.done, p.frames, p.touched, p.chunk0, p.skip,
                            p.open_chunks, p.open_frames);
        }
        else if (std::sscanf(line, "config %u %u %u %u %u %u %u %u %llu", &B, &first, &G, &Bo, &K, &nok, &rok, &fmt, &mf) == 9)
        {
            char msg[256] = "ok";
            fpow_config_ok(B, first, G, Bo, K, nok != 0, rok != 0, fmt, mf, msg);
            std::printf("%s\n", msg);
        }
        else if (std::sscanf(line, "work %llu %u", &F, &K) == 2)
            std::printf("%" PRIu64 "\n", fpow_max_chunks(F, K));
        else
            return std::printf("bad request: %s", line), 1;
    }
    return 0;
}

int main(int argc, char **argv)
{
    if (argc > 1 && !std::strcmp(argv[1], "query"))
        return query();
    std::vector<uint32_t> ks;
    for (uint32_t K = 1; K <= 20; K++)
        ks.push_back(K);
    ks.push_back(65535);
    const uint64_t two32 = (uint64_t)1 << 32;
    for (uint32_t K : ks)
    {
        std::vector<uint64_t> positions;
        for (uint64_t c = 0; c < (K <= 20 ? 2 * K + 1 : 20); c++)
            positions.push_back(c);
        if (K > 20)
            for (uint64_t c : {(uint64_t)K - 9, (uint64_t)K - 8, (uint64_t)K - 1, (uint64_t)K, (uint64_t)K + 1, (uint64_t)65528, (uint64_t)65527})
                positions.push_back(c);
        for (uint64_t base : {two32, UINT64_MAX - 4 * (uint64_t)K - 30})
            for (int64_t d = -3; d <= 3; d++)
                positions.push_back(base + (uint64_t)d);
        const uint64_t counts[] = {0, 1, 7, 8, 9, (uint64_t)K - 1, K, (uint64_t)K + 1, 3 * (uint64_t)K + 5};
        for (uint64_t c : positions)
            for (uint64_t F : counts)
                if (c + F >= c)
                    one_call(c, F, K);
        for (uint64_t c : {(uint64_t)0, (uint64_t)5, two32 - 1, two32 + 1, UINT64_MAX - two32, UINT64_MAX - two32 + 1, UINT64_MAX - 1, UINT64_MAX})
            for (uint64_t F : {(uint64_t)0, (uint64_t)1, (uint64_t)2, two32 - 1, two32})
                big_call(c, F, K);
        FpowPlan p;
        CHECK(!fpow_plan(0, two32 + 1, K, &p), "a call above 2^32 frames was not refused");
        // every cut
        std::vector<float> e(3 * (size_t)K);
        uint32_t seed = 12345u + K;
        for (float &v : e)
        {
            seed = seed * 1664525u + 1013904223u;
            v = (float)(seed >> 8) * (1.0f / 16777216.0f) + 0.001f; // 24 random bits: sums round
        }
        std::vector<uint64_t> at;
        if (K <= 20)
            for (uint64_t a = 0; a <= e.size(); a++)
                at.push_back(a);
        else
            for (uint64_t edge : {(uint64_t)0, (uint64_t)8, (uint64_t)16, (uint64_t)65528, (uint64_t)K, (uint64_t)K + 8, (uint64_t)K + 32768, 2 * (uint64_t)K, 3 * (uint64_t)K})
                for (int64_t d = -1; d <= 1; d++)
                    if ((int64_t)edge + d >= 0 && edge + d <= e.size())
                        at.push_back(edge + d);
        cuts(K, e, at, false);
        cuts(K, e, at, true);
        // workspace sizing
        uint64_t before = 0;
        for (uint64_t F = 0; F <= (K <= 20 ? 5 * (uint64_t)K + 20 : 40); F++)
        {
            const uint64_t most = fpow_max_chunks(F, K);
            CHECK(most >= before, "fpow_max_chunks decreases at F=%" PRIu64, F);
            before = most;
            for (uint64_t c = 0; c < (K <= 20 ? K : 30); c++)
            {
                FpowPlan q;
                CHECK(fpow_plan(c, F, K, &q) && q.chunks <= most, "K=%u F=%" PRIu64 " c=%" PRIu64 ": %" PRIu64 " chunks of at most %" PRIu64, K, F, c, q.chunks, most);
            }
        }
    }
    CHECK(fpow_max_chunks(two32, 1) == two32 && fpow_max_chunks(two32, 65535) == (two32 / 65535 + 2) * 8192, "fpow_max_chunks at 2^32");
    // the init rules in order, each with its message
    rule(918, 0, 1, 918, 20, true, true, 0, 4096, "ok");
    rule(8192, 0, 64, 1, 65535, true, true, 1, two32 / 2, "ok");
    rule(8192, 0, 64, 1, 65535, true, true, 1, two32,
         "a call of ullMaxFrames = 4294967296 frames would need 536895488 chunk sums of 1 bins; the workspace is limited to 2^29 values: lower ullMaxFrames");
    rule(0, 0, 1, 1, 1, true, true, 0, 1, "bins must be 1..8192 (got 0)");
    rule(8193, 0, 1, 1, 1, true, true, 0, 1, "bins must be 1..8192 (got 8193)");
    rule(64, 0, 0, 1, 1, true, true, 0, 1, "group must be 1..64 (got 0)");
    rule(64, 0, 65, 1, 1, true, true, 0, 1, "group must be 1..64 (got 65)");
    rule(64, 0, 1, 0, 1, true, true, 0, 1, "elements [0, 0) of 0 output bins in groups of 1 are outside the frame's 64 (ulOutBins >= 1)");
    rule(64, 1, 8, 8, 1, true, true, 0, 1, "elements [1, 65) of 8 output bins in groups of 8 are outside the frame's 64 (ulOutBins >= 1)");
    rule(64, 4294967295u, 64, 4294967295u, 1, true, true, 0, 1,
         "elements [4294967295, 279172874175) of 4294967295 output bins in groups of 64 are outside the frame's 64 (ulOutBins >= 1)");
    rule(64, 0, 1, 64, 0, true, true, 0, 1, "frames per output frame must be 1..65535 (got 0)");
    rule(64, 0, 1, 64, 65536, true, true, 0, 1, "frames per output frame must be 1..65535 (got 65536)");
    rule(64, 0, 1, 64, 8, false, true, 0, 1, "fNorm must be a finite value > 0");
    rule(64, 0, 1, 64, 8, true, false, 0, 1, "fRefPower must be a finite value > 0");
    rule(64, 0, 1, 64, 8, true, true, 2, 1, "unknown input format 2");
    rule(64, 0, 1, 64, 8, true, true, 0, 0, "ullMaxFrames must be 1..2^32 (got 0)");
    rule(64, 0, 1, 64, 8, true, true, 0, two32 + 1, "ullMaxFrames must be 1..2^32 (got 4294967297)");
    rule(8192, 0, 1, 8192, 1, true, true, 0, 65537,
         "a call of ullMaxFrames = 65537 frames would need 65537 chunk sums of 8192 bins; the workspace is limited to 2^29 values: lower ullMaxFrames");
    rule(8192, 0, 1, 8192, 1, true, true, 0, 65536, "ok");
    rule(0, 9, 0, 0, 0, false, false, 7, 0, "bins must be 1..8192 (got 0)"); // the first rule broken speaks
    std::printf("%llu calls, %llu cuts, %llu rules checked: OK\n", g_calls, g_cuts, g_rules);
    return 0;
}
