// psd_plan_check.cpp — stand-alone checker of qo-100-tools_amd/csrc/if_fir_psd_plan.h (docs/SPEC.md §8), the header the
// estimator's shim and kernel unit use.  Plain g++, its own main; tests/test_psd_host.py builds it with
// -fsanitize=address,undefined and runs it.
//
// For every N in {256 .. 4096}, H in {1, 3, N/4, N/2, N-1, N}, K in {1, 3, 8, 9, 20, 65535} and stream positions 0, just below
// and just above 2^32 samples, a run of calls whose lengths lie around the next segment, chunk and frame boundary:
//   - segments, chunks, frames and the carried samples of psd_plan equal a brute-force walk, chunk by chunk, of the definition;
//   - the carry stays below 7 H + N, the open chunk starts on a chunk boundary and is really incomplete;
//   - psd_chunk_entry lists exactly the chunks of the walk (first segment, size, frame) and every sample a chunk reads lies
//     inside (carried || call);
//   - the chunk and frame counts stay within psd_max_chunks / psd_max_frames of the call length;
//   - psd_bin_position is a permutation of 0 .. N-1 that matches the digit reversal of radix-4 passes and a last radix-2 pass.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "if_fir_psd_plan.h"

using namespace if_fir;

static unsigned long long g_calls = 0;

#define CHECK(cond, ...)                    \
    do                                      \
    {                                       \
        if (!(cond))                        \
        {                                   \
            std::printf("FAIL %s: ", #cond); \
            std::printf(__VA_ARGS__);       \
            std::printf("\n");              \
            std::exit(1);                   \
        }                                   \
    } while (0)

struct Walk
{
    uint64_t segments, chunks, frames, carry;
};

static uint64_t chunk_size(uint64_t s, uint32_t K)
{
    const uint64_t left = K - s % K;
    return left < (uint64_t)PSD_CHUNK ? left : (uint64_t)PSD_CHUNK;
}

// the definition, chunk by chunk: a chunk is summed when its last sample (s + size - 1) H + N - 1 is there
static Walk walk(uint64_t pos, uint64_t carried, uint64_t n, uint32_t N, uint32_t H, uint32_t K, std::vector<uint64_t> *firsts)
{
    const uint64_t s0 = (pos - carried) / H, total = pos + n;
    uint64_t s = s0;
    Walk w{0, 0, 0, 0};
    for (;;)
    {
        const uint64_t size = chunk_size(s, K);
        if ((s + size - 1) * H + N > total)
            break;
        if (firsts && firsts->size() < 64)
            firsts->push_back(s);
        s += size;
        w.chunks++;
    }
    w.segments = s - s0;
    w.frames = s / K - s0 / K;
    w.carry = total - s * H;
    return w;
}

static void one_call(uint64_t &pos, uint64_t &carried, uint64_t n, uint32_t N, uint32_t H, uint32_t K)
{
    PsdPlan p;
    CHECK(psd_plan(pos, carried, n, N, H, K, &p), "plan refused pos=%llu n=%llu", (unsigned long long)pos, (unsigned long long)n);
    std::vector<uint64_t> firsts;
    const Walk w = walk(pos, carried, n, N, H, K, &firsts);
    CHECK(p.segments == w.segments && p.chunks == w.chunks && p.frames == w.frames && p.carry == w.carry,
          "N=%u H=%u K=%u pos=%llu carried=%llu n=%llu: plan (%llu %llu %llu %llu) walk (%llu %llu %llu %llu)", N, H, K,
          (unsigned long long)pos, (unsigned long long)carried, (unsigned long long)n, (unsigned long long)p.segments,
          (unsigned long long)p.chunks, (unsigned long long)p.frames, (unsigned long long)p.carry, (unsigned long long)w.segments,
          (unsigned long long)w.chunks, (unsigned long long)w.frames, (unsigned long long)w.carry);
    CHECK(p.carry < (uint64_t)(PSD_CHUNK - 1) * H + N, "carry %llu N=%u H=%u", (unsigned long long)p.carry, N, H);
    CHECK(p.seg0 == (pos - carried) / H && p.chunk0 == (p.seg0 % K) / PSD_CHUNK, "seg0");
    CHECK(p.chunks <= psd_max_chunks(n, H, K) && p.frames <= psd_max_frames(n, H, K) && p.segments <= psd_max_segments(n, H),
          "bounds: %llu chunks of at most %llu", (unsigned long long)p.chunks, (unsigned long long)psd_max_chunks(n, H, K));
    // the chunk list the kernel derives
    for (size_t c = 0; c < firsts.size(); c++)
    {
        uint32_t seg_rel, count, frame_rel;
        psd_chunk_entry(p.chunk0, (uint32_t)c, K, &seg_rel, &count, &frame_rel);
        CHECK(p.seg0 + seg_rel == firsts[c] && count == chunk_size(firsts[c], K), "chunk %zu: segment %llu + %u, want %llu", c,
              (unsigned long long)p.seg0, seg_rel, (unsigned long long)firsts[c]);
        CHECK(frame_rel == firsts[c] / K - p.seg0 / K, "chunk %zu frame", c);
        // samples relative to the call's first one: [first, last]
        const int64_t first = (int64_t)seg_rel * H - (int64_t)carried, last = (int64_t)(seg_rel + count - 1) * H + N - 1 - (int64_t)carried;
        CHECK(first >= -(int64_t)carried && last < (int64_t)n, "chunk %zu reads [%lld, %lld] of [-%llu, %llu)", c, (long long)first,
              (long long)last, (unsigned long long)carried, (unsigned long long)n);
    }
    pos += n;
    carried = p.carry;
    // the state after: the open chunk starts on a boundary and lacks samples
    const uint64_t s = (pos - carried) / H;
    CHECK((pos - carried) % H == 0 && (s % K) % PSD_CHUNK == 0, "open chunk off a boundary");
    CHECK((s + chunk_size(s, K) - 1) * H + N > pos, "open chunk is complete");
    CHECK(p.open_chunks == (s % K) / PSD_CHUNK, "open_chunks");
    g_calls++;
}

static void config(uint32_t N, uint32_t H, uint32_t K, uint64_t start)
{
    uint64_t pos = 0, carried = 0;
    if (start)
        one_call(pos, carried, start, N, H, K); // (the walk is O(1) per chunk: a jump is only taken where it stays cheap)
    for (int round = 0; round < 3; round++)
    {
        const uint64_t s = (pos - carried) / H;
        const uint64_t done = pos < N ? 0 : (pos - N) / H + 1; // segments complete so far
        const uint64_t to_seg = done * H + N - pos;
        const uint64_t to_chunk = (s + chunk_size(s, K) - 1) * H + N - pos;
        const uint64_t to_frame = ((s / K + 1) * (uint64_t)K - 1) * H + N - pos;
        const uint64_t dist[3] = {to_seg, to_chunk, round == 2 ? to_frame : to_chunk + H};
        uint64_t fed = 0; // calls are consecutive: each feeds what is missing to reach its goal from the round's start
        for (uint64_t d : dist)
            for (int k = -1; k <= 1; k++)
            {
                const uint64_t goal = d + (uint64_t)(int64_t)k;
                const uint64_t n = goal > fed ? goal - fed : 0;
                one_call(pos, carried, n, N, H, K);
                fed += n;
            }
        one_call(pos, carried, 0, N, H, K);
        one_call(pos, carried, 1, N, H, K);
    }
    if (K <= 20)
        one_call(pos, carried, (2 * (uint64_t)K + 1) * H + 5, N, H, K);
}

int main()
{
    unsigned configs = 0;
    const uint32_t sizes[] = {256, 512, 1024, 2048, 4096};
    const uint32_t ks[] = {1, 3, 8, 9, 20, 65535};
    for (uint32_t N : sizes)
    {
        // bin positions: a permutation, equal to the digit reversal written out
        std::vector<int> seen(N, 0);
        for (uint32_t k = 0; k < N; k++)
        {
            const uint32_t p = psd_bin_position(k, N);
            CHECK(p < N && !seen[p], "bin position %u of %u", p, k);
            seen[p] = 1;
            uint32_t want = 0, len = N, kk = k;
            while (len >= 4)
            {
                len /= 4;
                want += (kk & 3) * len;
                kk >>= 2;
            }
            if (len == 2)
                want += kk & 1;
            CHECK(p == want, "bin %u of %u at %u, want %u", k, N, p, want);
        }
        const uint32_t hs[] = {1, 3, N / 4, N / 2, N - 1, N};
        for (uint32_t H : hs)
            for (uint32_t K : ks)
            {
                const uint64_t two32 = (uint64_t)1 << 32;
                // the jump to 2^32 walks (2^32 / H) / 8 chunks: taken where that is at most 4 Mi
                const uint64_t starts[] = {0, two32 - 3 * (uint64_t)N - 7, two32 + 11};
                for (uint64_t start : starts)
                {
                    if (start && (two32 / H) / (K < 8 ? K : 8) > (4u << 20))
                        continue;
                    config(N, H, K, start);
                    configs++;
                }
            }
    }
    // positions past 2^32 at every hop, also where the walk from 0 is too long: the state is built directly (an open chunk at segment
    // s with c samples carried) and the calls from there are walked
    for (uint32_t N : sizes)
        for (uint32_t H : {1u, 3u, N / 4, N / 2, N - 1, N})
            for (uint32_t K : ks)
                // an open chunk at the last chunk boundary at or below `base` samples: just above 2^32, and just below it, so
                // that the calls cross 2^32
                for (uint64_t base : {((uint64_t)1 << 32) + 12345, ((uint64_t)1 << 32) - 2 * (uint64_t)N - 40})
                {
                    const uint64_t s = (base / H / K) * K + (K > 8 ? 8 : 0);
                    uint64_t carried = N - 1, pos = s * H + carried;
                    const uint64_t before = pos;
                    for (uint64_t n : {(uint64_t)0, (uint64_t)1, (uint64_t)H, (uint64_t)7 * H, (uint64_t)N, (uint64_t)N + 41,
                                       (uint64_t)(K < 100 ? K : 100) * H + N})
                        one_call(pos, carried, n, N, H, K);
                    CHECK(before > ((uint64_t)1 << 32) || (K * (uint64_t)H > 3 * (uint64_t)N) || pos > ((uint64_t)1 << 32),
                          "the run from %llu did not cross 2^32", (unsigned long long)before);
                    configs++;
                }
    std::printf("%u configurations, %llu calls checked: OK\n", configs, g_calls);
    return 0;
}
