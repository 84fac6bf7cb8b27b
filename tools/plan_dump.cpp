// plan_dump.cpp — one listing of everything the plan headers qo-100-tools_amd/csrc/if_fir_X_plan.h of the streaming families
// compute, for comparing two versions of them: compile this file once against each (plain g++, -I the csrc directory, nothing
// else), run both and compare the outputs.  It calls the family-named functions only, so it builds against any version that
// keeps them.
//
// Per family, over the grid its plan checker under tests/c walks: every field of the shape, lds_bytes, groups_per_cu, the call
// plans at c in {0, 1, D-1, D, 2^32-3 .. 2^32+3, 2^40+3, 2^63, 2^63+D-1, 2^64-1-n} x n in {0, 1, 2, D-1, D, D+1, 1000} (D = the
// family's hop) and the tap tables and NCO-shifted taps (`mix`).  An image is printed as its length and the FNV-1a hash of its
// bytes; on a small sub-grid (FULL below) also value by value as hexadecimal floats.
#include <cstdio>
#include <cstring>
#include <vector>

#include "if_fir_arb_plan.h"
#include "if_fir_ddc_plan.h"
#include "if_fir_duc_plan.h"
#include "if_fir_pfb_plan.h"
#include "if_fir_psd_plan.h"
#include "if_fir_resamp_plan.h"
#include "if_fir_synth_plan.h"

using namespace if_fir;
typedef unsigned long long ull;

static void image(const char *name, const std::vector<float> &v, bool full)
{
    ull h = 1469598103934665603ull;
    const unsigned char *p = reinterpret_cast<const unsigned char *>(v.data());
    for (size_t i = 0; i < v.size() * sizeof(float); i++)
        h = (h ^ p[i]) * 1099511628211ull;
    printf("  %s %zu %016llx\n", name, v.size(), h);
    if (full)
        for (size_t i = 0; i < v.size(); i++)
            printf("    %a\n", v[i]);
}

static std::vector<ull> positions(ull D, ull n)
{
    return {0, 1, D - 1, D, 4294967293ull, 4294967294ull, 4294967295ull, 4294967296ull, 4294967297ull, 4294967298ull,
            4294967299ull, (1ull << 40) + 3, 1ull << 63, (1ull << 63) + D - 1, ~0ull - n};
}
static std::vector<ull> lengths(ull D)
{
    return {0, 1, 2, D - 1, D, D + 1, 1000};
}

// h[k] = (k + 1) / T, and as complex taps (h, -h / 2)
static std::vector<float> taps_of(int T, bool complex_taps)
{
    std::vector<float> h((size_t)T * (complex_taps ? 2 : 1));
    for (int k = 0; k < T; k++)
    {
        const float v = (float)(k + 1) / (float)T;
        if (complex_taps)
        {
            h[2 * k] = v;
            h[2 * k + 1] = -0.5f * v;
        }
        else
            h[k] = v;
    }
    return h;
}

static const uint32_t WORDS[5] = {0u, 1u, 1u << 31, 0xffffffffu, 858993459u}; // the last: llround(0.2 2^32)
static bool FULL(int hop, int T)
{
    return (hop == 1 || hop == 3 || hop == 64) && (T == 1 || T == 255);
}

static void dump_resamp()
{
    for (int L = 1; L <= RESAMP_MAX_L; L++)
        for (int M = 1; M <= RESAMP_MAX_M; M++)
        {
            const int Ts[6] = {1, L - 1, L, L + 1, 255, 4096};
            for (int T : Ts)
            {
                if (T < 1)
                    continue;
                const ResampShape s = resamp_shape(T, L, M);
                printf("resamp shape L=%d M=%d T=%d: %d %d %d %d %d %d %d %d hist %d lds %zu %zu\n", L, M, T, s.K, s.KP, s.W, s.B, s.tile_out,
                       s.tile_in, s.x_len, s.tap_entries, resamp_hist_len(T, L), resamp_lds_bytes(s, 0), resamp_lds_bytes(s, 1));
                if (M == 1 || M == 64)
                    for (int ct = 0; ct < 2; ct++)
                    {
                        std::vector<float> tab((size_t)s.tap_entries * (ct ? 2 : 1), -1.0f);
                        resamp_build_taps(taps_of(T, ct).data(), T, ct, L, tab.data());
                        image(ct ? "ctable" : "table", tab, FULL(L, T) && M == 1);
                    }
            }
            for (ull n : lengths((ull)M))
                for (ull c : positions((ull)M, n))
                {
                    ResampCall call;
                    if (resamp_call(c, n, L, M, &call))
                        printf("resamp call L=%d M=%d c=%llu n=%llu: %llu %llu %u\n", L, M, c, n, (ull)call.m0, (ull)call.count, call.t0);
                    else
                        printf("resamp call L=%d M=%d c=%llu n=%llu: refused\n", L, M, c, n);
                }
            int p, dq;
            resamp_period_entry(M - 1, L - 1, L, M, &p, &dq);
            printf("resamp period L=%d M=%d: %d %d\n", L, M, p, dq);
        }
}

static void dump_psd()
{
    for (uint32_t N = 0; N <= 8193; N++)
        if (psd_size_ok(N))
            printf("psd size %u\n", N);
    for (uint32_t N = PSD_MIN_N; N <= (uint32_t)PSD_MAX_N; N *= 2)
    {
        std::vector<float> pos(N);
        for (uint32_t k = 0; k < N; k++)
            pos[k] = (float)psd_bin_position(k, N);
        image("psd bin positions", pos, false);
        const uint32_t Hs[6] = {1, 3, N / 4, N / 2, N - 1, N}, Ks[6] = {1, 3, 8, 9, 20, 65535};
        for (uint32_t H : Hs)
            for (uint32_t K : Ks)
            {
                const ull starts[3] = {0, (4294967296ull / H) * H - 5ull * H, (4294967296ull / H + 3) * H};
                for (ull start : starts)
                {
                    ull position = start, carried = 0;
                    const ull ns[8] = {0, 1, N - 1, N, (ull)7 * H + N, 1000, (ull)K * H, 100000};
                    for (ull n : ns)
                    {
                        PsdPlan plan;
                        if (!psd_plan(position, carried, n, N, H, K, &plan))
                        {
                            printf("psd plan N=%u H=%u K=%u pos=%llu carried=%llu n=%llu: refused\n", N, H, K, position, carried, n);
                            continue;
                        }
                        printf("psd plan N=%u H=%u K=%u pos=%llu carried=%llu n=%llu: %llu %llu %llu %llu %llu %u %u max %llu %llu %llu\n", N, H, K,
                               position, carried, n, (ull)plan.seg0, (ull)plan.segments, (ull)plan.chunks, (ull)plan.frames, (ull)plan.carry,
                               plan.chunk0, plan.open_chunks, (ull)psd_max_segments(n, H), (ull)psd_max_frames(n, H, K),
                               (ull)psd_max_chunks(n, H, K));
                        for (uint32_t c = 0; c < plan.chunks && c < 4; c++)
                        {
                            uint32_t seg_rel, count, frame_rel;
                            psd_chunk_entry(plan.chunk0, c, K, &seg_rel, &count, &frame_rel);
                            printf("  chunk %u: %u %u %u\n", c, seg_rel, count, frame_rel);
                        }
                        position += n;
                        carried = plan.carry;
                    }
                }
            }
    }
}

static void dump_ddc()
{
    for (int D = 1; D <= DDC_MAX_D; D++)
    {
        const int Ts[13] = {1, D - 1, D, D + 1, 4 * D, 4 * D + 1, 16 * D, 16 * D + 1, 17 * D, 255, 1023, 4095, 4096};
        for (int T : Ts)
        {
            if (T < 1 || T > DDC_MAX_TAPS)
                continue;
            const DdcShape s = ddc_shape(T, D);
            printf("ddc shape T=%d D=%d: %d %d %d %d %d %d %d lds %zu per_cu %d\n", T, D, s.K, s.G, s.tile_out, s.tile_in, s.cols, s.RS,
                   s.tap_entries, ddc_lds_bytes(s, D), ddc_groups_per_cu(s, D));
            for (uint32_t word : WORDS)
                for (int ct = 0; ct < 2; ct++)
                {
                    std::vector<float> g(2 * (size_t)T, -1.0f), tab(2 * (size_t)s.tap_entries, -1.0f);
                    ddc_mix_taps(taps_of(T, ct).data(), T, ct, word, g.data());
                    ddc_build_table(g.data(), T, D, tab.data());
                    printf(" word %u complex %d\n", word, ct);
                    image("mix", g, FULL(D, T));
                    image("table", tab, FULL(D, T));
                }
        }
        for (ull n : lengths((ull)D))
            for (ull c : positions((ull)D, n))
            {
                DdcCall call;
                if (ddc_call(c, n, D, &call))
                    printf("ddc call D=%d c=%llu n=%llu: %u %llu %llu\n", D, c, n, call.n0, (ull)call.count, call.count ? (ull)call.first : 0ull);
                else
                    printf("ddc call D=%d c=%llu n=%llu: refused\n", D, c, n);
            }
        DdcCall call;
        printf("ddc call D=%d past 2^64: %d\n", D, (int)ddc_call(~0ull - 5, 10, D, &call));
    }
}

static void dump_duc()
{
    for (int L = 1; L <= DUC_MAX_L; L++)
    {
        const int Ts[15] = {1, L - 1, L, L + 1, 2 * L, 2 * L + 1, 15 * L, 16 * L, 16 * L + 1, 17 * L, 33 * L, 255, 1023, 4095, 4096};
        for (int T : Ts)
        {
            if (T < 1 || T > DUC_MAX_TAPS)
                continue;
            const DucShape s = duc_shape(T, L);
            printf("duc shape T=%d L=%d: %d %d %d %d %d %d %d %d %d lds %zu per_cu %d magic %u\n", T, L, s.K, s.KP, s.top, s.Q, s.tile_out,
                   s.window, s.RS, s.x_floats, s.tap_entries, duc_lds_bytes(s, L), duc_groups_per_cu(s, L), duc_div_magic(L));
            for (uint32_t word : WORDS)
                for (int ct = 0; ct < 2; ct++)
                {
                    std::vector<float> g(2 * (size_t)T, -1.0f), tab(2 * (size_t)s.tap_entries, -1.0f);
                    duc_mix_taps(taps_of(T, ct).data(), T, ct, word, g.data());
                    duc_build_table(g.data(), T, L, tab.data());
                    printf(" word %u complex %d\n", word, ct);
                    image("mix", g, FULL(L, T));
                    image("table", tab, FULL(L, T));
                }
        }
        for (ull n : lengths((ull)L))
            for (ull c : positions((ull)L, n))
            {
                uint64_t count;
                if (duc_call(c, n, L, &count))
                    printf("duc call L=%d c=%llu n=%llu: %llu\n", L, c, n, (ull)count);
                else
                    printf("duc call L=%d c=%llu n=%llu: refused\n", L, c, n);
            }
    }
    const float vs[12] = {0.0f, -0.0f, 1.0f, -1.0f, 0.99998474f, 0.5f / 32768.0f, 1.5f / 32768.0f, 2.5f / 32768.0f, -1.00002f, 7.0f, -7.0f, 1e-30f};
    for (float v : vs)
        printf("duc i16 %a: %d\n", v, (int)duc_to_i16(v));
}

static void dump_arb()
{
    for (int b = ARB_MIN_BITS; b <= ARB_MAX_BITS; b++)
    {
        const int P = 1 << b, Ts[6] = {1, P - 1, P, P + 1, 255, 8192};
        const uint64_t Rs[5] = {ARB_MIN_STEP, ARB_MAX_STEP, (uint64_t)63 << 26 | 1, 1234567891ull, ((uint64_t)3 << 32) + 1234567};
        for (int T : Ts)
        {
            for (uint64_t R : Rs)
            {
                const ArbShape s = arb_shape(T, b, R);
                printf("arb shape T=%d b=%d R=%llu: %d %d %d %d %d %d lds %zu valid %d\n", T, b, (ull)R, s.K, s.KP, s.P, s.tile_out, s.x_len,
                       s.tap_entries, arb_lds_bytes(s), (int)arb_valid((uint32_t)T, (uint32_t)b, R));
            }
            std::vector<float> tab(2 * (size_t)P * arb_row_stride(arb_phase_taps(T, b)), -1.0f);
            arb_build_taps(taps_of(T, false).data(), T, b, tab.data());
            image("table", tab, b == 4 && T == 1);
        }
        for (uint64_t R : Rs)
        {
            for (ull n : lengths(4))
                for (ull c : positions(4, n))
                {
                    const arb_u128 taus[3] = {(arb_u128)c << 32, ((arb_u128)c << 32) + 12345, ((arb_u128)c << 32) + (((arb_u128)1 << 34) - 1)};
                    for (arb_u128 tau : taus)
                    {
                        uint64_t count = 0;
                        const bool ok = arb_out_count(c, tau, n, R, &count);
                        printf("arb count b=%d R=%llu c=%llu n=%llu tau+%llu: %d %llu state %d\n", b, (ull)R, c, n, (ull)(tau - ((arb_u128)c << 32)),
                               (int)ok, (ull)count, (int)arb_state_ok(c, tau));
                    }
                }
            const ull is[4] = {0, 1, 1023, (1ull << 43) - 1};
            for (ull i : is)
            {
                int64_t q;
                uint32_t f;
                arb_time(((uint64_t)1 << 34) - 1, i, R, &q, &f);
                int dq, p;
                float mu;
                arb_place(f, 1023, R, b, &dq, &p, &mu);
                printf("arb time b=%d R=%llu i=%llu: %lld %u place %d %d %a\n", b, (ull)R, i, (long long)q, f, dq, p, mu);
            }
        }
    }
    printf("arb step %llu %llu %llu\n", (ull)arb_step_from_rates(48000.0, 44100.0), (ull)arb_step_from_rates(1.0, 65.0), (ull)arb_step_from_rates(4.0, 1.0));
}

static void dump_pfb()
{
    for (uint32_t M = 0; M <= 8193; M++)
        if (pfb_size_ok(M))
            printf("pfb size %u\n", M);
    for (uint32_t M = PFB_MIN_M; M <= (uint32_t)PFB_MAX_M; M *= 2)
    {
        printf("pfb M=%u: batch %u group_frames %u lds %zu per_cu %d\n", M, pfb_batch(M), pfb_group_frames(M), pfb_lds_bytes(M), pfb_groups_per_cu(M));
        const uint32_t Ts[7] = {1, M - 1, M, M + 1, 3 * M - 5, 16 * M - 1, 16 * M}, Ds[6] = {1, 17, M / 2, 3 * M / 4, M - 1, M};
        for (uint32_t T : Ts)
        {
            std::vector<float> tab((size_t)pfb_rows(T, M) * M, -1.0f);
            pfb_build_taps(taps_of((int)T, false).data(), T, M, tab.data());
            printf("pfb M=%u T=%u rows %u\n", M, T, pfb_rows(T, M));
            image("taps", tab, false);
            for (uint32_t D : Ds)
            {
                std::vector<ull> ns = lengths(D);
                ns.push_back(1ull << 36);
                for (ull n : ns)
                    for (ull c : positions(D, n))
                    {
                        PfbCall call;
                        if (pfb_call(c, n, M, D, T, &call))
                            printf("pfb call M=%u T=%u D=%u c=%llu n=%llu: %llu %llu %u %u %u\n", M, T, D, c, n, (ull)call.frames, (ull)call.groups,
                                   call.frames ? call.n0 : 0u, call.cmod, call.carry);
                        else
                            printf("pfb call M=%u T=%u D=%u c=%llu n=%llu: refused\n", M, T, D, c, n);
                    }
            }
        }
        const int32_t firsts[4] = {-(int32_t)M / 2, -1, 0, (int32_t)M - 1};
        for (int32_t first : firsts)
        {
            std::vector<float> places(M);
            for (uint32_t j = 0; j < M; j++)
                places[j] = (float)(pfb_bin_channel(first, j, M) * 8192u + pfb_bin_place(first, j, M));
            printf("pfb M=%u first_bin %d\n", M, first);
            image("places", places, false);
        }
    }
    PfbCall call;
    printf("pfb refusals %d %d %d %d\n", (int)pfb_call(~0ull - 5, 10, 64, 3, 100, &call), (int)pfb_call(5, 10, 64, 0, 100, &call),
           (int)pfb_call(5, 10, 0, 3, 100, &call), (int)pfb_call(5, 10, 64, 3, 0, &call));
}

static void dump_synth()
{
    for (uint32_t M = 0; M <= 8193; M++)
        if (synth_size_ok(M))
            printf("synth size %u\n", M);
    for (uint32_t M = 64; M <= 4096; M *= 2)
    {
        printf("synth M=%u: batch %u lds %zu per_cu %d\n", M, synth_batch(M), synth_lds_bytes(M), synth_groups_per_cu(M));
        const uint32_t Ls[6] = {1, 17, M / 2, 3 * M / 4, M - 1, M};
        for (uint32_t L : Ls)
        {
            const uint32_t Ts[10] = {1, L, L + 1, M - 1, M, 3 * M - 5, 16 * M - 1, 16 * M, 32 * L, 32 * L + 1};
            for (uint32_t T : Ts)
            {
                if (T < 1 || T > 16 * M)
                    continue;
                const uint32_t J = synth_terms(T, L);
                printf("synth M=%u T=%u L=%u: ok %d J %u\n", M, T, L, (int)synth_config_ok(M, T, L), J);
                if (!synth_config_ok(M, T, L))
                    continue;
                printf("  ring %zu fits %d preferred %d per_cu %d routes %u %u %u %u\n", synth_lds_route_bytes(M, J), (int)synth_lds_route_fits(M, J),
                       (int)synth_lds_route_preferred(M, J), synth_lds_route_groups_per_cu(M, J), synth_route(M, J, 0), synth_route(M, J, 1),
                       synth_route(M, J, 2), synth_route(M, J, 3));
                const ull budgets[4] = {1, (ull)M * 8 * 40, SYNTH_WORKSPACE_DEFAULT, SYNTH_WORKSPACE_MAX + 1};
                for (ull bytes : budgets)
                {
                    const ull wf = synth_workspace_frames(bytes, M, J), cf = synth_chunk_frames(wf, J);
                    const ull F = 100001, per = synth_even_chunk_frames(F, cf), chunks = synth_chunks(F, per);
                    const SynthChunk last = synth_chunk(chunks - 1, F, per, M, L, 5 % M);
                    printf("  workspace %llu: %llu %llu %llu %llu last %llu %llu %u runs %llu\n", bytes, wf, cf, per, chunks, (ull)last.first,
                           (ull)last.frames, last.smod, (ull)synth_run_batches(chunks, 7));
                }
                std::vector<float> tab((size_t)J * L, -1.0f);
                synth_build_taps(taps_of((int)T, false).data(), T, L, tab.data());
                image("taps", tab, false);
                const ull Fs[7] = {0, 1, 2, 999, 1000, 1001, 1ull << 32};
                const ull cs[8] = {0, 1, 4294967295ull, 4294967296ull, (1ull << 40) + 12345, 1ull << 63, ~0ull / L - 1000, ~0ull - 1000};
                for (ull F : Fs)
                    for (ull c : cs)
                    {
                        SynthCall call;
                        if (synth_call(c, F, M, L, T, &call))
                            printf("  call c=%llu F=%llu: %llu %u %u\n", c, F, (ull)call.outputs, call.smod, call.carry);
                        else
                            printf("  call c=%llu F=%llu: refused\n", c, F);
                    }
            }
        }
        std::vector<float> places(M), index(M);
        for (uint32_t s = 0; s < M; s++)
        {
            places[s] = (float)synth_slot_place(s, M);
            index[s] = (float)synth_channel_index(-(int32_t)M / 2 + 3, s, M);
        }
        image("slot places", places, false);
        image("channel index", index, false);
    }
}

int main()
{
    dump_resamp();
    dump_psd();
    dump_ddc();
    dump_duc();
    dump_arb();
    dump_pfb();
    dump_synth();
    return 0;
}
