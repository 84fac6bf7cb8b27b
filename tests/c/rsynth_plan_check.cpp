// rsynth_plan_check.cpp — walks qo-100-tools_amd/csrc/if_fir_rsynth_plan.h (and what it shares of if_fir_synth_plan.h), the
// planning the real-output synthesis bank's shim and kernels use, with a plain host compiler (tests/test_rsynth_host.py builds
// it plain and with -fsanitize=address,undefined and runs it directly).
//
// Without arguments, every M of the list with T in {1, L, L+1, M-1, M, 3M-5, 16M-1, 16M, 32L, 32L+1} (those within 1..16M) and
// L in {1, 17, M/2, 3M/4, M-1, M}: J = ceil(T / L), accepted up to 32 and refused from 33; the sizes 64 and 16384 and the spans
// past M/2 + 1 refused; the batch fills the 256 lanes and the transform kernel's LDS fits a CU, twice at M = 8192;
// the tap table, built into a heap buffer of exactly its size, holds h[t] at t and zeros from T on; the places are the mirrored
// permutation of the M/2-point transform; the pre-tangle table, in a heap buffer of exactly its size, holds float64 cos and sin
// of 2 pi k / M rounded once, and (-re, im) of entry k is that of H - k; for workspace budgets from 1 byte to the default and F
// around the multiples of a chunk, the chunks cover every frame of a call once, in order, a chunk's rows of 4 M bytes fit the
// workspace, every row an output reads lies inside it, and a chunk's first output index modulo M is the absolute one (128-bit
// arithmetic here); for frame positions up to 2^64 a call is refused exactly when (c + F) L passes 2^64 - 1, outputs = F L,
// (c L) mod M, carry = J - 1.  At M = 128 and 256 (H = 64, and 128 with its last radix-2 pass): random channels through the
// pre-tangle with the table's twiddles, a host restatement of the in-place radix-4 transform and the places, against the
// definition's sum over the channels by brute force.
//
// `rsynth_plan_check query` answers one request per line of standard input: `config M T L` -> J (or `refused`), `span M first
// bins` -> ok / refused, `call c F M L T` -> outputs smod carry (or `refused`), `shape M` -> batch pair_items lds_bytes
// groups_per_cu, `chunks F bytes M T L smod` -> count, then first frames smod per chunk, `taps T L` -> the table of the taps
// k + 1, `place M n` -> place, `twiddle M k` -> re im (%.9g).
#include <cmath>
#include <complex>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "if_fir_rsynth_plan.h"

typedef unsigned __int128 u128;
typedef std::complex<double> cd;

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
            if (rsynth_config_ok(M, T, L))
                printf("%u\n", synth_terms(T, L));
            else
                printf("refused\n");
        }
        else if (!strcmp(word, "span") && sscanf(line, "%*s %u %u %u", &M, &T, &L) == 3)
            printf(rsynth_span_ok(T, L, M) ? "ok\n" : "refused\n");
        else if (!strcmp(word, "call") && sscanf(line, "%*s %llu %llu %u %u %u", &c, &n, &M, &L, &T) == 5)
        {
            SynthCall call;
            if (!synth_call(c, n, M, L, T, &call))
                printf("refused\n");
            else
                printf("%llu %u %u\n", (unsigned long long)call.outputs, call.smod, call.carry);
        }
        else if (!strcmp(word, "shape") && sscanf(line, "%*s %u", &M) == 1 && rsynth_size_ok(M))
            printf("%u %u %zu %d\n", rsynth_batch(M), rsynth_pair_items(M), rsynth_lds_bytes(M), rsynth_groups_per_cu(M));
        else if (!strcmp(word, "chunks") && sscanf(line, "%*s %llu %llu %u %u %u %u", &n, &c, &M, &T, &L, &s) == 6 && rsynth_config_ok(M, T, L))
        {
            const unsigned J = synth_terms(T, L);
            const unsigned long long most = synth_chunk_frames(rsynth_workspace_frames(c, M, J), J), per = synth_even_chunk_frames(n, most),
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
        else if (!strcmp(word, "place") && sscanf(line, "%*s %u %u", &M, &s) == 2 && rsynth_size_ok(M) && s < M / 2)
            printf("%u\n", rsynth_slot_place(s, M));
        else if (!strcmp(word, "twiddle") && sscanf(line, "%*s %u %u", &M, &s) == 2 && rsynth_size_ok(M) && s <= M / 4)
        {
            std::vector<float> w(2 * (size_t)rsynth_pair_items(M));
            rsynth_build_twiddles(M, w.data());
            printf("%.9g %.9g\n", w[2 * s], w[2 * s + 1]);
        }
        else
        {
            printf("bad request: %s", line);
            return 2;
        }
    }
    return 0;
}

// the shared in-place transform restated on the host in float64: radix-4 decimation-in-frequency passes over sub-blocks of len
// (butterfly j of a sub-block on the places j, j + len/4, j + len/2, j + 3 len/4), one last radix-2 pass where len ends at 2
static void dif_passes(std::vector<cd> &x, unsigned N)
{
    const double tau = 6.283185307179586476925286766559;
    unsigned len = N;
    for (; len >= 4; len /= 4)
    {
        const unsigned q = len / 4;
        for (unsigned base0 = 0; base0 < N; base0 += len)
            for (unsigned j = 0; j < q; j++)
            {
                const unsigned b = base0 + j;
                const cd a0 = x[b], a1 = x[b + q], a2 = x[b + 2 * q], a3 = x[b + 3 * q];
                const cd t0 = a0 + a2, t1 = a0 - a2, t2 = a1 + a3, t3 = cd(0, -1) * (a1 - a3);
                x[b] = t0 + t2;
                x[b + q] = (t1 + t3) * std::polar(1.0, -tau * j / len);
                x[b + 2 * q] = (t0 - t2) * std::polar(1.0, -tau * 2 * j / len);
                x[b + 3 * q] = (t1 - t3) * std::polar(1.0, -tau * 3 * j / len);
            }
    }
    if (len == 2)
        for (unsigned b = 0; b < N; b += 2)
        {
            const cd a0 = x[b], a1 = x[b + 1];
            x[b] = a0 + a1;
            x[b + 1] = a0 - a1;
        }
}

// random channels 0 .. H of one frame through the kernel's steps against the definition's sum, in float64
static int check_slots(unsigned M)
{
    using namespace if_fir;
    const unsigned H = M / 2;
    const double tau = 6.283185307179586476925286766559;
    std::vector<cd> X(H + 1), Z(H);
    unsigned long long seed = 12345 + M;
    for (unsigned k = 0; k <= H; k++)
    {
        double v[2];
        for (double &u : v)
        {
            seed = seed * 6364136223846793005ull + 1442695040888963407ull;
            u = (double)(seed >> 11) / 9007199254740992.0 - 0.5;
        }
        X[k] = cd(v[0], v[1]); // channels 0 and H with imaginary parts: ignored
    }
    std::vector<float> w(2 * (size_t)rsynth_pair_items(M));
    rsynth_build_twiddles(M, w.data());
    Z[0] = cd(X[0].real() + X[H].real(), X[0].real() - X[H].real());
    for (unsigned k = 1; k < H; k++)
    {
        const unsigned e = k <= H / 2 ? k : H - k;
        const cd W = k <= H / 2 ? cd(w[2 * e], w[2 * e + 1]) : cd(-w[2 * e], w[2 * e + 1]);
        const cd A = X[k], B = X[H - k];
        Z[k] = (A + std::conj(B)) + cd(0, 1) * W * (A - std::conj(B));
    }
    dif_passes(Z, H);
    double worst = 0, peak = 0;
    for (unsigned s = 0; s < M; s++)
    {
        double want = X[0].real() + ((s & 1) ? -1.0 : 1.0) * X[H].real();
        for (unsigned k = 1; k < H; k++)
            want += 2.0 * (X[k] * std::polar(1.0, tau * (double)((unsigned long long)k * s % M) / M)).real();
        const cd z = Z[rsynth_slot_place(s / 2, M)];
        const double got = (s & 1) ? z.imag() : z.real();
        worst = fabs(got - want) > worst ? fabs(got - want) : worst;
        peak = fabs(want) > peak ? fabs(want) : peak;
    }
    // (the table's twiddles are float32: 6e-8 each)
    if (!(worst <= 2e-6 * peak))
    {
        printf("FAILED: slots at M=%u: worst %g of peak %g\n", M, worst, peak);
        return 1;
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
    const unsigned Ms[7] = {128, 256, 512, 1024, 2048, 4096, 8192};
    if (rsynth_size_ok(64) || rsynth_size_ok(96) || rsynth_size_ok(192) || rsynth_size_ok(16384) || rsynth_size_ok(0))
        return fail("a size outside the list was accepted", 0, 0, 0, 0, 0);
    if (check_slots(128) || check_slots(256))
        return 1;
    for (unsigned M : Ms)
    {
        if (!rsynth_size_ok(M))
            return fail("size refused", M, 0, 0, 0, 0);
        const unsigned H = M / 2, B = rsynth_batch(M), P = rsynth_pair_items(M);
        if (B < 1 || B * H < (unsigned)STREAM_BANK_POINTS || (B > 1 && B * H != (unsigned)STREAM_BANK_POINTS) || (B * H) % RSYNTH_THREADS)
            return fail("batch", M, 0, 0, 0, 0);
        const int per_cu = rsynth_groups_per_cu(M);
        if (P != H / 2 + 1 || rsynth_lds_bytes(M) != (size_t)B * H * 8 + (size_t)H * 10 || per_cu < 1 || per_cu > 8 ||
            (size_t)per_cu * rsynth_lds_bytes(M) > (size_t)STREAM_LDS_PER_CU ||
            (per_cu < 8 && (size_t)(per_cu + 1) * rsynth_lds_bytes(M) <= (size_t)STREAM_LDS_PER_CU) || (M == 8192 && per_cu != 2))
            return fail("LDS", M, 0, 0, 0, 0);
        // the spans: channels 0 .. M/2, no wrap
        if (!rsynth_span_ok(0, H + 1, M) || !rsynth_span_ok(H, 1, M) || !rsynth_span_ok(0, 1, M) || rsynth_span_ok(0, H + 2, M) ||
            rsynth_span_ok(H, 2, M) || rsynth_span_ok(H + 1, 1, M) || rsynth_span_ok(3, 0, M) || rsynth_span_ok(~0u, 2, M))
            return fail("span", M, 0, 0, 0, 0);
        // the places: the permutation of the shared H-point transform, mirrored; slot pair 0 is bin 0
        std::vector<char> seen(H, 0);
        for (unsigned n = 0; n < H; n++)
        {
            const unsigned p = rsynth_slot_place(n, M);
            if (p >= H || seen[p] || p != psd_bin_position((H - n) % H, H))
                return fail("place", M, 0, 0, n, 0);
            seen[p] = 1;
        }
        if (rsynth_slot_place(0, M) != 0)
            return fail("place of slot 0", M, 0, 0, 0, 0);
        // the pre-tangle table: exactly its size; float64 cos and sin rounded once; (-re, im) of entry k is the twiddle of H - k
        {
            float *w = (float *)malloc(2 * (size_t)P * sizeof(float));
            if (!w)
                return fail("out of memory", M, 0, 0, 0, 0);
            rsynth_build_twiddles(M, w);
            const double tau = 6.283185307179586476925286766559;
            for (unsigned k = 0; k < P; k++)
            {
                const double a = tau * (double)k / (double)M, b = tau * (double)(H - k) / (double)M;
                // (entries 0 and H/2 are never mirrored: item 0 makes Z_0 alone, item H/2 is its own partner)
                const bool mirrored = k >= 1 && k < H / 2;
                if (w[2 * k] != (float)cos(a) || w[2 * k + 1] != (float)sin(a) ||
                    (mirrored && (-w[2 * k] != (float)cos(b) || w[2 * k + 1] != (float)sin(b))))
                {
                    free(w);
                    return fail("pre-tangle twiddle", M, 0, 0, k, 0);
                }
            }
            if (w[0] != 1.0f || w[1] != 0.0f || fabsf(w[2 * (P - 1)]) > 1e-7f || w[2 * (P - 1) + 1] != 1.0f)
            {
                free(w);
                return fail("pre-tangle twiddle ends", M, 0, 0, 0, 0);
            }
            free(w);
        }
        const unsigned Ls[6] = {1, 17, M / 2, 3 * M / 4, M - 1, M};
        for (unsigned L : Ls)
        {
            const unsigned Ts[10] = {1, L, L + 1, M - 1, M, 3 * M - 5, 16 * M - 1, 16 * M, 32 * L, 32 * L + 1};
            for (unsigned T : Ts)
            {
                if (T < 1 || T > 16 * M)
                {
                    if (rsynth_config_ok(M, T, L))
                        return fail("taps outside 1..16 M accepted", M, T, L, 0, 0);
                    continue;
                }
                const unsigned J = synth_terms(T, L);
                if (J < 1 || (unsigned long long)J * L < T || (unsigned long long)(J - 1) * L >= T)
                    return fail("terms", M, T, L, 0, 0);
                if (rsynth_config_ok(M, T, L) != (J <= 32))
                    return fail(J <= 32 ? "a configuration with J <= 32 was refused" : "J = 33 or more was accepted", M, T, L, 0, 0);
                if (J > 32)
                    continue;
                shapes++;
                if (rsynth_config_ok(M, T, 0) || rsynth_config_ok(M, T, M + 1) || rsynth_config_ok(M, 0, L) || rsynth_config_ok(M, 16 * M + 1, L))
                    return fail("a hop or a tap count outside its range was accepted", M, T, L, 0, 0);
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
                // chunking: budgets from nothing to the default; calls of 1 frame to many and around the multiples of a chunk
                const unsigned long long budgets[5] = {1, (unsigned long long)M * 4 * (J + 1), (unsigned long long)M * 4 * (J + 6), 1ull << 20,
                                                       RSYNTH_WORKSPACE_DEFAULT};
                const unsigned long long cs[3] = {0, (1ull << 40) + 12345, (~0ull / L) - 5000};
                for (unsigned long long bytes : budgets)
                {
                    const unsigned long long rows = rsynth_workspace_frames(bytes, M, J), most = synth_chunk_frames(rows, J);
                    if (rows < J || most < 1 || (rows > J && rows * M * 4 > bytes) || rows * M * 4 > RSYNTH_WORKSPACE_MAX)
                        return fail("workspace", M, T, L, bytes, 0);
                    const unsigned long long near = most < 1000 ? most : 1000;
                    const unsigned long long Fs[9] = {1, 2, J, 3ull * J + 7, near - (near > 1), near, near + 1, 2 * near - (near > 1), 2 * near + 1};
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
    if (synth_call(~0ull - 5, 10, 8192, 3, 100, &call) || synth_call(5, 10, 8192, 0, 100, &call) || synth_call(~0ull / 3, 1, 8192, 3, 100, &call))
        return fail("a position past 2^64, or a zero hop, was accepted", 8192, 100, 3, ~0ull - 5, 10);
    printf("%llu shapes, %llu calls, %llu chunks checked: OK\n", shapes, calls, chunks);
    return 0;
}
