// combiner_tables_asan.cpp — the channel combiner's host arithmetic (qo-100-tools_amd/csrc/if_fir_combiner_tables.h: the split of
// a phase word, the multiply table of a residual) under AddressSanitizer + UndefinedBehaviorSanitizer on the CPU: a stand-alone
// program that tests/test_combiner_host.py compiles with -fsanitize=address,undefined and runs.  Every table is built into a heap
// buffer of exactly its size, so a write past the end lands in a red zone.  Test infrastructure only.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "if_fir_combiner_tables.h"

int main()
{
    using namespace if_fir;
    std::vector<float> taps(2 * 4096);
    for (size_t i = 0; i < taps.size(); i++)
        taps[i] = (float)((int)(i * 2654435761u % 2001) - 1000) / 1000.0f;
    const uint32_t words[] = {0u, 1u, (1u << 19) - 1u, 1u << 19, (1u << 19) + 1u, 1u << 20, (100u << 20) + (1u << 19), 1u << 31,
                              0xfff7ffffu, 0xfff80000u, 0xffffffffu, 860266324u};
    for (uint32_t P : words)
    {
        uint32_t G;
        int32_t r;
        combiner_split_word(P, &G, &r);
        if (G > 4095u || r < -(1 << 19) || r >= (1 << 19) || (uint32_t)((G << 20) + (uint32_t)r) != P)
            return printf("split of %u: G = %u, r = %d\n", P, G, r), 1;
        for (int T : {1, 2, 255, 3073, 4096})
            for (int ct = 0; ct < 2; ct++)
            {
                float *t = (float *)malloc(sizeof(float) * (size_t)T * (ct ? 2 : 1)); // exact-size taps too
                float *H = (float *)malloc(sizeof(float) * 2 * COMBINER_TABLE_N);
                for (int i = 0; i < T * (ct ? 2 : 1); i++)
                    t[i] = taps[i];
                combiner_residual_table(t, T, ct, r, H);
                if (T == 1 && !ct && !(H[0] == t[0] / 4096.0f && H[2 * 4095] == t[0] / 4096.0f))
                    return printf("one tap: H[0] = %g\n", H[0]), 1;
                free(H);
                free(t);
            }
    }
    printf("combiner host tables: clean\n");
    return 0;
}
