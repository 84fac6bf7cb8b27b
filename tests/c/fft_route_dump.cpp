// fft_route_dump.cpp — prints the route of overlap-save calls as qo-100-tools_amd/csrc/if_fir_fft_route.h (the very header the
// launchers and the shim consume) decides it, one line per call, for tests/test_fft_matrix_gpu.py to compare its Python statement
// of the route with: every boundary tap count x decimation 1..64 x no bank / slots / own centres x NCO off / on.  Arguments, if
// any, are slot lists ("0,2,4,14,1"): the decimation-8 bank's plan for each (fft_bank8_plan, all-slots form available).
// Compiled with a plain g++ by the test, needs neither HIP nor a device.  Test infrastructure only.
#include <cstdio>
#include <cstdlib>
#include "if_fir_fft_route.h"
using namespace if_fir;

int main(int argc, char **argv)
{
    const int Ts[] = {1, 2, 3, 257, 258, 383, 384, 513, 514, 767, 768, 1025, 1026, 2049, 2050, 3073, 3074, 4095, 4096};
    for (int T : Ts)
        for (int D = 1; D <= 64; D++)
            for (int bank = FFT_NO_BANK; bank <= FFT_BANK_OWN_CENTRES; bank++)
                for (int nco = 0; nco < 2; nco++)
                {
                    const FftRoute r = fft_route(T, D, bank, nco != 0, false);
                    int oF = 0, oSub = 0, oOvlr = 0;
                    const int odd = fft_odd_tail(T, D, &oF, &oSub, &oOvlr) ? 1 : 0;
                    printf("R %d %d %d %d: family %d rows %d tail %d dec4 %d decn %d nco %d F %d sub %d hist %d | odd %d %d %d %d | "
                           "rows %d advance %d bank_tail %d %d\n",
                           T, D, bank, nco, r.family, r.rows, r.tail, (int)r.dec4, (int)r.decn, (int)r.nco, r.F, r.sub, r.hist_need, odd, oF,
                           oSub, oOvlr, fft_overlap_rows(T, D), fft_block_advance(T, D), fft_bank_tail(D, false), fft_bank_tail(D, true));
                }
    for (int i = 1; i < argc; i++)
    {
        uint32_t slots[32], count = 0, pmask[2] = {0, 0}, rest = 0;
        for (const char *p = argv[i]; *p && count < 32;)
        {
            char *end = nullptr;
            slots[count++] = (uint32_t)strtoul(p, &end, 10);
            p = (*end == ',') ? end + 1 : end;
        }
        fft_bank8_plan(slots, count, true, pmask, &rest);
        printf("P %s: even %u odd %u rest %u\n", argv[i], pmask[0], pmask[1], rest);
    }
    return 0;
}
