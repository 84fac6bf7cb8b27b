// fft_route_check.cpp — the route of every overlap-save call (qo-100-tools_amd/csrc/if_fir_fft_route.h, the very header the launchers
// and the shim consume) against the properties the design states (docs/SPEC.md): compiled with a
// plain g++ by tests/test_host.py, needs neither HIP nor a device.  Test infrastructure only.
#include <cstdio>
#include "if_fir_fft_route.h"
using namespace if_fir;

static int fails = 0;
#define CHECK(cond)                                                                                                       \
    do                                                                                                                    \
    {                                                                                                                     \
        if (!(cond) && fails++ < 20)                                                                                      \
            printf("FAIL T=%d D=%d bank=%d nco=%d no_fold=%d: %s\n", T, D, bank, nco, no_fold, #cond);                     \
    } while (0)

int main()
{
    const int Ts[] = {1, 2, 129, 257, 258, 513, 514, 1025, 1026, 2049, 2050, 3073, 3074, 4096}; // both ends of every tap class
    const int min_rows[] = {4, 4, 4, 4, 8, 8, 16, 16, 32, 32, 48, 48, 32, 32};                 // 64 rows >= T - 1 (two partitions: <= 2048 each)
    long routes = 0;
    for (int ti = 0; ti < 14; ti++)
        for (int D = 1; D <= 64; D++)
            for (int bank = FFT_NO_BANK; bank <= FFT_BANK_OWN_CENTRES; bank++)
                for (int nco = 0; nco < 2; nco++)
                    for (int no_fold = 0; no_fold < 2; no_fold++)
                    {
                        const int T = Ts[ti];
                        const FftRoute r = fft_route(T, D, bank, nco != 0, no_fold != 0);
                        routes++;
                        const bool two = T > 3073;
                        if (bank)
                        {
                            // the bank serves decimation 4, 8, 16 on the slot grid, every multiple of 4 with channels at their own
                            // centres, filters of one partition, and no common NCO where the tail's own decimation is 4
                            const bool served = !two && D % 4 == 0 && (bank == FFT_BANK_OWN_CENTRES || D == 4 || D == 8 || D == 16) &&
                                                !(nco && D % 8 != 0);
                            CHECK((r.family != FFT_FAMILY_NONE) == served);
                            if (!served)
                                continue;
                            CHECK(r.family == FFT_FAMILY_ROWS && tail_is_bank(r.tail) && r.dec4 && !r.decn);
                            CHECK(tail_own_centres(r.tail) == (bank == FFT_BANK_OWN_CENTRES && r.F != 8)); // (tail 8 serves both)
                            CHECK(r.F == (D % 16 == 0 ? 16 : D % 8 == 0 ? 8 : 4));
                        }
                        else
                        {
                            const bool odd = fft_odd_tail(T, D, nullptr, nullptr, nullptr) && !no_fold;
                            CHECK((r.family == FFT_FAMILY_ODD) == odd);
                            CHECK((r.family == FFT_FAMILY_TWO_PARTITIONS) == (two && !odd));
                            if (odd)
                            {
                                CHECK(r.image.kind == FFT_IMAGE_ODD && r.image.floats == fft_odd_table_floats(r.F) && r.image.nco_step == r.F);
                                CHECK(r.F * r.sub == D && r.F == 3 && (r.rows == 2 || r.rows == 4) && r.F * 64 * r.rows >= T - 1);
                                CHECK(r.hist_need == r.F * 64 * r.rows);
                                continue;
                            }
                            CHECK(tail_single(r.tail));
                            if (two) // two partitions: the 32-row kernel, single-channel tails only
                                CHECK(r.rows == 32 && r.tail <= TAIL_DEC2_SUB && r.image.images == 2 && r.hist_need == 4096);
                            // every even decimation runs behind a decimating tail; the fold can be switched off for F = 2 only
                            CHECK(r.F == (D % 4 == 0 ? 4 : (D % 2 == 0 && !no_fold) ? 2 : 1));
                            CHECK(r.decn == (r.F == 1 && D > 1));
                            CHECK(tail_in_dec2_units(r.tail) == (r.F == 2));
                        }
                        CHECK(tail_valid(r.tail));
                        CHECK(r.F == tail_factor(r.tail, r.dec4) && r.F * r.sub == D);
                        CHECK(tail_thins(r.tail) || r.decn || r.sub == 1);              // only a thinning tail (or the selecting store) drops outputs
                        CHECK(tail_sub_word(r.tail, r.dec4, D, 0) == (tail_thins(r.tail) ? (unsigned)r.sub : 1u));
                        CHECK(!r.nco || (nco && tail_has_nco(r.tail)));                 // no NCO form for a tail that has none
                        CHECK(r.nco || !nco || !tail_has_nco(r.tail));
                        CHECK(r.dec4 == (r.F > 1) && !(r.dec4 && r.rows < 4));          // a decimating tail drops whole rows of its fs/F-rate block
                        CHECK(r.rows == min_rows[ti] && (two || 64 * r.rows >= T - 1)); // the overlap covers the filter
                        CHECK(r.hist_need >= 64 * r.rows);
                        // the image is the one the tail's (cos, tan) trait demands
                        const int k = r.image.kind;
                        CHECK(tail_wants_tan(r.tail, r.dec4) == (k == FFT_IMAGE_DEC4 || k == FFT_IMAGE_BANK8 || k == FFT_IMAGE_BANK16));
                        CHECK((k == FFT_IMAGE_FULL_RATE) == !r.dec4 && (k == FFT_IMAGE_PLAIN) == tail_in_dec2_units(r.tail));
                        CHECK((k == FFT_IMAGE_DEC4) == (r.F == 4) && (k == FFT_IMAGE_BANK8) == (r.F == 8) && (k == FFT_IMAGE_BANK16) == (r.F == 16));
                        CHECK(r.image.nco_step == (tail_wants_tan(r.tail, r.dec4) ? r.F : 1)); // row phasors per kept output / per full-rate output
                        CHECK(r.image.images == ((two || k == FFT_IMAGE_BANK8) ? 2 : 1) && r.image.floats == r.image.images * FFT_TABLE_FLOATS);
                    }
    // outside the library's range: not served
    if (fft_route(0, 1, 0, false, false).family || fft_route(4097, 1, 0, false, false).family || fft_route(255, 0, 0, false, false).family ||
        fft_route(255, 65, 0, false, false).family)
    {
        printf("FAIL: a call outside 1..4096 taps, decimation 1..64 got a route\n");
        fails++;
    }
    printf("%ld routes checked: %s\n", routes, fails ? "FAILED" : "OK");
    return fails ? 1 : 0;
}
