// if_fir_fft_route.h — which kernel and which table image serve an overlap-save call: the named block tails with their traits, the
// routing predicates and fft_route().  Pure host arithmetic without HIP types (if_fir_kernels.h includes it for the launchers and
// the shim; tests/c/fft_route_check.cpp compiles it with a plain g++); the traits are constexpr, the kernel evaluates them too.
#pragma once
#include <stdint.h>

namespace if_fir
{

// The tail of a block after the forward transform = fir_fft_kernel's template argument CHAN (plain ints: the mangled kernel names
// carry the numbers; DEC4 = any decimating tail):
constexpr int TAIL_FULL_OR_DEC4 = 0;   // full rate (DEC4 = false; DECN: selecting store), or the decimate-by-4 tail
constexpr int TAIL_DEC4_SUB = 1;       // decimate-by-4 tail keeping every sub-th output
constexpr int TAIL_DEC2 = 2;           // decimate-by-2 tail
constexpr int TAIL_DEC2_SUB = 3;       // the same keeping every sub-th output
constexpr int TAIL_BANK4_SLOTS = 4;    // filter bank at decimation 4, channels on the fs/16 slot grid (per channel)
constexpr int TAIL_BANK4_OWN = 5;      // the same, every channel at its own centre bin
constexpr int TAIL_BANK4_OWN_SUB = 6;  // tail 5 keeping every sub-th output (decimation 12, 20, 28, ...; tails 8-general and 17 do that inside, by a wave-uniform branch)
constexpr int TAIL_BANK8_CHANNEL = 8;  // filter bank at decimation 8 per channel: slot grid (NCO = false) / any centre bin or a common offset (NCO = true)
constexpr int TAIL_BANK8_ALL = 9;      // filter bank at decimation 8, all slots of one parity from two 8-point transforms per group
constexpr int TAIL_BANK16_ALL = 16;    // filter bank at decimation 16, all 16 slots from one 16-point transform per group (NCO: a common offset)
constexpr int TAIL_BANK16_CHANNEL = 17; // filter bank at decimation 16 per channel, every channel at its own centre bin
// (round 5: compiled with single LDS reads, IF_FIR_LDS_SINGLE_READS in if_fir_fft_dev.h)

constexpr bool tail_in_dec2_units(int t) { return t == TAIL_DEC2 || t == TAIL_DEC2_SUB; } // instantiated in units of their own (csrc/Makefile)
constexpr bool tail_is_bank(int t) { return t >= TAIL_BANK4_SLOTS; }                       // filter-bank form: takes the whole ChanArgs
constexpr bool tail_single(int t) { return t >= 0 && !tail_is_bank(t); }
constexpr bool tail_valid(int t) { return tail_single(t) || (t >= TAIL_BANK4_SLOTS && t <= TAIL_BANK4_OWN_SUB) || t == TAIL_BANK8_CHANNEL || t == TAIL_BANK8_ALL || t == TAIL_BANK16_ALL || t == TAIL_BANK16_CHANNEL; }
// channels at their own centres: no common NCO on top
constexpr bool tail_own_centres(int t) { return t == TAIL_BANK4_OWN || t == TAIL_BANK4_OWN_SUB || t == TAIL_BANK16_CHANNEL; }
// has an NCO = true instantiation (the decimate-by-4 bank takes none: a single channel with an NCO is the DEC4 kernel)
constexpr bool tail_has_nco(int t) { return !tail_own_centres(t) && t != TAIL_BANK4_SLOTS; }
constexpr int tail_factor(int t, bool dec4) // the tail's own decimation F
{
    return (t == TAIL_BANK16_ALL || t == TAIL_BANK16_CHANNEL) ? 16 : (t == TAIL_BANK8_CHANNEL || t == TAIL_BANK8_ALL) ? 8 : tail_in_dec2_units(t) ? 2 : dec4 ? 4 : 1;
}
constexpr int tail_lout(int t, bool dec4, int L) { return L / tail_factor(t, dec4); } // outputs per block of L new samples (per channel)
// keeps every sub-th output of its fs/F-rate block: D = F x sub
constexpr bool tail_thins(int t) { return t == TAIL_DEC4_SUB || t == TAIL_DEC2_SUB || t == TAIL_BANK4_OWN_SUB || t == TAIL_BANK8_CHANNEL || t == TAIL_BANK16_CHANNEL; }
// twiddles in (cos, tan) form on the inputs of passes 2 and 3 and of the small inverse (round 4): the decimate-by-4 kernels (single
// channel incl. the multiples of 4) and every bank (8, 9, 16, 17: the banks' own images); the decimate-by-2 tails keep round 3's form
constexpr bool tail_wants_tan(int t, bool dec4) { return dec4 && !tail_in_dec2_units(t); }
// The `sub` word of the kernel's tail argument for a call at decimation D.  Tail 9 is the special case: it does not thin, its word
// carries what the launcher put there -- bit 0: the slot parity, bit 1: both parities in one launch over virtual blocks.
constexpr uint32_t tail_sub_word(int t, bool dec4, int D, uint32_t call_sub)
{
    return t == TAIL_BANK8_ALL ? (call_sub & 3u) : tail_thins(t) ? (uint32_t)(D / tail_factor(t, dec4)) : 1u;
}

constexpr int FFT_N = 4096;
constexpr int FFT_PART = 2048; // filters of 3074..4096 taps: two partitions of at most this many taps
constexpr int FFT_TABLE_FLOATS = 2 * (4096 + 4096 + 256 + 1024 + 1024 + 64 + 256); // ... + 64 NCO row phasors + 256 W2048 twiddles
constexpr int fft_odd_table_floats(int F) { return 2 * (F * 1024 + 256 + 768 + 1024 + 64 + 64 + 256); } // G_p | TB | TC | TWD | TWE | NCO | phasor tables (round 5)

// D = 1 and D = 4 have their own kernels; any other decimation runs the full-rate kernel with a selecting store.
// Taps: the first T-1 outputs of a 4096-point block are discarded, in whole 64-sample rows (4, 8, 16, 32 or 48 of the
// 64): up to 257 taps cost 6 % of the block, 513 taps 12.5 %, 1025 taps 25 %, 2049 taps half, 3073 taps three quarters.
inline bool fft_supported(int T, int D) { return D >= 1 && D <= 64 && T >= 1 && T <= 4096; }

// Which decimations have a decimating tail (frequency-domain alias fold + small inverse): every EVEN one, D = F * sub with F the
// tail's own decimation.  F = 4: decimation 4 and every other multiple of 4 up to 64 -- the decimate-by-4 tail keeping every
// sub-th output (round 3; measured faster than the one-channel filter-bank tails at 8 / 16 it replaced for single channels,
// profiles/r03_composite_decimations.txt).  F = 2: decimation 2, and 6, 10, ..., 62 the same way behind the decimate-by-2 tail.
// Odd decimations run the full-rate kernel with a selecting store.  Filters of 3074..4096 taps (two partitions) take the same
// tails, the second partition accumulating.  (The multi-channel front's chunk grid asks this too.)
inline bool fft_tail(int T, int D, int *pF, int *pSub)
{
    int F = 1;
    if (fft_supported(T, D))
        F = (D % 4 == 0) ? 4 : (D % 2 == 0) ? 2 : 1;
    if (pF)
        *pF = F;
    if (pSub)
        *pSub = D / F;
    return F > 1;
}

// 3074..4096 taps: two partitions of at most FFT_PART taps each, y = h_a * x + h_b * (x delayed by FFT_PART)
inline bool fft_two_partitions(int T) { return T > 3073; }

// Odd decimations divisible by 3 (round 4, fir_odd_kernel): D = F sub; a block of F x 1024 input samples gives 1024 outputs
// at the fs/F rate, the first ceil((T - 1 + F - 1) / F) of which are invalid -- dropped as 2 or 4 rows of 64 (*pOvlr).  False: no
// such tail (the full-rate pipeline + selecting store serves the pair).
inline bool fft_odd_tail(int T, int D, int *pF, int *pSub, int *pOvlr)
{
    int F = 1, ovlr = 0;
    if (D >= 3 && D <= 64 && (D & 1) && T >= 1 && !fft_two_partitions(T))
    {
        // (F = 5 -- decimation 5, 25, 35, 55 -- was written and dropped: five phase streams of 16 registers + the transforms'
        // temporaries do not fit 256 VGPRs, the compiler spilled 112 of them; those decimations keep the selecting store)
        F = (D % 3 == 0) ? 3 : 1;
        if (F > 1)
        {
            const int need = (T - 1 + F - 1 + F - 1) / F; // outputs of a block that see samples ahead of it
            // (8 dropped rows -- up to 1535 taps -- were built and measured 18 % slower than the selecting store: half of every
            // block is overlap, profiles/r04_odd_decimation.txt)
            ovlr = need <= 128 ? 2 : need <= 256 ? 4 : 0;
            if (!ovlr)
                F = 1;
        }
    }
    if (pF)
        *pF = F;
    if (pSub)
        *pSub = F > 1 ? D / F : 1;
    if (pOvlr)
        *pOvlr = ovlr;
    return F > 1;
}

// Overlap rows of the (taps, decimation) pair.  (Round 4 built and measured a 2-row kernel, L = 3968, for filters of at most 129
// taps on the full-rate pipeline -- 16 913 instead of 17 477 blocks for BASELINE configs[1]: within 1 % of the 4-row kernel on a
// stream that is not re-read from the memory-side cache, profiles/r04_two_row_overlap.txt -- and removed it again.)
inline int fft_overlap_rows(int T, int D)
{
    (void)D;
    if (fft_two_partitions(T))
        return 32; // each partition runs the 32-row kernel
    return (T - 1 <= 256) ? 4 : (T - 1 <= 512) ? 8 : (T - 1 <= 1024) ? 16 : (T - 1 <= 2048) ? 32 : 48;
}

// new input samples per block of the overlap-save kernel for this filter: streams cut at multiples of it (and of the
// decimation) give bit-identical results to the unsplit stream (the multi-channel front's chunk unit)
inline int fft_block_advance(int T, int D)
{
    int F = 1, ovlr = 0;
    if (fft_odd_tail(T, D, &F, nullptr, &ovlr))
        return F * (1024 - 64 * ovlr);
    return fft_two_partitions(T) ? FFT_N - FFT_PART : FFT_N - 64 * fft_overlap_rows(T, D);
}

// The filter bank's tail for a decimation: 4, 8, 16 themselves; channels at their own centres (`general`) also every other multiple
// of 4 up to 64 -- the largest of 16, 8, 4 that divides it, the tail then keeps every (D / F)-th output.  0: not served.
inline int fft_bank_tail(int D, bool general)
{
    if (D == 4 || D == 8 || D == 16)
        return D;
    if (!general || D < 4 || D > 64 || (D & 3))
        return 0;
    return (D % 16 == 0) ? 16 : (D % 8 == 0) ? 8 : 4;
}

// Routing of a decimation-8 filter-bank call whose channels sit on the slot grid (launch_fft_rows; one definition for the launcher and
// the CPU test): a slot parity with at least four channels, none of the call's slots listed twice, is served by ONE all-slots launch
// (pmask[parity] = its slots, else 0); `rest` = bit c set for every channel c left to the per-channel form.
inline void fft_bank8_plan(const uint32_t *slots, uint32_t count, bool all_slots_available, uint32_t pmask[2], uint32_t *rest)
{
    uint32_t seen = 0, m[2] = {0, 0};
    int npar[2] = {0, 0};
    bool dup = false;
    for (uint32_t c = 0; c < count; c++)
    {
        const uint32_t sl = slots[c] & 15u;
        dup = dup || ((seen >> sl) & 1u);
        seen |= 1u << sl;
        m[sl & 1u] |= 1u << sl;
        npar[sl & 1u]++;
    }
    *rest = 0;
    for (int par = 0; par < 2; par++)
        pmask[par] = (all_slots_available && !dup && npar[par] >= 4) ? m[par] : 0u;
    for (uint32_t c = 0; c < count; c++)
        if (!((pmask[slots[c] & 1u] >> (slots[c] & 15u)) & 1u))
            *rest |= 1u << c;
}

// ---- the route of a call: ONE decision for the launchers (which kernel) and the shim (which table image, how much history) ----
enum FftBankMode { FFT_NO_BANK = 0, FFT_BANK_SLOTS = 1, FFT_BANK_OWN_CENTRES = 2 };
enum FftFamily { FFT_FAMILY_NONE = 0, FFT_FAMILY_ODD, FFT_FAMILY_TWO_PARTITIONS, FFT_FAMILY_ROWS }; // NONE: the call is not served
enum FftImageKind
{
    FFT_IMAGE_PLAIN = 0, // H and round 3's twiddles: the decimate-by-2 tails
    FFT_IMAGE_FULL_RATE, // the full-rate pipeline's (D = 1, the selecting store), twiddles in (cos, tan) form
    FFT_IMAGE_DEC4,      // the merged table of the decimate-by-4 tails (single channel, bank at 4) in (cos, tan) form
    FFT_IMAGE_ODD,       // fir_odd_kernel's (fft_build_tables_odd)
    FFT_IMAGE_BANK8,     // the merged table of the bank at decimation 8: `parity` 0 (per-channel forms, the all-slots form's even slots), 1 (its odd slots)
    FFT_IMAGE_BANK16     // the merged table of the bank at decimation 16
};
struct FftImage
{
    int kind;     // FftImageKind
    int parity;   // FFT_IMAGE_BANK8: which of the two images (fft_build_tables builds one at a time)
    int images;   // images back to back in the context's buffer: 2 for two partitions and for FFT_IMAGE_BANK8
    int floats;   // of the whole buffer
    int nco_step; // NCO row phasors for the phase word x nco_step: per kept output (decimate-by-4, bank, odd tails) or per full-rate output
};
struct FftRoute
{
    int family;   // FftFamily
    int rows;     // overlap rows: of the 64 of a block (ROWS / TWO_PARTITIONS), of the 16 of a phase stream's block (ODD)
    int tail;     // fir_fft_kernel's CHAN with its DEC4 / DECN (0 / false / false for the odd kernel, which has no such argument);
    bool dec4;    //   a decimation-8 bank call on the slot grid may still be split between tails 8 and 9 by the launcher (fft_bank8_plan)
    bool decn;
    bool nco;     // the NCO = true instantiation (tail 8 takes it for channels off the slot grid as well: launch_fft_bank8)
    int F, sub;   // D = F x sub: the kernel's own decimation and the outputs it keeps (selecting store: 1 x D)
    int hist_need; // input samples ahead of a call's first one that its first block reads
    FftImage image;
};

inline FftRoute fft_route(int T, int D, int bank, bool nco, bool no_fold)
{
    FftRoute r{};
    if (!fft_supported(T, D) || (bank && fft_two_partitions(T)))
        return r;
    const auto image = [](int kind, int images, int nco_step) { return FftImage{kind, 0, images, images * FFT_TABLE_FLOATS, nco_step}; };
    r.sub = 1;
    if (!bank && !no_fold && fft_odd_tail(T, D, &r.F, &r.sub, &r.rows))
    {
        r.family = FFT_FAMILY_ODD;
        r.nco = nco;
        r.hist_need = r.F * 64 * r.rows;
        r.image = FftImage{FFT_IMAGE_ODD, 0, 1, fft_odd_table_floats(r.F), r.F};
        return r;
    }
    const bool two = fft_two_partitions(T);
    r.family = two ? FFT_FAMILY_TWO_PARTITIONS : FFT_FAMILY_ROWS;
    r.rows = fft_overlap_rows(T, D);
    r.hist_need = two ? 2 * FFT_PART : 64 * r.rows; // (two partitions: FFT_PART samples of delay + the 32-row overlap)
    if (bank)
    {
        const bool own = bank == FFT_BANK_OWN_CENTRES;
        const int Fb = fft_bank_tail(D, own);
        if (!Fb || (Fb == 4 && nco))
            return FftRoute{};
        r.tail = Fb == 16 ? (own ? TAIL_BANK16_CHANNEL : TAIL_BANK16_ALL) : Fb == 8 ? TAIL_BANK8_CHANNEL
                 : !own ? TAIL_BANK4_SLOTS : D == 4 ? TAIL_BANK4_OWN : TAIL_BANK4_OWN_SUB;
        r.nco = nco && tail_has_nco(r.tail);
        r.dec4 = true;
        r.image = Fb == 4 ? image(FFT_IMAGE_DEC4, 1, 4) : Fb == 8 ? image(FFT_IMAGE_BANK8, 2, 8) : image(FFT_IMAGE_BANK16, 1, 16);
    }
    else
    {
        int F = 1;
        (void)fft_tail(T, D, &F, nullptr);
        if (F == 2 && no_fold) // (development: decimation 2, 6, 10, ... through the selecting store)
            F = 1;
        r.tail = F == 4 ? (D == 4 ? TAIL_FULL_OR_DEC4 : TAIL_DEC4_SUB) : F == 2 ? (D == 2 ? TAIL_DEC2 : TAIL_DEC2_SUB) : TAIL_FULL_OR_DEC4;
        r.dec4 = F > 1;
        r.decn = F == 1 && D != 1;
        r.nco = nco;
        r.image = image(F == 4 ? FFT_IMAGE_DEC4 : F == 2 ? FFT_IMAGE_PLAIN : FFT_IMAGE_FULL_RATE, two ? 2 : 1, F == 4 ? 4 : 1);
    }
    r.F = tail_factor(r.tail, r.dec4);
    r.sub = D / r.F;
    return r;
}

} // namespace if_fir
