// if_fir_fft_launch.inc -- part of the overlap-save kernel's source (if_fir_fft.hip includes it; not a translation unit of its own).
// Launchers of the per-overlap-length units: launch_fft_t, launch_fft_form (the (int16, NCO) dispatch), launch_fft_rows (a route's instantiation), the two-partition launches.
// the kernel of an instantiation; the decimate-by-2 tails (tail_in_dec2_units) are instantiated in units of their own (-DIF_FIR_FFT_DEC2_UNIT, csrc/Makefile)
template <int OVL_ROWS, bool DEC4, bool I16, bool NCO, int CHAN, bool DECN, bool ACC>
static constexpr auto fft_kernel_of()
{
#ifdef IF_FIR_FFT_DEC2_UNIT
    static_assert(tail_in_dec2_units(CHAN), "the decimate-by-2 units hold the decimate-by-2 tails only");
#else
    static_assert(!tail_in_dec2_units(CHAN), "the decimate-by-2 tails live in the decimate-by-2 units (launch_fft_dec2_rows)");
#endif
    return &fir_fft_kernel<OVL_ROWS, DEC4, I16, NCO, CHAN, DECN, ACC>;
}
// the decimate-by-2 units' entry point (tail = TAIL_DEC2 | TAIL_DEC2_SUB); acc = the second launch of a two-partition filter (32 overlap rows only)
template <int ROWS>
hipError_t launch_fft_dec2_rows(const LaunchArgs &a, int tail, bool nco, bool acc);
template <int OVL_ROWS, bool DEC4, bool I16, bool NCO, int CHAN, bool DECN, bool ACC>
static hipError_t launch_fft_t(const LaunchArgs &a)
{
    auto kern = fft_kernel_of<OVL_ROWS, DEC4, I16, NCO, CHAN, DECN, ACC>();
    constexpr int L = FFT_N - 64 * OVL_ROWS;
    constexpr int LOUT = tail_lout(CHAN, DEC4, L);
    static DeviceSetup setup;
    int ncus = 0;
    {
        const hipError_t e = device_setup(setup, a.device, reinterpret_cast<const void *>(kern), FFT_LDS_BYTES, &ncus);
        if (e != hipSuccess)
            return e;
    }
    // DECN: the kernel runs at full rate over the N inputs (blocks, run queue, history as for D = 1) and keeps every
    // D-th output, the first one at full-rate index n0
    // (a thinning tail, e.g. decimation 4 sub behind TAIL_DEC4_SUB: the tail runs at the fs/F rate and keeps every sub-th output)
    constexpr int F = tail_factor(CHAN, DEC4); // the tail's own decimation
    ChanArgs ca = a.chan ? *a.chan : ChanArgs{};
    ca.sub = tail_sub_word(CHAN, DEC4, a.D, ca.sub);
    const bool both = CHAN == TAIL_BANK8_ALL && (ca.sub & 2u); // both slot parities in one launch: virtual blocks
    const int64_t m_rate = DECN ? a.N : CHAN == TAIL_BANK8_ALL ? a.M : (a.M - 1) * (int64_t)ca.sub + 1; // (tail 9: `sub` carries the slot parity)
    const int32_t n0_rate = DECN ? 0 : a.n0;
    const int64_t nblocks = (a.M > 0 ? (m_rate + LOUT - 1) / LOUT : 0) * (both ? 2 : 1);
    if (nblocks <= 0)
        return hipSuccess;
    const int64_t wgs_max = (a.grid_limit > 0 && a.grid_limit < ncus) ? a.grid_limit : ncus;
    // (round 5) a call of at most one block per wave of the chip is a SINGLE-ROUND launch (fft_launch_plan; the kernel's bit 131072).  Not for the
    // all-slots bank launch over virtual blocks (the two parities of a block want neighbouring waves: the second read of its rows comes from L2) and
    // not under the development switch 262144.  Diag 256 (development) switches the queue's tail phase off.
    const FftLaunchPlan plan = fft_launch_plan(nblocks, wgs_max, !both && !(a.diag & 262144),
                                               (a.diag & 256) ? 0 : Q_TAIL_MAX_ROUNDS);
    uint32_t qsel = 0;
    {
        const hipError_t e = fft_queue_select(a, &qsel);
        if (e != hipSuccess)
            return e;
    }
    chan_arg_t<CHAN> cak;
    if constexpr (tail_is_bank(CHAN))
        cak = ca;
    else
        cak.sub = ca.sub;
    hipLaunchKernelGGL(kern, dim3((unsigned)plan.wgs), dim3(512), FFT_LDS_BYTES, a.stream,
                       reinterpret_cast<const f2v *>(a.in), reinterpret_cast<f2v *>(a.out),
                       reinterpret_cast<const f2v *>(a.fft_tables), reinterpret_cast<const f2v *>(a.hist_full), a.hist_len, a.N,
                       n0_rate, m_rate, nblocks, plan.nblocks_main, (unsigned int *)a.queue,
                       (unsigned long long *)a.dbg, (int32_t)a.diag | (plan.single ? 131072 : 0),
                       DECN ? 0u - a.nco_word * a.nco_abs0 : nco_phi0(a),
                       DECN ? 0u - a.nco_word : 0u - a.nco_word * (uint32_t)F,
                       cak, qsel, a.hist_out, (int32_t)a.D, (int32_t)a.n0, a.M,
                       (int32_t)a.in_shift);
    return fft_queue_launched(a);
}

// THE (int16 input, NCO) dispatch: the two runtime booleans of a call become template arguments here and nowhere else.  FORMS states
// which NCO instantiations the call site can reach: both (by `nco`), never (tails without any: tail_has_nco) or always.
// (The units' objects list their kernels in the order of instantiation -- the order of the cases here and of the calls below.)
enum { NCO_NEVER, NCO_BOTH, NCO_ALWAYS };
template <int ROWS, bool DEC4, int CHAN, bool DECN = false, bool ACC = false, int FORMS = tail_has_nco(CHAN) ? NCO_BOTH : NCO_NEVER>
static hipError_t launch_fft_form(const LaunchArgs &a, bool nco = false)
{
    static_assert(FORMS == NCO_NEVER || tail_has_nco(CHAN), "this tail has no NCO instantiation");
    if constexpr (FORMS == NCO_BOTH)
        switch ((a.in_i16 ? 2 : 0) | (nco ? 1 : 0))
        {
        case 0: return launch_fft_t<ROWS, DEC4, false, false, CHAN, DECN, ACC>(a);
        case 1: return launch_fft_t<ROWS, DEC4, false, true, CHAN, DECN, ACC>(a);
        case 2: return launch_fft_t<ROWS, DEC4, true, false, CHAN, DECN, ACC>(a);
        default: return launch_fft_t<ROWS, DEC4, true, true, CHAN, DECN, ACC>(a);
        }
    else
        return a.in_i16 ? launch_fft_t<ROWS, DEC4, true, FORMS == NCO_ALWAYS, CHAN, DECN, ACC>(a)
                        : launch_fft_t<ROWS, DEC4, false, FORMS == NCO_ALWAYS, CHAN, DECN, ACC>(a);
}

#ifdef IF_FIR_FFT_DEC2_UNIT
template <int ROWS>
hipError_t launch_fft_dec2_rows(const LaunchArgs &a, int tail, bool nco, bool acc)
{
    const bool plain = tail == TAIL_DEC2;
    if constexpr (ROWS == 32)
        if (acc)
            return plain ? launch_fft_form<ROWS, true, TAIL_DEC2, false, true>(a, nco) : launch_fft_form<ROWS, true, TAIL_DEC2_SUB, false, true>(a, nco);
    if (acc)
        return hipErrorInvalidConfiguration;
    return plain ? launch_fft_form<ROWS, true, TAIL_DEC2>(a, nco) : launch_fft_form<ROWS, true, TAIL_DEC2_SUB>(a, nco);
}
#if defined(IF_FIR_FFT_ONLY) // (development: ONE instantiation of this unit's kernel)
__attribute__((used)) static auto *const if_fir_fft_only_kernel = &fir_fft_kernel<IF_FIR_FFT_ONLY>;
#elif defined(IF_FIR_FFT_HAZARD_PROBE) // (tests/test_host.py: one instantiation, the decimate-by-2 tail with its 16-byte stores)
template __global__ void fir_fft_kernel<IF_FIR_FFT_ROWS, true, false, false, TAIL_DEC2, false, false>(
    const f2v *, f2v *, const f2v *, const f2v *, int, int64_t, int32_t, int64_t, int64_t, int64_t, unsigned int *,
    unsigned long long *, int32_t, uint32_t, uint32_t, chan_arg_t<TAIL_DEC2>, uint32_t, void *, int32_t, int32_t, int64_t, int32_t);
#else
template hipError_t launch_fft_dec2_rows<IF_FIR_FFT_ROWS>(const LaunchArgs &a, int tail, bool nco, bool acc);
#endif
#else // ================= the units of every other tail =================
// the filter bank at decimation 8 (and behind 24, 40, 56: r.sub > 1), per channel (pairs share a small inverse) or all slots of a parity
template <int ROWS>
static hipError_t launch_fft_bank8(const LaunchArgs &a, const FftRoute &r)
{
    // slot form (chan->tw[] = W16^(a slot), a = 1..7) when every channel sits on the fs/16 grid and the context has no NCO;
    // the general form (chan->bin[] / pword[]: centre bin and mix-down word of a channel) otherwise
    bool general = a.chan->general || r.sub != 1;
    for (uint32_t c = 0; c < a.chan->count; c++)
        general = general || (a.chan->bin[c] & 255u) || a.chan->pword[c] != (a.chan->bin[c] << 20) + a.nco_word;
    if (general)
        return launch_fft_form<ROWS, true, TAIL_BANK8_CHANNEL, false, false, NCO_ALWAYS>(a);
    const bool nco = a.nco_word != 0; // channels on the slot grid shifted by the context's NCO (a common offset)
    // Channels on the slot grid.  A parity (even / odd slots) with at least four channels, none listed twice, runs the
    // ALL-SLOTS form (round 4): one launch computes the eight slots of that parity from two 8-point transforms per group
    // (2340 packed instructions a block whatever the count, against 1008 + 415 per channel) and stores the wanted ones; the
    // other channels keep the per-channel form.  Both parities qualifying: ONE launch over virtual blocks (kernel).  Up to two
    // launches per call on the context's stream; only the first one writes the next call's history.
    const ChanArgs &cin = *a.chan;
    uint32_t pmask[2], rest = 0;
    // (diag 4096, development: per-channel form only)
    fft_bank8_plan(cin.slot, cin.count, a.fft_tables_b != nullptr && !(a.diag & 4096), pmask, &rest);
    bool first = true;
    // one all-slots launch for the slots of `mask`; sub = the slot parity, or 2: both parities over virtual blocks
    const auto all_slots = [&](uint32_t mask, uint32_t sub, const void *tables) -> hipError_t {
        ChanArgs cs{};
        cs.count = (uint32_t)__builtin_popcount(mask);
        cs.sub = sub;
        cs.rot_e = cin.abs0n0 & 15u;
        cs.abs0n0 = cin.abs0n0;
        cs.mask16 = mask;
        for (uint32_t c = 0; c < cin.count; c++)
            if ((mask >> (cin.slot[c] & 15u)) & 1u)
                cs.out[cin.slot[c] & 15u] = cin.out[c];
        LaunchArgs p = a;
        p.chan = &cs;
        p.fft_tables = tables;
        if (!first)
            p.hist_out = nullptr;
        first = false;
        return launch_fft_form<ROWS, true, TAIL_BANK8_ALL>(p, nco);
    };
    if (pmask[0] && pmask[1] && !(a.diag & 8192)) // both parities: ONE launch over virtual blocks (diag 8192, development: two launches)
    {
        const hipError_t e = all_slots(pmask[0] | pmask[1], 2u, a.fft_tables);
        if (e != hipSuccess)
            return e;
        pmask[0] = pmask[1] = 0;
    }
    for (uint32_t par = 0; par < 2; par++)
        if (pmask[par]) // (even slots: the bank's own image; odd slots: the image behind it)
        {
            const hipError_t e = all_slots(pmask[par], par, par ? a.fft_tables_b : a.fft_tables);
            if (e != hipSuccess)
                return e;
        }
    ChanArgs cl{};
    for (uint32_t c = 0; c < cin.count; c++)
    {
        if (!((rest >> c) & 1u))
            continue;
        const uint32_t k = cl.count++;
        cl.slot[k] = cin.slot[c];
        for (int w = 0; w < 30; w++)
            cl.tw[k][w] = cin.tw[c][w];
        cl.rot0[k][0] = cin.rot0[c][0];
        cl.rot0[k][1] = cin.rot0[c][1];
        cl.out[k] = cin.out[c];
        cl.bin[k] = cin.bin[c];
        cl.pword[k] = cin.pword[c];
    }
    cl.abs0n0 = cin.abs0n0;
    if (!cl.count)
        return hipSuccess;
    LaunchArgs p = a;
    p.chan = &cl;
    if (!first)
        p.hist_out = nullptr;
    if (nco) // (the slot form proper has no NCO: the left-over channels of a shifted grid take the general form)
        return launch_fft_form<ROWS, true, TAIL_BANK8_CHANNEL, false, false, NCO_ALWAYS>(p);
    return launch_fft_form<ROWS, true, TAIL_BANK8_CHANNEL, false, false, NCO_NEVER>(p);
}

template <int ROWS>
hipError_t launch_fft_rows(const LaunchArgs &a, const FftRoute &r)
{
    if (a.chan)
    {
        // the filter bank: decimation 4, 8, 16; channels at their own centres (chan->general) also at every other multiple of 4 up to 64,
        // behind the tail of the largest of 16, 8, 4 that divides the decimation, keeping every sub-th output
        if (a.chan->count < 1 || a.chan->count > CHAN_MAX)
            return hipErrorInvalidConfiguration;
        switch (r.tail)
        {
        case TAIL_BANK8_CHANNEL: return launch_fft_bank8<ROWS>(a, r);
        case TAIL_BANK16_CHANNEL: return launch_fft_form<ROWS, true, TAIL_BANK16_CHANNEL>(a); // (per channel; arrays indexed by channel)
        case TAIL_BANK16_ALL: return launch_fft_form<ROWS, true, TAIL_BANK16_ALL>(a, r.nco); // chan->out[] / rot0[] are indexed by SLOT
        case TAIL_BANK4_OWN: return launch_fft_form<ROWS, true, TAIL_BANK4_OWN>(a);
        case TAIL_BANK4_OWN_SUB: return launch_fft_form<ROWS, true, TAIL_BANK4_OWN_SUB>(a); // decimation 12, 20, 28, ...
        case TAIL_BANK4_SLOTS: return launch_fft_form<ROWS, true, TAIL_BANK4_SLOTS>(a);
        default: return hipErrorInvalidConfiguration;
        }
    }
    if (tail_in_dec2_units(r.tail)) // decimation 2: frequency-domain fold + 2048-point inverse (round 3); 6, 10, ..., 62: keeping every sub-th output
        return launch_fft_dec2_rows<ROWS>(a, r.tail, r.nco, false);
    if (r.dec4 && r.tail == TAIL_FULL_OR_DEC4)
        return launch_fft_form<ROWS, true, TAIL_FULL_OR_DEC4>(a, r.nco);
    if (r.dec4) // decimation 8, 12, ..., 64: the decimate-by-4 tail keeping every sub-th output (tables as for decimation 4)
        return launch_fft_form<ROWS, true, TAIL_DEC4_SUB>(a, r.nco);
    if (!r.decn)
        return launch_fft_form<ROWS, false, TAIL_FULL_OR_DEC4>(a, r.nco);
    return launch_fft_form<ROWS, false, TAIL_FULL_OR_DEC4, true>(a, r.nco); // any other decimation: full-rate kernel + selecting store
}

#ifdef IF_FIR_FFT_ONLY // (development: ONE instantiation, e.g. -DIF_FIR_FFT_ONLY='4,true,false,false,17,false,false', to read its code)
__attribute__((used)) static auto *const if_fir_fft_only_kernel = &fir_fft_kernel<IF_FIR_FFT_ONLY>;
#else
template hipError_t launch_fft_rows<IF_FIR_FFT_ROWS>(const LaunchArgs &a, const FftRoute &r);
#endif

#if IF_FIR_FFT_ROWS == 32
// Filters of 3074..4096 taps: h = (h_a, h_b) with 2048 taps in h_a.  Launch 1: y = h_a * x (writes the history);
// launch 2: y += h_b * x(n - 2048): the same kernel with h_b's table, reading the input FFT_PART samples late and adding
// its result to what launch 1 stored (ACC).  Both are the 32-row (2049-tap) kernel; an even decimation runs behind the
// decimating tails like shorter filters do (round 3), an odd one through the selecting store.  The history holds 4096
// samples: 2048 of delay + the overlap.
template <bool ACC>
static hipError_t launch_fft_partition(const LaunchArgs &a, const FftRoute &r)
{
    if (!r.dec4 && !r.decn)
        return launch_fft_form<32, false, TAIL_FULL_OR_DEC4, false, ACC>(a, r.nco);
    if (r.dec4 && r.tail == TAIL_FULL_OR_DEC4)
        return launch_fft_form<32, true, TAIL_FULL_OR_DEC4, false, ACC>(a, r.nco);
    if (r.tail == TAIL_DEC4_SUB)
        return launch_fft_form<32, true, TAIL_DEC4_SUB, false, ACC>(a, r.nco);
    if (tail_in_dec2_units(r.tail))
        return launch_fft_dec2_rows<32>(a, r.tail, r.nco, ACC);
    return launch_fft_form<32, false, TAIL_FULL_OR_DEC4, true, ACC>(a, r.nco);
}

hipError_t launch_fft_two_partitions(const LaunchArgs &a, const FftRoute &r)
{
    if (a.chan || !a.fft_tables_b || a.hist_len < 2 * FFT_PART)
        return hipErrorInvalidConfiguration;
    LaunchArgs p = a;
    const hipError_t e = launch_fft_partition<false>(p, r);
    if (e != hipSuccess)
        return e;
    p.fft_tables = a.fft_tables_b;
    p.in_shift = FFT_PART;
    p.hist_out = nullptr; // the first launch wrote the next history
    return launch_fft_partition<true>(p, r);
}
#endif // 32-row unit
#endif // !IF_FIR_FFT_DEC2_UNIT
