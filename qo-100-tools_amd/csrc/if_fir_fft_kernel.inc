// if_fir_fft_kernel.inc -- part of the overlap-save kernel's source (if_fir_fft.hip includes it; not a translation unit of its own).
// fir_fft_kernel: load, forward transform, block queue; the tails of a block live in if_fir_fft_tails_bank.inc / _single.inc.
// CHAN names the tail of a block after the forward transform: the TAIL_* constants and their traits, if_fir_fft_route.h.
template <int OVL_ROWS, bool DEC4, bool I16, bool NCO, int CHAN, bool DECN, bool ACC>
__global__ __launch_bounds__(512, 2) IF_FIR_LDS_SINGLE_READS void fir_fft_kernel(const f2v *__restrict__ in_, f2v *__restrict__ out,
                                                        const f2v *__restrict__ tables, const f2v *__restrict__ hist,
                                                        int HL, int64_t N, int32_t n0, int64_t M, int64_t nblocks,
                                                        int64_t nblocks_main, unsigned int *queue, unsigned long long *dbg, int32_t diag,
                                                        uint32_t nco_phi0, uint32_t nco_delta, chan_arg_t<CHAN> chan,
                                                        uint32_t qsel, void *__restrict__ hist_out,
                                                        int32_t decn, int32_t decn_n0, int64_t decn_m, int32_t in_shift)
{
    // ACC (filters of 3074..4096 taps, two partitions of <= 2048 taps): this launch filters the input DELAYED by in_shift
    // samples with the second partition's table and adds its result to what the first launch stored
    // (round 3: also behind the single-channel decimating tails (tail_single), so that two-partition filters decimate in the
    // frequency domain like shorter ones)
    static_assert(!ACC || (tail_single(CHAN) && OVL_ROWS == 32), "accumulating store: single-channel pipelines, 32 overlap rows");
    static_assert(!DECN || (!DEC4 && CHAN == TAIL_FULL_OR_DEC4), "general decimation = the full-rate pipeline with a selecting store");
    static_assert(tail_valid(CHAN) && (CHAN == TAIL_FULL_OR_DEC4 || DEC4), "every named tail but the first is a decimating one");
    static_assert(tail_has_nco(CHAN) || !NCO, "channels at their own centres: no common offset on top; the decimate-by-4 bank takes no NCO either");
    // 2 overlap rows (<= 129 taps, round 4): the full-rate pipeline only -- the decimating tails drop whole 64-output rows of the
    // fs/F-rate block (OVL_ROWS / 4, / 2, ...), which 128 samples are not
    static_assert(OVL_ROWS >= 4 || (!DEC4 && !ACC), "2 overlap rows: full-rate pipeline (D = 1, odd D) only");
    // diag (development only, results are wrong when set): 1 = skip the global loads, 2 = skip the global stores
    // decimate-by-4 kernels (single channel incl. the multiples of 4, and the bank at decimation 4): twiddles in (cos, tan) form
    // on the inputs of passes 2 and 3 and of the small inverse (round 4); every other tail keeps round 3's form and tables
    constexpr bool TAN = tail_wants_tan(CHAN, DEC4);
    // the full-rate pipeline the same way, forward and inverse (the inverse's twiddles already sat on the inputs of its passes)
    constexpr bool TANF = !DEC4;
    constexpr int OVL = 64 * OVL_ROWS;
    constexpr int ISZ = I16 ? 4 : 8;       // bytes per input sample
    const char *in = reinterpret_cast<const char *>(in_);
    constexpr int L = FFT_N - OVL;         // new input samples per block
    constexpr int LOUT = tail_lout(CHAN, DEC4, L); // outputs per block (per channel)
    constexpr int EARLY_GROUPS = CHAN == TAIL_DEC4_SUB ? FFT_EARLY_GROUPS_SUB : FFT_EARLY_GROUPS; // dec4: batches of next-block loads issued during pass 3
    constexpr int LAUX = FFT_LOAD_AUX; // cache policy of the row loads
    constexpr int EDGE = OVL_ROWS; // first / last rows of a block loaded with the default policy
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63;
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // diag 512 (development: the fault path's test): the waves of workgroup 0 behave like waves whose bounded wait has expired --
    // they count a fault and leave (the whole workgroup, ahead of its barrier), their blocks stay unwritten -- and the caller
    // must be told (if_fir_synchronize)
    if ((diag & 512) && blockIdx.x == 0)
    {
        if (lane == 0)
            atomicAdd(queue + 4, 1u);
        return;
    }
    cf r[64];
    // TAIL_BANK8_ALL with both slot parities in ONE launch (chan.sub bit 1; round 4): the queue hands out VIRTUAL blocks 2 b + parity -- block b of
    // the stream is transformed twice, by neighbouring waves of a workgroup, and the second read of its rows is served by L2
    const bool both = (CHAN == TAIL_BANK8_ALL) && ((chan.sub & 2u) != 0u);
    auto rb = [&](int64_t b) -> int64_t { return (CHAN == TAIL_BANK8_ALL && both) ? (b >> 1) : b; }; // virtual block -> block of the stream
    bool loaded = false; // the rows of `blk` are already in flight (issued by the prologue or the previous iteration's epilogue)
    // ---- first block: static (wave w of workgroup b takes block w of global group b), and its rows are requested BEFORE
    //      the table copy below, so that the two transfers overlap at the head of the launch
    // (round 5) only the first wave of every SIMD (waves 0-3) requests ahead of the table copy; the second one (waves 4-7) requests its first block behind the
    // workgroup barrier like any later block.  With all eight requesting ahead the table copy queued behind 512 row loads per CU and every wave started late,
    // together: 127 taps on 2^26 samples -2.0 %, 2^24 samples -8 %, the headline -0.5 % (profiles/r05_launch_head.txt; 0, 2 or 6 waves ahead gain less).
    const bool ahead = wid < FFT_WAVES / 2;
    // (round 5) single-round launch (bit 131072, set by the LAUNCHER for calls of at most one block per wave of the chip): every wave takes at most ONE block and
    // the blocks are dealt slot-major -- block w * (workgroups) + b to wave w of workgroup b -- so that a small call spreads over all CUs, one wave per SIMD first,
    // instead of filling eight waves of a few CUs (profiles/r05_small_calls_spread.txt).  The block queue needs no switch: the launch has at most 8 x workgroups
    // blocks, so the first group a workgroup draws (global group workgroups + b) lies beyond the end and its waves leave.
    const bool single = (diag & 131072) != 0;
    int64_t blk = single ? (int64_t)wid * gridDim.x + blockIdx.x : (int64_t)blockIdx.x * FFT_WAVES + wid; // slot wid of local group 0 = global group blockIdx.x
    {
        const int64_t s0 = rb(blk) * L - OVL + n0 - in_shift;
        if (blk < nblocks && s0 >= 0 && !(diag & 1) && ahead)
        {
            const srd_t srd = make_srd(in + s0 * ISZ, (N - s0) * ISZ);
#pragma unroll
            for (int rho = 0; rho < 4; rho++)
#pragma unroll
                for (int j = 0; j < 16; j++)
                    load_row<I16, LAUX, EDGE>(r, srd, lane, 4 * j + rho);
            loaded = true;
        }
    }
    // ---- tables: global -> LDS (once per workgroup) ------------------------------------------------------------
    {
        const f4v_t *src = reinterpret_cast<const f4v_t *>(tables);
        f4v_t *dst = reinterpret_cast<f4v_t *>(smem);
        // all 11 loads of a thread in flight before the first LDS write: as a plain loop the compiler waits for each load
        // before the next one (11 memory round trips, ~8 us at the head of every launch with nothing else running on the CU)
        constexpr int NV = LDS_XB / 16, NK = (NV + 511) / 512;
        // (round 5 tried the table copy by waves 4-7 alone -- in waves 0-3 the table loads return behind the 64 row loads, a wave's loads return in order --:
        // +-0.3 %, profiles/r05_launch_head.txt)
        f4v_t tv[NK];
#pragma unroll
        for (int k = 0; k < NK; k++)
            if ((int)threadIdx.x + 512 * k < NV)
                tv[k] = src[threadIdx.x + 512 * k];
#pragma unroll
        for (int k = 0; k < NK; k++)
            if ((int)threadIdx.x + 512 * k < NV)
                dst[threadIdx.x + 512 * k] = tv[k];
        if constexpr (CHAN == TAIL_BANK16_ALL || CHAN == TAIL_BANK8_ALL)
        {
            if (threadIdx.x < 16)
                reinterpret_cast<float2 **>(smem + LDS_QPTR)[threadIdx.x] = chan.out[threadIdx.x];
        }
        if constexpr (CHAN == TAIL_BANK8_CHANNEL || tail_own_centres(CHAN))
        {
            // per channel, the phasors of output rows 0..15 of a block: row k is 32 outputs (decimation 16: 16, decimation 4: 64) = 256
            // input samples behind row 0
            if (threadIdx.x < 16u * chan.count)
            {
                const float2 w = nco_phasor(0u - chan.pword[threadIdx.x >> 4] * 256u * (threadIdx.x & 15u));
                reinterpret_cast<cf *>(smem + LDS_ROWT)[threadIdx.x] = (cf){w.x, w.y};
            }
        }
        // block queue (if_fir_fft_queue.h): the current-group word and the look-ahead ring
        if (threadIdx.x < Q_RING)
            reinterpret_cast<unsigned long long *>(smem + LDS_Q + 16)[threadIdx.x] = queue_ring_init(threadIdx.x, blockIdx.x, gridDim.x);
        if (threadIdx.x < 4)
            reinterpret_cast<unsigned int *>(smem + LDS_QCLAIM)[threadIdx.x] = 0u;
        if (threadIdx.x == 0)
        {
            *reinterpret_cast<unsigned long long *>(smem + LDS_Q) = queue_cur_init(blockIdx.x, gridDim.x, true);
            *reinterpret_cast<unsigned long long *>(smem + LDS_QTAIL) = 0ull;
            // the other global counters are the next launch's: zero them here (this launch never touches them)
            if (blockIdx.x == 0)
            {
                queue[qsel ^ 1u] = 0u;
                queue[2u + (qsel ^ 1u)] = 0u;
            }
        }
    }
    __syncthreads();
    DevQueue dq{smem + LDS_Q, smem + LDS_QTAIL, smem + LDS_QCLAIM, queue + qsel, queue + 2 + qsel, queue + 4, lane};
    const unsigned simd = (unsigned)wid & 3u; // waves w and w + 4 of a workgroup share a SIMD
    if (wid == 0)
        queue_start(dq); // the fetch the (static) slot 0 of local group 0 owes
    // streaming state: the history of the NEXT call = the last HL samples of (history || input) (HL = the block overlap,
    // >= T-1: the first block of a call then sees the very samples an interior block sees), written to the other
    // ping-pong buffer by one wave (everything it reads is read-only in this launch); spares a launch per call
    if (hist_out && blockIdx.x == 0 && wid == 0)
    {
        const int64_t keep = (int64_t)HL;
        for (int64_t i = lane; i < keep; i += 64)
        {
            const int64_t gi = N - keep + i, hi = keep + gi;
            if constexpr (I16)
            {
                const int *src = reinterpret_cast<const int *>(in_), *hsrc = reinterpret_cast<const int *>(hist);
                reinterpret_cast<int *>(hist_out)[i] = gi >= 0 ? src[gi] : (hi >= 0 ? hsrc[hi] : 0);
            }
            else
                reinterpret_cast<f2v *>(hist_out)[i] = gi >= 0 ? in_[gi] : (hi >= 0 ? hist[hi] : (f2v){0.f, 0.f});
        }
    }
    const f2v *tw1 = reinterpret_cast<const f2v *>(smem + LDS_TW1);
    const f2v *hp = reinterpret_cast<const f2v *>(smem + LDS_HP);
    const f2v *tw2 = reinterpret_cast<const f2v *>(smem + LDS_TW2);
    const f2v *twd = reinterpret_cast<const f2v *>(smem + LDS_TWD);
    const f2v *twe = reinterpret_cast<const f2v *>(smem + LDS_TWE);
    const f2v *twf = reinterpret_cast<const f2v *>(smem + LDS_TWF);  // decimate-by-2 inverse: W2048^(16 k1 + k0)
    (void)twf;
    const f2v *ncob = reinterpret_cast<const f2v *>(smem + LDS_NCO); // NCO: phasor of output row r of a block
    (void)ncob;
    const f2v *pht = reinterpret_cast<const f2v *>(smem + LDS_PH);   // phasor tables (the (cos, tan) images: lds_phasor)
    (void)pht;
    auto phasor = [&](uint32_t ph) -> float2 { // exp(+j 2 pi ph / 2^32): from the tables where the image has them
        if constexpr (TAN || TANF)
        {
            const cf w = lds_phasor(pht, ph);
            return make_float2(w.x, w.y);
        }
        else
            return nco_phasor(ph);
    };
    char *xb = smem + LDS_XB + wid * XBUF;
    const XAddr xa = DEC4 ? xaddr_xy(xb, lane) : xaddr_x(xb, lane); // the lane's exchange addresses (read bases opaque)
    (void)twd;
    (void)twe;
    // full-rate pipeline: the shared table T and this lane's three positions in it (tsw)
    const f2v *tt = reinterpret_cast<const f2v *>(smem + LDS_TT);
    const unsigned t_fwd3 = tsw(4u * ((unsigned)lane >> 4) + 16u * ((unsigned)lane & 15u)); // + i: xor (bits 0, 1 of the position)
    const unsigned t_inv1 = tsw((unsigned)lane), t_inv1s = tsw(4u * (unsigned)lane);
    (void)tt; (void)t_fwd3; (void)t_inv1; (void)t_inv1s;

    // diagnostics (only with a debug buffer): phase stamps of the first 32 iterations of a few waves
    int dbg_it = 0;
    const bool dbg_on = dbg && ((blockIdx.x & 63) == 0) && (wid < 2);
    (void)dbg_it;
    (void)dbg_on;
#ifdef IF_FIR_FFT_STAMPS
#define FFT_STAMP(slot)                                                                                          \
    do                                                                                                           \
    {                                                                                                            \
        if (dbg_on && dbg_it < 32 && lane == 0)                                                                  \
        {                                                                                                        \
            dbg[(((blockIdx.x >> 6) * 2 + wid) * 32 + dbg_it) * 8 + (slot)] = __builtin_amdgcn_s_memrealtime();   \
            dbg[4096 + (((blockIdx.x >> 6) * 2 + wid) * 32 + dbg_it) * 8 + (slot)] = __builtin_amdgcn_s_memtime(); \
        }                                                                                                        \
    } while (0)
#else
#define FFT_STAMP(slot) (void)0
#endif
    // whole-launch stamps per wave (only with a debug buffer: if_fir_debug_stamps): realtime (100 MHz) and shader clock
    unsigned long long st_r0 = 0, st_c0 = 0;
    if (dbg)
    {
        st_r0 = __builtin_amdgcn_s_memrealtime();
        st_c0 = __builtin_amdgcn_s_memtime();
    }
    // Work distribution: if_fir_fft_queue.h
    const unsigned voff = (unsigned)lane * 8u;
    while (blk < nblocks)
    {
        FFT_STAMP(0);
        const int64_t s0 = rb(blk) * L - OVL + n0 - in_shift; // stream index of the block's first sample (n0: decimation phase)
        if (!loaded && !(diag & 1))
        {
            if (s0 >= 0)
            {
                // rows beyond the end of the input read 0 through the descriptor's bounds check
                const srd_t srd = make_srd(in + s0 * ISZ, (N - s0) * ISZ);
#pragma unroll
                for (int rho = 0; rho < 4; rho++)
#pragma unroll
                    for (int j = 0; j < 16; j++)
                        load_row<I16, LAUX, EDGE>(r, srd, lane, 4 * j + rho);
            }
            else
            {
                // first block of a call: negative stream indices come from the history (or are zero); one of the two
                // loads of every element is out of range and returns 0
                // (an int16 stream keeps its history as raw int16 pairs too, so the block stays raw: OR of the two loads)
                const srd_t srd_in = make_srd(in, N * ISZ);
                const srd_t srd_h = make_srd(hist, (int64_t)HL * ISZ);
#pragma unroll
                for (int row = 0; row < 64; row++)
                {
                    const int64_t gidx = s0 + row * 64 + lane;
                    const int64_t hidx = gidx + HL;
                    const unsigned oi = (gidx >= 0) ? (unsigned)gidx * (unsigned)ISZ : 0x80000000u;
                    const unsigned oh = (gidx < 0 && hidx >= 0) ? (unsigned)hidx * (unsigned)ISZ : 0x80000000u;
                    if constexpr (I16)
                        r[row].x = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(srd_in, oi, 0, 0) |
                                                   __builtin_amdgcn_raw_buffer_load_b32(srd_h, oh, 0, 0));
                    else
                        r[row] = buf_load(srd_in, oi, 0) + buf_load(srd_h, oh, 0);
                }
            }
            // (round 5) This path -- a wave's first block, or a block behind a queue miss -- joins the steady-state path, where the rows
            // were requested a block ago, right in front of pass 1.  The compiler's wait insertion merges the two paths' pending
            // loads and stores conservatively: with 64 loads just issued here its pass-1 wait came out as vmcnt(3), which in the
            // STEADY state means "wait for 12 of the previous block's 15 stores" -- a write round trip exposed per block.  With this
            // path drained here (a few times per wave and launch) the join inherits the steady state's precise counts.
            __builtin_amdgcn_s_waitcnt(0x0f70); // vmcnt(0)
        }

        FFT_STAMP(1);
        // ---- forward ------------------------------------------------------------------------------------------
#pragma unroll
        for (int rho = 0; rho < 4; rho++)
        {
            cf t[16], w1[15];
            if constexpr (!(TAN || TANF))
                lds_fetch<15, 64>(w1, tw1 + (rho * 16 + 1) * 64 + lane); // (round 5: the 15 twiddles requested ahead of the transform)
#pragma unroll
            for (int j = 0; j < 16; j++)
                t[j] = I16 ? cvt_i16(__float_as_uint(r[4 * j + rho].x)) : r[4 * j + rho];
            fft16<false>(t);
#pragma unroll
            for (int j = 0; j < 16; j++)
            {
                if (j == 0 || TAN || TANF) // (the twiddle W4096^((lane + 64 rho) k0) is applied on the inputs of passes 2 and 3)
                    r[4 * j + rho] = t[j];
                else
                {
                    r[4 * j + rho] = cmul_v<false>(t[j], w1[j - 1]);
                }
            }
        }
        FFT_STAMP(2);
        exchange1_fwd(r);
#pragma unroll
        for (int i = 0; i < 4; i++)
        {
            cf t[16];
#pragma unroll
            for (int j = 0; j < 16; j++)
                t[j] = r[phys(i, j)];
            if constexpr (TAN || TANF)
            {
                // inputs carry W256^(n1 k0), k0 = 4 (lane / 16) + i: the part of pass 1's twiddle that depends on n1; the rest,
                // W4096^(n2 k0), joins this pass's own W256^(n2 k1) on the inputs of pass 3
                fft16_tw<false, 4>(t, tw2 + i * 60 + (lane >> 4));
#pragma unroll
                for (int j = 0; j < 16; j++)
                    r[phys(i, j)] = t[j];
            }
            else
            {
            cf w2[15];
            lds_fetch<15, 16>(w2, tw2 + 16 + (lane & 15)); // (round 5: requested ahead of the transform)
            fft16<false>(t);
#pragma unroll
            for (int j = 0; j < 16; j++)
            {
                if (j == 0)
                    r[phys(i, j)] = t[j];
                else
                {
                    r[phys(i, j)] = cmul_v<false>(t[j], w2[j - 1]);
                }
            }
            }
        }
        FFT_STAMP(3);
        exchange2(r, xa);
        FFT_STAMP(4);
        // taken here: the block's own rows have all landed and the next block's are not issued yet, so the wait
        // behind the (rare) global atomic inside drains nothing
        // (Round 4 tried an "end game": during the launch's last one or two groups per workgroup the take was deferred until the
        // current block was stored, so that no wave holds one and a half blocks while another leaves empty-handed.  Measured
        // -0.4 % on 2^26 samples with one buffer, +0.1..0.5 % on rotating buffers and on 2^28-sample launches: removed,
        // profiles/r04_end_game.txt.)
        const int64_t blk_next = queue_take(dq, simd, nblocks_main, nblocks);
        const int64_t s0n = rb(blk_next) * L - OVL + n0 - in_shift;
        const bool next_fast = (blk_next < nblocks) && (s0n >= 0) && !(diag & 1);
        const srd_t nsrd = make_srd(in + (next_fast ? s0n : 0) * ISZ, next_fast ? (N - s0n) * ISZ : 0);
        // outputs beyond M are dropped by the descriptor's bounds check
        const int64_t obase = rb(blk) * LOUT;
        const srd_t osrd = make_srd(out + obase, (diag & 2) ? 0 : (M - obase) * 8);
        // filter-bank tails with an NCO: the block's share of the output rotation, phasor(phi0 + delta obase), wave-uniform;
        // parked in a per-wave LDS word until the tails need it (the 16-slot tail has neither SGPRs nor VGPRs to spare)
        if constexpr (NCO && (CHAN == TAIL_BANK16_ALL || CHAN == TAIL_BANK8_ALL))
        {
            const float2 pb = phasor(nco_phi0 + nco_delta * (uint32_t)obase);
            if (lane == 0)
                *reinterpret_cast<cf *>(smem + LDS_QNCO + wid * 8) = (cf){pb.x, pb.y};
        }
        // ---- the tail of the block, by family (textual includes: one kernel body, the families in their own files) ----
        if constexpr (tail_is_bank(CHAN))
        {
#include "if_fir_fft_tails_bank.inc"
        }
        else
        {
#include "if_fir_fft_tails_single.inc"
        }
        FFT_STAMP(7);
        dbg_it++;
        loaded = next_fast;
        blk = blk_next;
    }
#ifndef IF_FIR_FFT_STAMPS
    if (dbg && lane == 0)
    {
        unsigned long long *d = dbg + 4 * ((size_t)blockIdx.x * FFT_WAVES + wid);
        d[0] = st_r0;
        d[1] = __builtin_amdgcn_s_memrealtime();
        d[2] = st_c0;
        d[3] = __builtin_amdgcn_s_memtime();
    }
#endif
}

