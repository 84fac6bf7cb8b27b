// if_fir_fft_tails_bank.inc -- part of the overlap-save kernel's source (if_fir_fft.hip includes it; not a translation unit of its own).
// Filter-bank tails of fir_fft_kernel (tail_is_bank: TAIL_BANK16_ALL, 16_CHANNEL, 8_ALL, 8_CHANNEL, 4_SLOTS, 4_OWN, 4_OWN_SUB = CHAN 16, 17, 9, 8, 4, 5, 6): included INSIDE the kernel body, behind the forward transform.
        if constexpr (CHAN == TAIL_BANK16_ALL)
        {
            // ---- 16-slot filter bank at the channel rate (decimation 16, round 3; tools/fft_model.py bank16) --------------
            // Channel s = the prototype moved up by s/16 cycles/sample; decimating by 16 aliases every slot centre to DC.
            // Folded spectrum of ALL 16 slots from one 16-point transform per group:
            //   Z_s(k0, k1) = sum_k2 H((k2 - s) mod 16) Y(k2) = FFT16(t * G0)[s],  G0[n2] = sum_k2 H(k2) W16^(n2 k2) (host table)
            // (round 4: the forward passes in (cos, tan) form; the b^n2 the inputs of this pass still carry is folded into the table)
#pragma unroll
            for (int i = 0; i < 4; i++)
            {
                cf t[16], hq[16];
                lds_fetch<16, 64>(hq, hp + (i * 16) * 64 + lane); // (round 5: the group's 16 table entries requested together, ahead of the products)
#pragma unroll
                for (int j = 0; j < 16; j++)
                    t[j] = cmul_v<false>(r[phys(i, j)], hq[j]);
                fft16<false>(t);
#pragma unroll
                for (int j = 0; j < 16; j++)
                    r[phys(i, j)] = t[j]; // slot (i, s = j)
            }
            // 256-point inverses, four slots at a time (cs = slot % 4 takes the place of mu2 in the 1024-point inverse):
            // lane = 4 mu1 + cs, slot mu0 -> y_s[16 mu0 + mu1], s = 4 b + cs; each lane stores to ITS channel's buffer
            constexpr int MU0_FIRST = OVL_ROWS / 4;
            constexpr int EARLY_B = I16 ? 3 : 1; // batches whose next-block rows are requested ahead of their inverse (no scratch)
            const int cs = lane & 3, mu1 = lane >> 2;
            // NCO (the context's NCO = a common fine offset of the whole slot grid):
            // output m = obase + 16 (mu0 - first) + mu1 is rotated by phasor(phi0 + delta m) = A(lane) * B(mu0 - first), B from
            // the table (step 16 delta, fft_build_tables)
            // with A(lane) = [phasor(phi0 + delta obase), wave-uniform, in SGPRs] * [phasor(delta mu1), table entries 32..47]
#pragma unroll
            for (int b = 0; b < 4; b++)
            {
                // a batch none of whose four slots is wanted is
                // not inverted; its registers are refilled with next-block rows all the same
                const bool wanted = ((chan.mask16 >> (4 * b)) & 15u) != 0u;
                cf a[16];
#pragma unroll
                for (int i = 0; i < 4; i++)
#pragma unroll
                    for (int q = 0; q < 4; q++)
                        a[4 * i + q] = r[phys(i, 4 * b + q)];
                // these 16 registers are dead: refill them with rows of the next block (the last batch after its inverse,
                // to keep the temporaries out of scratch)
                if (b < EARLY_B && next_fast)
                {
#pragma unroll
                    for (int i = 0; i < 4; i++)
#pragma unroll
                        for (int q = 0; q < 4; q++)
                            load_row<I16, LAUX, EDGE>(r, nsrd, lane, phys(i, 4 * b + q));
                }
                if (wanted)
                {
                    cf c[16];
                    inverse_tail256_tan<false>(a, c, twe, xa, lane); // (no registers for the table prefetch here)
                    // this lane's channel: its buffer (pointer table in LDS) and the call-constant mix-down phase
                    // exp(-j 2 pi s (abs0 + n0) / 16) = W16^(s rot_e) (table entries 16..31: the 16th roots of unity)
                    float2 *po = reinterpret_cast<float2 *const *>(smem + LDS_QPTR)[4 * b + cs];
                    cf wl = ncob[16 + (((4 * b + cs) * (int)chan.rot_e) & 15)];
                    if constexpr (NCO)
                        wl = cmul_v<false>(cmul_v<false>(wl, *reinterpret_cast<const cf *>(smem + LDS_QNCO + wid * 8)), ncob[32 + mu1]);
                    const int64_t o0 = obase + mu1;
                    cf nb[16 - MU0_FIRST];
                    if constexpr (NCO)
                        lds_fetch<16 - MU0_FIRST, 1>(nb, ncob); // (round 5: the NCO's row phasors requested together, ahead of the store loop)
                    if (po != nullptr && !(diag & 2))
                        store_lane_rows<16 - MU0_FIRST, 16>(reinterpret_cast<cf *>(po) + o0, obase + LOUT <= M, o0, M, [&](int k) {
                            if constexpr (NCO)
                                return cmul_v<false>(c[MU0_FIRST + k], cmul_v<false>(wl, nb[k]));
                            else
                                return cmul_v<false>(c[MU0_FIRST + k], wl);
                        });
                }
                if (b >= EARLY_B && next_fast)
                {
#pragma unroll
                    for (int i = 0; i < 4; i++)
#pragma unroll
                        for (int q = 0; q < 4; q++)
                            load_row<I16, LAUX, EDGE>(r, nsrd, lane, phys(i, 4 * b + q));
                }
            }
        }
        else if constexpr (CHAN == TAIL_BANK16_CHANNEL)
        {
            // ---- filter bank at decimation 16, every channel at its own centre bin (round 4; the decimation-8 general form below at
            // the channel rate).  Centre bin B = 256 s + b: H_c(k) = H(k - B); with k = k_low + 256 k2 and k_low - b = kappa - 256 cy
            //   Z_c(k_low) = sum_n2 t[n2] W16^(n2 s') G0^kappa[n2],  s' = s + cy,  G0[n2] = sum_k2 H(k_low + 256 k2) W16^(n2 k2)
            // (t = the inputs of pass 3, G0 = the 16-slot bank's table, gathered from the lane that holds kappa); 256-point inverses,
            // four channels at a time: lane = 4 mu1 + ch, slot mu0 -> y_ch[16 mu0 + mu1].  The inputs still carry b_klow^n2 ((cos, tan)
            // forward passes); the gathered entry carries b_kappa^n2, and b_klow^n2 W16^(n2 s') = b_kappa^n2 W4096^(n2 B): the factor
            // beside the entry is wave-uniform (host, chan.tw, SGPRs), as in the decimation-8 general form.
            constexpr int MU0_FIRST = OVL_ROWS / 4;
            const int nch = (int)chan.count;
            const int lq = (lane >> 4) + 4 * (lane & 15); // k_low >> 2
            const f2v *rowt = reinterpret_cast<const f2v *>(smem + LDS_ROWT);
            for (int cq = 0; cq < nch; cq += 4)
            {
                const bool last = cq + 4 >= nch; // the inputs of pass 3 die with the last four channels: refill with the next block
                cf a[16];
                // (round 5: channel by channel, its 15 twiddles loaded once and in SGPRs before its first table gather; per group the
                // 16 gathers fly under the 15 products t[n2] W4096^(n2 B): gather_mac)
#pragma unroll
                for (int ch = 0; ch < 4; ch++)
                {
                    if (cq + ch >= nch) // fewer than four: empty quarters
                    {
#pragma unroll
                        for (int i = 0; i < 4; i++)
                            a[4 * i + ch] = (cf){0.f, 0.f};
                        continue;
                    }
                    const int cb = (int)chan.bin[cq + ch], b = cb & 255; // wave-uniform (the slot s = cb >> 8 is absorbed: see above)
                    cf tw[15];
#pragma unroll
                    for (int n2 = 1; n2 < 16; n2++)
                        tw[n2 - 1] = (cf){chan.tw[cq + ch][2 * (n2 - 1)], chan.tw[cq + ch][2 * (n2 - 1) + 1]}; // W4096^(n2 B)
                    // the lane that holds kappa: (k_low - b) >> 2 = lq - (b >> 2), one less in the groups below b % 4 (a borrow) -- two
                    // lanes per channel, picked per group by a wave-uniform test (round 4 recomputed them per group)
                    const int lk0 = (lq - (b >> 2)) & 63, lk1 = (lk0 - 1) & 63;
                    const int lane_k0 = ((lk0 & 3) << 4) | (lk0 >> 2), lane_k1 = ((lk1 & 3) << 4) | (lk1 >> 2);
#pragma unroll
                    for (int i = 0; i < 4; i++)
                    {
                        const int ik = (i - b) & 3;                            // table group of kappa (kappa % 4)
                        const int lane_k = (i < (b & 3)) ? lane_k1 : lane_k0;
                        cf t[16];
#pragma unroll
                        for (int n2 = 0; n2 < 16; n2++)
                            t[n2] = r[phys(i, n2)];
                        a[4 * i + ch] = gather_mac<16, 64>(t, tw, hp + (ik * 16) * 64 + lane_k);
                    }
                }
                if (last && next_fast)
                {
#pragma unroll
                    for (int i = 0; i < EARLY_GROUPS; i++)
#pragma unroll
                        for (int j = 0; j < 16; j++)
                            load_row<I16, LAUX, EDGE>(r, nsrd, lane, phys(i, j));
                }
                cf c[16];
                inverse_tail256_tan(a, c, twe, xa, lane);
                if (last && next_fast)
                {
#pragma unroll
                    for (int i = EARLY_GROUPS; i < 4; i++)
#pragma unroll
                        for (int j = 0; j < 16; j++)
                            load_row<I16, LAUX, EDGE>(r, nsrd, lane, phys(i, j));
                }
                // mix-down: output o = obase + 16 (mu0 - first) + mu1 of the call belongs to input sample abs0n0 + 16 o: a lane factor
                // (exact 32-bit phase) times the channel's row phasor (256 input samples per row)
                const int cs = lane & 3, mu1 = lane >> 2;
                const int cl = (cq + cs < nch) ? cq + cs : nch - 1;
                const int c1 = (cq + 1 < nch) ? cq + 1 : nch - 1, c2 = (cq + 2 < nch) ? cq + 2 : nch - 1, c3 = (cq + 3 < nch) ? cq + 3 : nch - 1;
                float2 *po = cs == 0 ? chan.out[cq] : cs == 1 ? chan.out[c1] : cs == 2 ? chan.out[c2] : chan.out[c3];
                const uint32_t pw = cs == 0 ? chan.pword[cq] : cs == 1 ? chan.pword[c1] : cs == 2 ? chan.pword[c2] : chan.pword[c3];
                const int64_t o0 = obase + mu1;
                const float2 pa = phasor(0u - pw * (chan.abs0n0 + 16u * (uint32_t)o0));
                const cf wl = {pa.x, pa.y};
                const f2v *rowp_t = rowt + cl * 16;
                cf rowp[16 - MU0_FIRST];
                lds_fetch<16 - MU0_FIRST, 1>(rowp, rowp_t); // (round 5: the channel's row phasors requested together, ahead of the store loop)
                // decimation 32, 48, 64 (16 x sub): every sub-th output of this tail is a real output (KeepEvery, as behind the
                // single-channel tails; sub = 1: all of them)
                if (chan.sub == 1u) // (wave-uniform: the plain decimation keeps its plain store loop -- the thinning costs it 5 %)
                {
                    if (cq + cs < nch && !(diag & 2))
                        store_lane_rows<16 - MU0_FIRST, 16>(reinterpret_cast<cf *>(po) + o0, obase + LOUT <= M, o0, M, [&](int k) {
                            return cmul_v<false>(c[MU0_FIRST + k], cmul_v<false>(wl, rowp[k]));
                        });
                }
                else if ((chan.sub & (chan.sub - 1u)) == 0u && chan.sub <= 16u)
                {
                    // decimation 32, 64 (sub = 2, 4 divides the 16 outputs of a row): a lane keeps all of its outputs or none, and the
                    // kept ones are 16 / sub apart -- the plain store loop with another step (round 5)
                    KeepEvery ke;
                    ke.init(blk, (unsigned)LOUT, chan.sub);
                    const int64_t kept0 = ke.index((unsigned)mu1); // of the lane's first output, or -1
                    if (cq + cs < nch && !(diag & 2) && kept0 >= 0)
                    {
                        cf *pl = reinterpret_cast<cf *>(po) + kept0;
                        const unsigned step = 16u / chan.sub;
                        const bool full = obase + LOUT <= M;
#pragma unroll
                        for (int mu0 = MU0_FIRST; mu0 < 16; mu0++)
                        {
                            const cf v = cmul_v<false>(c[mu0], cmul_v<false>(wl, rowp[mu0 - MU0_FIRST]));
                            if (full || o0 + 16 * (mu0 - MU0_FIRST) < M)
                                __builtin_nontemporal_store(v, pl);
                            pl += step;
                        }
                    }
                }
                else
                {
                    KeepEvery ke;
                    ke.init(blk, (unsigned)LOUT, chan.sub);
                    if (cq + cs < nch && !(diag & 2))
                    {
#pragma unroll
                        for (int mu0 = MU0_FIRST; mu0 < 16; mu0++)
                        {
                            const int64_t idx = o0 + 16 * (mu0 - MU0_FIRST);
                            const int64_t kept = ke.index((unsigned)mu1 + 16u * (unsigned)(mu0 - MU0_FIRST));
                            const cf v = cmul_v<false>(c[mu0], cmul_v<false>(wl, rowp[mu0 - MU0_FIRST]));
                            if (idx < M && kept >= 0)
                                __builtin_nontemporal_store(v, reinterpret_cast<cf *>(po) + kept);
                        }
                    }
                }
            }
        }
        else if constexpr (CHAN == TAIL_BANK8_ALL)
        {
            // ---- filter bank at decimation 8, ALL SLOTS OF ONE PARITY (round 4, VERDICT r3 #2; tools/fft_model.py bank8_parity) ----
            // Z_s(k2') = sum_a w_{k2'}[a] W16^(a s) G_q[a], q = (k2' - s) mod 2 (the per-channel form above).  For the slots of one parity,
            // s = 2 sigma + par, W16^(a s) = W16^(a par) W8^(a sigma): with the factor W16^(a par) in the table (a second image for
            // the odd slots, fft_build_tables bank_parity)
            //     Z_s(0) = FFT8( w0 . G_par )[sigma],      Z_s(1) = FFT8( w1 . G_(1 - par) )[sigma]
            // -- w0 and w1 are used ONCE each, so the 64 registers of the block turn into the 64 values Z_s(k2') (8 slots x 2 x 4 groups)
            // in place.  (All 16 slots at once would need 128 live values: the other parity is a second launch.)  16 multiplies
            // and two 8-point transforms per group serve eight channels: 88 packed instructions where the per-channel form spends
            // 8 x 60.  The inverses follow two slots at a time exactly as in the per-channel form; every lane stores to its slot's
            // buffer (pointer table in LDS, as in the 16-slot bank); slots nobody asked for are not inverted.
            // (the launcher passes the parity in `sub`; both parities in one launch: the virtual block's low bit -- then the ODD slots
            // take the even slots' image with the halves exchanged and the eight constants W16^a on top, so one image serves both)
            const int par = both ? (int)(blk & 1) : ((int)chan.sub & 1);
            const bool swap = both && par;
            const int h0 = swap ? 8 : 0, h1 = swap ? 0 : 8;
#pragma unroll
            for (int i = 0; i < 4; i++)
            {
                cf t0[8], t1[8];
                // (cos, tan) form: the inputs of this pass still carry b^n2, b = W4096^(k0 + 16 k1) (passes 1 and 2 as in the
                // decimate-by-4 kernels).  t[a] b^a +- t[a + 8] b^(a + 8) = b^a (t[a] +- b^8 t[a + 8]): b^a sits in the table image,
                // b^8 = c (1 + j t) is the second of the three first-stage entries of pass 3 -- 3 packed FMAs per pair
                const cf e8 = tw1[(i * 3 + 1) * 64 + lane];
                cf hq[16];
                lds_fetch<16, 64>(hq, hp + (i * 16) * 64 + lane); // (round 5: the group's 16 table entries requested together, ahead of the products)
#pragma unroll
                for (int a8 = 0; a8 < 8; a8++)
                {
                    const cf u = r[phys(i, a8)], vb = tw_u<false>(r[phys(i, a8 + 8)], e8);
                    t0[a8] = cmul_v<false>(tw_ac<false>(u, vb, e8), swap ? hq[8 + a8] : hq[a8]); // w0 . (b^a G_par W16^(a par)): first half of the image
                    t1[a8] = cmul_v<false>(tw_ac<true>(u, vb, e8), swap ? hq[a8] : hq[8 + a8]);  // w1 . (b^a G_(1 - par) W16^(a par)): second half
                }
                if (swap) // (wave-uniform) W16^a, a = 1..7
                {
                    constexpr float C1 = 0.92387953251128674f, S1 = 0.38268343236508977f, R = 0.70710678118654752f;
                    t0[1] = cmul_s<false>(t0[1], (cf){C1, -S1}); t1[1] = cmul_s<false>(t1[1], (cf){C1, -S1});
                    t0[2] = cmul_s<false>(t0[2], (cf){R, -R});   t1[2] = cmul_s<false>(t1[2], (cf){R, -R});
                    t0[3] = cmul_s<false>(t0[3], (cf){S1, -C1}); t1[3] = cmul_s<false>(t1[3], (cf){S1, -C1});
                    t0[4] = (cf){t0[4].y, -t0[4].x};             t1[4] = (cf){t1[4].y, -t1[4].x}; // -j
                    t0[5] = cmul_s<false>(t0[5], (cf){-S1, -C1}); t1[5] = cmul_s<false>(t1[5], (cf){-S1, -C1});
                    t0[6] = cmul_s<false>(t0[6], (cf){-R, -R});  t1[6] = cmul_s<false>(t1[6], (cf){-R, -R});
                    t0[7] = cmul_s<false>(t0[7], (cf){-C1, -S1}); t1[7] = cmul_s<false>(t1[7], (cf){-C1, -S1});
                }
                fft8<false>(t0);
                fft8<false>(t1);
#pragma unroll
                for (int sg = 0; sg < 8; sg++)
                {
                    r[phys(i, sg)] = t0[sg];     // Z_s(0), s = 2 sg + par
                    r[phys(i, sg + 8)] = t1[sg]; // Z_s(1)
                }
            }
            constexpr int MU0_FIRST = OVL_ROWS / 4;
            constexpr int EARLY_B = I16 ? 3 : 1; // batches whose next-block rows are requested ahead of their inverse (no scratch)
#pragma unroll
            for (int b = 0; b < 4; b++)
            {
                // slots of this batch: sigma = 2 b, 2 b + 1
                const unsigned want = (chan.mask16 >> (2 * (2 * b) + par)) & 1u, want1 = (chan.mask16 >> (2 * (2 * b + 1) + par)) & 1u;
                const bool wanted = (want | want1) != 0u;
                cf a[16];
#pragma unroll
                for (int i = 0; i < 4; i++)
#pragma unroll
                    for (int ch = 0; ch < 2; ch++)
                    {
                        const cf z0 = r[phys(i, 2 * b + ch)], z1 = r[phys(i, 8 + 2 * b + ch)];
                        a[4 * i + 2 * ch] = z0 + z1;
                        a[4 * i + 2 * ch + 1] = cmul_v<true>(z0 - z1, twd[(i * 4 + 2) * 64 + lane]); // conj W512^(16 k1 + k0)
                    }
                auto refill = [&]() {
#pragma unroll
                    for (int i = 0; i < 4; i++)
#pragma unroll
                        for (int ch = 0; ch < 2; ch++)
                        {
                            load_row<I16, LAUX, EDGE>(r, nsrd, lane, phys(i, 2 * b + ch));
                            load_row<I16, LAUX, EDGE>(r, nsrd, lane, phys(i, 8 + 2 * b + ch));
                        }
                };
                if (b < EARLY_B && next_fast)
                    refill();
                if (wanted)
                {
                    cf c[16];
                    inverse_tail256_tan<false>(a, c, twe, xa, lane); // (no registers for the table prefetch here)
                    // lane = 4 mu1 + 2 ch + mu2, slot mu0 -> y_s[32 mu0 + 2 mu1 + mu2], s = 2 (2 b + ch) + par.  Mix-down: the call
                    // constant W16^(s rot_e) (16th roots: table entries 16..31) times (-1)^(s m), m = obase + 32 (..) + 2 mu1 + mu2
                    // with obase even: the sign is (-1)^(s mu2)
                    const int sl = 2 * (2 * b + ((lane >> 1) & 1)) + par;
                    float2 *po = reinterpret_cast<float2 *const *>(smem + LDS_QPTR)[sl];
                    cf wl = ncob[16 + ((sl * (int)chan.rot_e) & 15)];
                    if ((sl & lane) & 1)
                        wl = (cf){-wl.x, -wl.y};
                    // NCO (the context's NCO = a common fine offset of the whole slot grid, as in the 16-slot tail): output m = obase +
                    // 32 (mu0 - first) + 2 mu1 + mu2 is also rotated by phasor(phi0 + delta m) = [block, per-wave LDS word] * [lane:
                    // table entries 32..63] * [row: entries 0..15]
                    if constexpr (NCO)
                        wl = cmul_v<false>(cmul_v<false>(wl, *reinterpret_cast<const cf *>(smem + LDS_QNCO + wid * 8)),
                                           ncob[32 + 2 * (lane >> 2) + (lane & 1)]);
                    const int64_t o0 = obase + 2 * (lane >> 2) + (lane & 1);
                    cf nb[16 - MU0_FIRST];
                    if constexpr (NCO)
                        lds_fetch<16 - MU0_FIRST, 1>(nb, ncob); // (round 5: the NCO's row phasors requested together, ahead of the store loop)
                    if (po != nullptr && !(diag & 2))
                        store_lane_rows<16 - MU0_FIRST, 32>(reinterpret_cast<cf *>(po) + o0, obase + LOUT <= M, o0, M, [&](int k) {
                            if constexpr (NCO)
                                return cmul_v<false>(c[MU0_FIRST + k], cmul_v<false>(wl, nb[k]));
                            else
                                return cmul_v<false>(c[MU0_FIRST + k], wl);
                        });
                }
                if (b >= EARLY_B && next_fast)
                    refill();
            }
        }
        else if constexpr (CHAN == TAIL_BANK8_CHANNEL)
        {
            // ---- filter bank at decimation 8 (fs/16 slots, 2x oversampled channels; tools/fft_model.py bank8) ------------
            // First radix-2 stage of pass 3 once, in place: r[phys(i, a)] = w0[a] = t[a] + t[a+8], r[phys(i, a+8)] = w1[a].
            // Channel at slot s:  Z_s(k2') = sum_a w_{k2'}[a] W16^(a s) G_q[a],  q = (k2' - s) mod 2 (host table G, kernel
            // arguments W16^(a s)); 512-point inverse, two channels per small inverse (low = 2 ch + mu2):
            // lane = 4 mu1 + 2 ch + mu2, slot mu0 -> y_ch[32 mu0 + 2 mu1 + mu2]
            // (cos, tan) form (round 4): the inputs of this pass still carry b^n2, b = W4096^(k0 + 16 k1);
            // t[a] b^a +- t[a + 8] b^(a + 8) = b^a (t[a] +- b^8 t[a + 8]): b^8 = c (1 + j t) is applied here (three packed FMAs a pair), b^a is
            // folded into the table for the lane that OWNS the entry (see the general form below for lanes that read another lane's)
            static_assert(CHAN != TAIL_BANK8_CHANNEL || TAN, "the decimation-8 bank is written for its (cos, tan) image");
#pragma unroll
            for (int i = 0; i < 4; i++)
            {
                const cf e8 = tw1[(i * 3 + 1) * 64 + lane];
#pragma unroll
                for (int a8 = 0; a8 < 8; a8++)
                {
                    const cf u = r[phys(i, a8)], vb = tw_u<false>(r[phys(i, a8 + 8)], e8);
                    r[phys(i, a8)] = tw_ac<false>(u, vb, e8);
                    r[phys(i, a8 + 8)] = tw_ac<true>(u, vb, e8);
                }
            }
            constexpr int MU0_FIRST = OVL_ROWS / 4;
            const int nch = (int)chan.count;
            if constexpr (!NCO)
            {
            // ---- channels on the fs/16 slot grid, no NCO on the context (round 3's form: slot twiddles in SGPRs, the mix-down a sign)
            for (int cp = 0; cp < nch; cp += 2)
            {
                const bool last = cp + 2 >= nch; // the w values die with the last pair: refill with the next block
                cf a[16];
#pragma unroll
                for (int ch = 0; ch < 2; ch++)
                {
                    if (ch == 1 && cp + 1 >= nch) // odd count: an empty second half
                    {
#pragma unroll
                        for (int i = 0; i < 4; i++)
                        {
                            a[4 * i + 2] = (cf){0.f, 0.f};
                            a[4 * i + 3] = (cf){0.f, 0.f};
                        }
                        continue;
                    }
                    const int c = cp + ch;
                    const int par = (int)chan.slot[c] & 1;
                    cf tw[7];
#pragma unroll
                    for (int a8 = 1; a8 < 8; a8++)
                        tw[a8 - 1] = (cf){chan.tw[c][2 * (a8 - 1)], chan.tw[c][2 * (a8 - 1) + 1]}; // W16^(a slot)
#pragma unroll
                    for (int i = 0; i < 4; i++)
                    {
                        const f2v *g0 = hp + (i * 16 + 8 * par) * 64 + lane;       // k2' = 0: q = s & 1       (+ a * 64 entries)
                        const f2v *g1 = hp + (i * 16 + 8 * (1 - par)) * 64 + lane; // k2' = 1: q = (1 - s) & 1
                        cf t0[8], t1[8];
#pragma unroll
                        for (int a8 = 0; a8 < 8; a8++)
                        {
                            t0[a8] = r[phys(i, a8)];
                            t1[a8] = r[phys(i, a8 + 8)];
                        }
                        const cf z0 = gather_mac<8, 64>(t0, tw, g0); // (round 5: table reads ahead of the products)
                        const cf z1 = gather_mac<8, 64>(t1, tw, g1);
                        a[4 * i + 2 * ch] = z0 + z1;
                        a[4 * i + 2 * ch + 1] = cmul_v<true>(z0 - z1, twd[(i * 4 + 2) * 64 + lane]); // conj W512^(16 k1 + k0)
                    }
                }
                if (last && next_fast)
                {
#pragma unroll
                    for (int i = 0; i < EARLY_GROUPS; i++)
#pragma unroll
                        for (int j = 0; j < 16; j++)
                            load_row<I16, LAUX, EDGE>(r, nsrd, lane, phys(i, j));
                }
                cf c[16];
                inverse_tail256_tan(a, c, twe, xa, lane);
                if (last && next_fast)
                {
#pragma unroll
                    for (int i = EARLY_GROUPS; i < 4; i++)
#pragma unroll
                        for (int j = 0; j < 16; j++)
                            load_row<I16, LAUX, EDGE>(r, nsrd, lane, phys(i, j));
                }
                // mix-down: exp(-j 2 pi s a / 16), a = abs0 + n0 + 8 m: the call constant rot0 times (-1)^(s m); m = obase +
                // 32 (mu0 - first) + 2 mu1 + mu2 with obase even, so the sign is (-1)^(s mu2)
                const int chl = (lane >> 1) & 1, cl = cp + chl;
                const int c1 = (cp + 1 < nch) ? cp + 1 : nch - 1;
                float2 *po = chl ? chan.out[c1] : chan.out[cp];
                const cf r0 = chl ? (cf){chan.rot0[c1][0], chan.rot0[c1][1]} : (cf){chan.rot0[cp][0], chan.rot0[cp][1]};
                const int sl = chl ? (int)chan.slot[c1] : (int)chan.slot[cp];
                cf wl = ((sl & lane) & 1) ? (cf){-r0.x, -r0.y} : r0;
                const int64_t o0 = obase + 2 * (lane >> 2) + (lane & 1);
                if (cl < nch && !(diag & 2))
                    store_lane_rows<16 - MU0_FIRST, 32>(reinterpret_cast<cf *>(po) + o0, obase + LOUT <= M, o0, M,
                                                        [&](int k) { return cmul_v<false>(c[MU0_FIRST + k], wl); });
            }
            }
            else
            {
            // ---- general form (template flag NCO): channels at any centre bin and / or an NCO on the context
            // Round 4: every channel has its own centre bin B = 256 s + b (the prototype moved up by B / 4096 cycles/sample: b = 0
            // is round 3's slot grid).  H_c(k) = H(k - B): with k = k_low + 256 k2 (k_low = k0 + 16 k1 < 256 held by this lane and
            // group) k_low - b = kappa - 256 cy, so the lane needs the table entries of low index kappa -- group (i - b) mod 4, the
            // lanes rotated: a permutation, conflict-free -- for the slot s' = s + cy (tools/fft_model.py bank8_bins):
            //   Z_c(k2') = sum_a w_{k2'}[a] W16^(a s') G_q^kappa[a],  q = (k2' - s') mod 2
            // The table entry of kappa carries b_kappa^a (folded in for its owner); this lane's data owe b_klow^a =
            // b_kappa^a W4096^(a b) W16^(-a cy), and W16^(a s') W16^(-a cy) = W16^(a s): the factor beside the gathered entry is the
            // WAVE-UNIFORM W4096^(a B), B = 256 s + b (host, chan.tw, in SGPRs as in the slot form) -- the lanes differ only in which
            // entry they read.
            // k_low >> 2 = lane / 16 + 4 (lane % 16) in every group
            const int lq = (lane >> 4) + 4 * (lane & 15);
            const f2v *rowt = reinterpret_cast<const f2v *>(smem + LDS_ROWT);
            for (int cp = 0; cp < nch; cp += 2)
            {
                const bool last = cp + 2 >= nch; // the w values die with the last pair: refill with the next block
                cf a[16];
                // (round 5: channel by channel, its seven twiddles in SGPRs before its first table gather; per group the 2 x 8 gathers
                // fly under the products w[a] W4096^(a B): gather_mac)
#pragma unroll
                for (int ch = 0; ch < 2; ch++)
                {
                    if (ch == 1 && cp + 1 >= nch) // odd count: an empty second half
                    {
#pragma unroll
                        for (int i = 0; i < 4; i++)
                        {
                            a[4 * i + 2] = (cf){0.f, 0.f};
                            a[4 * i + 3] = (cf){0.f, 0.f};
                        }
                        continue;
                    }
                    const int c = cp + ch;
                    const int cb = (int)chan.bin[c], b = cb & 255, s = cb >> 8; // wave-uniform
                    cf tw[7];
#pragma unroll
                    for (int a8 = 1; a8 < 8; a8++)
                        tw[a8 - 1] = (cf){chan.tw[c][2 * (a8 - 1)], chan.tw[c][2 * (a8 - 1) + 1]}; // W4096^(a B)
                    // the lane that holds kappa and the parity of s' = s + cy: (k_low - b) >> 2 = lq - (b >> 2), one less in the groups below
                    // b % 4 (a borrow); negative: a borrow from k2 (cy = 1).  Two variants per channel, picked per group by a
                    // wave-uniform test (round 4 recomputed them per group): entry offsets of the halves q = s' & 1 and 1 - q
                    const int d0 = lq - (b >> 2), d1 = d0 - 1;
                    const int lk0 = d0 & 63, lk1 = d1 & 63;
                    const int par0 = (s + (d0 < 0 ? 1 : 0)) & 1, par1 = (s + (d1 < 0 ? 1 : 0)) & 1;
                    const int e0a = (((lk0 & 3) << 4) | (lk0 >> 2)) + 512 * par0, e0b = e0a + 512 - 1024 * par0;
                    const int e1a = (((lk1 & 3) << 4) | (lk1 >> 2)) + 512 * par1, e1b = e1a + 512 - 1024 * par1;
#pragma unroll
                    for (int i = 0; i < 4; i++)
                    {
                        const int ik = (i - b) & 3;                                 // table group of kappa (kappa % 4)
                        const bool bor = i < (b & 3);
                        const f2v *g0 = hp + ik * 1024 + (bor ? e1a : e0a); // k2' = 0: q = s' & 1       (+ a * 64 entries)
                        const f2v *g1 = hp + ik * 1024 + (bor ? e1b : e0b); // k2' = 1: q = (1 - s') & 1
                        cf t0[8], t1[8];
#pragma unroll
                        for (int a8 = 0; a8 < 8; a8++)
                        {
                            t0[a8] = r[phys(i, a8)];
                            t1[a8] = r[phys(i, a8 + 8)];
                        }
                        const cf z0 = gather_mac<8, 64>(t0, tw, g0);
                        const cf z1 = gather_mac<8, 64>(t1, tw, g1);
                        a[4 * i + 2 * ch] = z0 + z1;
                        a[4 * i + 2 * ch + 1] = cmul_v<true>(z0 - z1, twd[(i * 4 + 2) * 64 + lane]); // conj W512^(16 k1 + k0)
                    }
                }
                if (last && next_fast)
                {
#pragma unroll
                    for (int i = 0; i < EARLY_GROUPS; i++)
#pragma unroll
                        for (int j = 0; j < 16; j++)
                            load_row<I16, LAUX, EDGE>(r, nsrd, lane, phys(i, j));
                }
                cf c[16];
                inverse_tail256_tan(a, c, twe, xa, lane);
                if (last && next_fast)
                {
#pragma unroll
                    for (int i = EARLY_GROUPS; i < 4; i++)
#pragma unroll
                        for (int j = 0; j < 16; j++)
                            load_row<I16, LAUX, EDGE>(r, nsrd, lane, phys(i, j));
                }
                // mix-down: output o = obase + 32 (mu0 - first) + 2 mu1 + mu2 of the call belongs to input sample abs0n0 + 8 o and is
                // rotated by exp(-j 2 pi pword (abs0n0 + 8 o) / 2^32): a lane factor (exact 32-bit phase, one sincos per lane and
                // channel pair) times the channel's row phasor (LDS table, 256 input samples per row)
                const int chl = (lane >> 1) & 1, cl = cp + chl;
                const int c1 = (cp + 1 < nch) ? cp + 1 : nch - 1;
                float2 *po = chl ? chan.out[c1] : chan.out[cp];
                const uint32_t pw = chl ? chan.pword[c1] : chan.pword[cp];
                const int64_t o0 = obase + 2 * (lane >> 2) + (lane & 1);
                const float2 pa = phasor(0u - pw * (chan.abs0n0 + 8u * (uint32_t)o0));
                const cf wl = {pa.x, pa.y};
                const f2v *rowp_t = rowt + (chl ? c1 : cp) * 16;
                cf rowp[16 - MU0_FIRST];
                lds_fetch<16 - MU0_FIRST, 1>(rowp, rowp_t); // (round 5: the channel's row phasors requested together, ahead of the store loop)
                // decimation 24, 40, 56 (8 x sub): every sub-th output of this tail is a real output (KeepEvery; sub = 1: all of them)
                if (chan.sub == 1u) // (wave-uniform: decimation 8 itself keeps its plain store loop)
                {
                    if (cl < nch && !(diag & 2))
                        store_lane_rows<16 - MU0_FIRST, 32>(reinterpret_cast<cf *>(po) + o0, obase + LOUT <= M, o0, M, [&](int k) {
                            return cmul_v<false>(c[MU0_FIRST + k], cmul_v<false>(wl, rowp[k]));
                        });
                }
                else
                {
                    KeepEvery ke;
                    ke.init(blk, (unsigned)LOUT, chan.sub);
                    if (cl < nch && !(diag & 2))
                    {
#pragma unroll
                        for (int mu0 = MU0_FIRST; mu0 < 16; mu0++)
                        {
                            const int64_t idx = o0 + 32 * (mu0 - MU0_FIRST);
                            const int64_t kept = ke.index((unsigned)(2 * (lane >> 2) + (lane & 1)) + 32u * (unsigned)(mu0 - MU0_FIRST));
                            if (idx < M && kept >= 0)
                            {
                                const cf v = cmul_v<false>(c[mu0], cmul_v<false>(wl, rowp[mu0 - MU0_FIRST]));
                                __builtin_nontemporal_store(v, reinterpret_cast<cf *>(po) + kept);
                            }
                        }
                    }
                }
            }
            }
        }
        else if constexpr (CHAN == TAIL_BANK4_SLOTS)
        {
            // ---- uniform filter bank (SURVEY §8f-2): one forward transform, one decimated inverse per channel ---------
            // Channel slot s = the prototype moved to s/16 cycles/sample and mixed down: H_s(k2) = H(k2 - s), so with the
            // merged table of the single-channel path  G_s[m0][q] = W16^(m0 s) * G[m0][(q - s) mod 4]  (DESIGN.md §3.7).
            // First radix-4 stage of pass 3 once, in place: r[phys(i, m0 + 4 q)] = y[q][m0].
#pragma unroll
            for (int i = 0; i < 4; i++)
            {
                cf t[16];
#pragma unroll
                for (int j = 0; j < 16; j++)
                    t[j] = r[phys(i, j)];
                if constexpr (TAN)
                {
                    // inputs carry b^n2, b = W4096^(k0 + 16 k1); the b^m0 this stage still owes sits in the table G'
                    const cf e1 = tw1[(i * 3 + 0) * 64 + lane], e2 = tw1[(i * 3 + 1) * 64 + lane], e3 = tw1[(i * 3 + 2) * 64 + lane];
#pragma unroll
                    for (int m0 = 0; m0 < 4; m0++)
                        bfly4_tw<false>(t[m0], t[m0 + 4], t[m0 + 8], t[m0 + 12], e1, e2, e3, r[phys(i, m0)], r[phys(i, m0 + 4)],
                                        r[phys(i, m0 + 8)], r[phys(i, m0 + 12)]);
                }
                else
                {
#pragma unroll
                for (int m0 = 0; m0 < 4; m0++)
                    bfly4<false>(t[m0], t[m0 + 4], t[m0 + 8], t[m0 + 12], r[phys(i, m0)], r[phys(i, m0 + 4)],
                                 r[phys(i, m0 + 8)], r[phys(i, m0 + 12)]);
                }
            }
            constexpr int MU0_FIRST = OVL_ROWS / 4;
            const int nch = (int)chan.count;
            for (int ch = 0; ch < nch; ch++)
            {
                const bool last = (ch == nch - 1); // the y values die with the last channel: refill with the next block
                const int slot = (int)chan.slot[ch];
                const cf w1 = {chan.tw[ch][0], chan.tw[ch][1]}, w2 = {chan.tw[ch][2], chan.tw[ch][3]},
                         w3 = {chan.tw[ch][4], chan.tw[ch][5]};
                cf z[16];
#pragma unroll
                for (int i = 0; i < 4; i++)
                {
                    // (round 5: two sums at a time, their table reads requested ahead of the products: see the general form below)
#pragma unroll
                    for (int qp = 0; qp < 4; qp += 2)
                    {
                        cf gq[2][4], pr[2][4];
#pragma unroll
                        for (int q = 0; q < 2; q++)
                        {
                            const f2v *g = hp + (i * 16 + ((qp + q - slot) & 3)) * 64 + lane; // + m0 * 256 entries
#pragma unroll
                            for (int m0 = 0; m0 < 4; m0++)
                                gq[q][m0] = g[256 * m0];
                        }
                        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                        for (int q = 0; q < 2; q++)
                        {
                            pr[q][0] = r[phys(i, 4 * (qp + q))];
                            pr[q][1] = cmul_s<false>(r[phys(i, 4 * (qp + q) + 1)], w1);
                            pr[q][2] = cmul_s<false>(r[phys(i, 4 * (qp + q) + 2)], w2);
                            pr[q][3] = cmul_s<false>(r[phys(i, 4 * (qp + q) + 3)], w3);
                        }
#pragma unroll
                        for (int q = 0; q < 2; q++)
                        {
                            const cf e = cmac_v(cmul_v<false>(pr[q][0], gq[q][0]), pr[q][2], gq[q][2]);
                            const cf o = cmac_v(cmul_v<false>(pr[q][1], gq[q][1]), pr[q][3], gq[q][3]);
                            z[4 * i + qp + q] = e + o;
                        }
                    }
                    if (last && i < EARLY_GROUPS && next_fast)
                    {
#pragma unroll
                        for (int j = 0; j < 16; j++)
                            load_row<I16, LAUX, EDGE>(r, nsrd, lane, phys(i, j));
                    }
                }
                cf c[16];
                if constexpr (TAN)
                    inverse_dec4_tan(z, c, twe, twd, xa, lane);
                else
                    inverse_dec4(z, c, twd, twe, xa, lane);
                if (last && next_fast)
                {
#pragma unroll
                    for (int i = EARLY_GROUPS; i < 4; i++)
#pragma unroll
                        for (int j = 0; j < 16; j++)
                            load_row<I16, LAUX, EDGE>(r, nsrd, lane, phys(i, j));
                }
                // mix-down of the decimated output: exp(-j 2 pi slot a / 16), a = abs0 + n0 + 4 m, m = obase + 64 r + lane
                // with obase a multiple of 4: a call constant (rot0, host) times a quarter turn per lane
                const cf r0 = {chan.rot0[ch][0], chan.rot0[ch][1]};
                const int qt = (slot * lane) & 3;
                const cf wl = qt == 0 ? r0 : qt == 1 ? (cf){r0.y, -r0.x} : qt == 2 ? (cf){-r0.x, -r0.y} : (cf){-r0.y, r0.x};
                const srd_t csrd = make_srd(chan.out[ch] + obase, (diag & 2) ? 0 : (M - obase) * 8);
#pragma unroll
                for (int mu0 = MU0_FIRST; mu0 < 16; mu0++)
                    buf_store(csrd, voff, (mu0 - MU0_FIRST) * 512, cmul_v<false>(c[mu0], wl));
            }
        }
        else if constexpr (CHAN == TAIL_BANK4_OWN || CHAN == TAIL_BANK4_OWN_SUB)
        {
            // ---- filter bank at decimation 4, every channel at its own centre bin (round 4) ---------------------------------------
            // The slot form above with the table entries of kappa (k_low - b = kappa - 256 cy, gathered from the lane that holds kappa)
            // and the slot s' = s + cy:  Z_c(k_low, q) = sum_m0 y[q][m0] W16^(m0 s') G^kappa[m0][(q - s') mod 4].  The table holds
            // G' = b_kappa^m0 G (the factor the first stage owes, folded in for the lane that owns the entry); this lane's data owe
            // b_klow^m0 = b_kappa^m0 W4096^(m0 b) W16^(-m0 cy), and W16^(m0 s') W16^(-m0 cy) = W16^(m0 s): the factor beside the table is
            // the wave-uniform W4096^(m0 B), B = 256 s + b (host, chan.tw) -- the lanes differ only in WHICH entry they read.
#pragma unroll
            for (int i = 0; i < 4; i++)
            {
                cf t[16];
#pragma unroll
                for (int j = 0; j < 16; j++)
                    t[j] = r[phys(i, j)];
                static_assert((CHAN != TAIL_BANK4_OWN && CHAN != TAIL_BANK4_OWN_SUB) || TAN, "the general form at decimation 4 is written for the (cos, tan) image");
                const cf e1 = tw1[(i * 3 + 0) * 64 + lane], e2 = tw1[(i * 3 + 1) * 64 + lane], e3 = tw1[(i * 3 + 2) * 64 + lane];
#pragma unroll
                for (int m0 = 0; m0 < 4; m0++)
                    bfly4_tw<false>(t[m0], t[m0 + 4], t[m0 + 8], t[m0 + 12], e1, e2, e3, r[phys(i, m0)], r[phys(i, m0 + 4)],
                                    r[phys(i, m0 + 8)], r[phys(i, m0 + 12)]);
            }
            constexpr int MU0_FIRST = OVL_ROWS / 4;
            const int nch = (int)chan.count;
            const int lq = (lane >> 4) + 4 * (lane & 15); // k_low >> 2
            const f2v *rowt = reinterpret_cast<const f2v *>(smem + LDS_ROWT);
            for (int ch = 0; ch < nch; ch++)
            {
                const bool last = (ch == nch - 1); // the y values die with the last channel: refill with the next block
                const int cb = (int)chan.bin[ch], b = cb & 255, s = cb >> 8; // wave-uniform
                const cf w1 = {chan.tw[ch][0], chan.tw[ch][1]}, w2 = {chan.tw[ch][2], chan.tw[ch][3]},
                         w3 = {chan.tw[ch][4], chan.tw[ch][5]};
                cf z[16];
#pragma unroll
                for (int i = 0; i < 4; i++)
                {
                    const int ik = (i - b) & 3;                            // table group of kappa (kappa % 4)
                    const int d = lq - (b >> 2) - ((i < (b & 3)) ? 1 : 0); // (k_low - b) >> 2, negative: a borrow from k2
                    const int lk = d & 63;
                    const int lane_k = ((lk & 3) << 4) | (lk >> 2);        // the lane that holds kappa in group ik
                    const int sp = s + (d < 0 ? 1 : 0);
                    // (round 5: two of the group's four sums at a time -- their eight gathers are requested first, the six products
                    // y w fly under them, then the multiply-accumulates; round 4's form had every table read in front of its use)
#pragma unroll
                    for (int qp = 0; qp < 4; qp += 2)
                    {
                        cf gq[2][4], pr[2][4];
#pragma unroll
                        for (int q = 0; q < 2; q++)
                        {
                            const f2v *g = hp + (ik * 16 + ((qp + q - sp) & 3)) * 64 + lane_k; // + m0 * 256 entries
#pragma unroll
                            for (int m0 = 0; m0 < 4; m0++)
                                gq[q][m0] = g[256 * m0];
                        }
                        __builtin_amdgcn_sched_barrier(0); // (the gathers stay up here: see gather_mac)
#pragma unroll
                        for (int q = 0; q < 2; q++)
                        {
                            pr[q][0] = r[phys(i, 4 * (qp + q))];
                            pr[q][1] = cmul_s<false>(r[phys(i, 4 * (qp + q) + 1)], w1);
                            pr[q][2] = cmul_s<false>(r[phys(i, 4 * (qp + q) + 2)], w2);
                            pr[q][3] = cmul_s<false>(r[phys(i, 4 * (qp + q) + 3)], w3);
                        }
#pragma unroll
                        for (int q = 0; q < 2; q++)
                        {
                            const cf e = cmac_v(cmul_v<false>(pr[q][0], gq[q][0]), pr[q][2], gq[q][2]);
                            const cf o = cmac_v(cmul_v<false>(pr[q][1], gq[q][1]), pr[q][3], gq[q][3]);
                            z[4 * i + qp + q] = e + o;
                        }
                    }
                    if (last && i < EARLY_GROUPS && next_fast)
                    {
#pragma unroll
                        for (int j = 0; j < 16; j++)
                            load_row<I16, LAUX, EDGE>(r, nsrd, lane, phys(i, j));
                    }
                }
                cf c[16];
                inverse_dec4_tan(z, c, twe, twd, xa, lane);
                if (last && next_fast)
                {
#pragma unroll
                    for (int i = EARLY_GROUPS; i < 4; i++)
#pragma unroll
                        for (int j = 0; j < 16; j++)
                            load_row<I16, LAUX, EDGE>(r, nsrd, lane, phys(i, j));
                }
                // mix-down: output o = obase + 64 (mu0 - first) + lane of the call belongs to input sample abs0n0 + 4 o: a lane factor
                // (exact 32-bit phase) times the channel's row phasor (256 input samples per row)
                const float2 pa = phasor(0u - chan.pword[ch] * (chan.abs0n0 + 4u * (uint32_t)(obase + lane)));
                const cf wl = {pa.x, pa.y};
                const f2v *rowp_t = rowt + ch * 16;
                cf rowp[16 - MU0_FIRST];
                lds_fetch<16 - MU0_FIRST, 1>(rowp, rowp_t); // (round 5: the channel's row phasors requested together, ahead of the store loop)
                // decimation 12, 20, 28, ... (4 x sub): every sub-th output of this tail is a real output (KeepEvery, as in the
                // single-channel tail; sub = 1: all of them).  Descriptor over the kept outputs from this block's first one on.
                if constexpr (CHAN == TAIL_BANK4_OWN) // (decimation 4 itself; its own instantiation: with both store loops in one kernel it ran 4 % slower)
                {
                    const srd_t csrd = make_srd(chan.out[ch] + obase, (diag & 2) ? 0 : (M - obase) * 8);
#pragma unroll
                    for (int mu0 = MU0_FIRST; mu0 < 16; mu0++)
                        buf_store(csrd, voff, (mu0 - MU0_FIRST) * 512, cmul_v<false>(c[mu0], cmul_v<false>(wl, rowp[mu0 - MU0_FIRST])));
                }
                else
                {
                    KeepEvery ke;
                    ke.init(blk, (unsigned)LOUT, chan.sub);
                    const int64_t qb = ke.qU + (ke.rem ? 1 : 0);
                    const srd_t csrd = make_srd(chan.out[ch] + qb, (diag & 2) ? 0 : (decn_m - qb) * 8);
                    const int lim = (int)((M - obase) < 65536 ? (M - obase) : 65536); // tail outputs of the call left from this block on
#pragma unroll
                    for (int mu0 = MU0_FIRST; mu0 < 16; mu0++)
                    {
                        const unsigned so = ke.store_offset((unsigned)lane + 64u * (unsigned)(mu0 - MU0_FIRST), lane + 64 * (mu0 - MU0_FIRST) < lim);
                        buf_store(csrd, so, 0, cmul_v<false>(c[mu0], cmul_v<false>(wl, rowp[mu0 - MU0_FIRST])));
                    }
                }
            }
        }
