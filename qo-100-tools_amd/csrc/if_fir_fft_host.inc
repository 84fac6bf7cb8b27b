// if_fir_fft_host.inc -- part of the overlap-save kernel's source (if_fir_fft.hip includes it; not a translation unit of its own).
// Host side (the unit compiled without a kernel selector): launch_fft, the table images (routing: if_fir_fft_route.h).
hipError_t launch_fft(const LaunchArgs &a)
{
    if (!a.fft_tables)
        return hipErrorInvalidConfiguration;
    const FftRoute r = fft_route_of(a);
    if (r.family == FFT_FAMILY_ODD)
        return launch_fft_odd(a);
    if (r.family == FFT_FAMILY_TWO_PARTITIONS)
        return launch_fft_two_partitions(a, r);
    if (r.family != FFT_FAMILY_ROWS) // (the call is not served)
        return hipErrorInvalidConfiguration;
    switch (r.rows)
    {
    case 4: return launch_fft_rows<4>(a, r);
    case 8: return launch_fft_rows<8>(a, r);
    case 16: return launch_fft_rows<16>(a, r);
    case 32: return launch_fft_rows<32>(a, r);
    default: return launch_fft_rows<48>(a, r);
    }
}

// (cos, tan) form of the twiddle exp(j th): (c, t) with c = cos th rounded to float32 and t = sin th / c; an exact zero of the
// cosine is stored as +-2^-30 (its own contribution is below rounding, the tangent stays finite).  c_ref != 0: the first
// component is c / c_ref instead (third input of a radix-4 butterfly, see bfly4_tw).
static double tan_cos(double th)
{
    double c = cos(th);
    if (fabs(c) < 9.3e-10)
        c = (c < 0.0 ? -1.0 : 1.0) * 9.313225746154785e-10;
    return (double)(float)c;
}
static void tan_entry(double th, double c_ref, float *e)
{
    const double c = tan_cos(th);
    e[1] = (float)(sin(th) / c);
    e[0] = (float)(c_ref != 0.0 ? c / c_ref : c);
}
// the 15 table entries of fft16_tw for the base twiddle exp(j th): entry k at out[2 * k * stride]
static void tan_fft16_entries(double th, float *out, int stride)
{
    const double w16 = -6.283185307179586476925286766559 / 16.0;
    tan_entry(4.0 * th, 0.0, out);
    tan_entry(8.0 * th, 0.0, out + 2 * stride);
    tan_entry(12.0 * th, tan_cos(4.0 * th), out + 4 * stride);
    for (int q = 0; q < 4; q++)
    {
        const double b = th + w16 * q;
        tan_entry(b, 0.0, out + 2 * (3 + 3 * q) * stride);
        tan_entry(2.0 * b, 0.0, out + 2 * (4 + 3 * q) * stride);
        tan_entry(3.0 * b, tan_cos(b), out + 2 * (5 + 3 * q) * stride);
    }
}

// the filter banks' forward passes 2 and 3 (first stage) in (cos, tan) form, as in the decimate-by-4 image (fft_build_tables)
// the filter-bank images' table between the two transforms of the small inverse (inverse_tail256_tan): twet[e * 16 + mu1], b = W256^mu1
static void bank_tan_inverse(float *twe)
{
    const double PI2 = 6.283185307179586476925286766559;
    for (int e = 0; e < 2 * 1024; e++)
        twe[e] = 0.0f;
    for (int mu1 = 0; mu1 < 16; mu1++)
        tan_fft16_entries(-PI2 * (double)mu1 / 256.0, twe + 2 * mu1, 16);
}

static void bank_tan_forward(float *tw1, float *tw2)
{
    const double PI2 = 6.283185307179586476925286766559;
    for (int e = 0; e < 2 * 4096; e++)
        tw1[e] = 0.0f;
    for (int e = 0; e < 2 * 256; e++)
        tw2[e] = 0.0f;
    for (int i = 0; i < 4; i++)
    {
        for (int lane = 0; lane < 64; lane++)
        {
            float all[30];
            tan_fft16_entries(-PI2 * (double)((4 * (lane / 16) + i) + 16 * (lane % 16)) / 4096.0, all, 1);
            for (int e = 0; e < 3; e++)
            {
                tw1[2 * ((i * 3 + e) * 64 + lane) + 0] = all[2 * e];
                tw1[2 * ((i * 3 + e) * 64 + lane) + 1] = all[2 * e + 1];
            }
        }
        for (int g = 0; g < 4; g++)
            tan_fft16_entries(-PI2 * (double)(4 * g + i) / 256.0, tw2 + 2 * (i * 60 + g), 4);
    }
}

// the phasor tables of lds_phasor, at bytes [6 KB, 8 KB) of the image: P1[k] = exp(j 2 pi k / 128), P2[k] = exp(j 2 pi k / 16384)
void fft_phasor_tables(float *tables)
{
    const double PI2 = 6.283185307179586476925286766559;
    float *pht = tables + 6144 / 4;
    for (int k = 0; k < 128; k++)
    {
        pht[2 * k + 0] = (float)cos(PI2 * (double)k / 128.0);
        pht[2 * k + 1] = (float)sin(PI2 * (double)k / 128.0);
        pht[2 * (128 + k) + 0] = (float)cos(PI2 * (double)k / 16384.0);
        pht[2 * (128 + k) + 1] = (float)sin(PI2 * (double)k / 16384.0);
    }
}

// Host side: twiddle and H tables in the kernel's LDS image order (float64 math, rounded once to float32).
//   [0, 32 KB)      tw1[(rho*16+k0)*64 + lane] = W4096^((lane+64*rho)*k0)
//   [32 KB, 64 KB)  hp [(i*16+k2)*64 + lane]   = FFT(taps)[(4*(lane/16)+i) + 16*(lane%16) + 256*k2] / 4096
//   [64 KB, 66 KB)  tw2[k1*16 + n2]            = W256^(n2*k1)
//   [66 KB, 82 KB)  twd, twe: twiddles of the decimate-by-4 1024-point inverse
void fft_build_tables(const float *taps, int T, int ctaps, const FftImage &image, uint32_t nco_delta, double in_scale,
                      float *tables /* FFT_TABLE_FLOATS floats */)
{
    const int bank = image.kind == FFT_IMAGE_BANK8 ? 8 : image.kind == FFT_IMAGE_BANK16 ? 16 : 0, bank_parity = image.parity;
    const int D = image.kind == FFT_IMAGE_DEC4 ? 4 : 1, full_rate = image.kind == FFT_IMAGE_FULL_RATE;
    const double PI2 = 6.283185307179586476925286766559;
    float *tw1 = tables, *hp = tables + 2 * 4096, *tw2 = tables + 4 * 4096;
    float *twd = tw2 + 2 * 256, *twe = twd + 2 * 1024, *ncob = twe + 2 * 1024, *twf = ncob + 2 * 64;
    // decimate-by-2 inverse: twf[i*64 + lane] = W2048^(16*(lane%16) + 4*(lane/16) + i)
    for (int i = 0; i < 4; i++)
        for (int lane = 0; lane < 64; lane++)
        {
            const int e = 16 * (lane % 16) + 4 * (lane / 16) + i;
            const double a = -PI2 * (double)e / 2048.0;
            twf[2 * (i * 64 + lane) + 0] = (float)cos(a);
            twf[2 * (i * 64 + lane) + 1] = (float)sin(a);
        }
    // NCO (SPEC §3.2): rotation shared by the 64 outputs of row r of a block, exp(+j*2*pi*((64 r delta) mod 2^32)/2^32)
    // (the decimating filter-bank tails store 16 / 32 outputs per slot: bank = 16 / 8)
    const uint32_t nco_step = bank == 16 ? 16u : bank == 8 ? 32u : 64u;
    for (uint32_t r = 0; r < 64; r++)
    {
        // (bank tails: entries 32..63 hold the lane's share, phasor((r - 32) delta): output index within a slot; entries
        // 16..31 the 16th roots of unity W16^(r - 16) = exp(-j 2 pi (r - 16) / 16): the slots' mix-down phases)
        const uint32_t ph = (bank && r >= 32) ? (r - 32u) * nco_delta
                            : (bank && r >= 16) ? 0u - ((r - 16u) << 28) : nco_step * r * nco_delta;
        const double a = PI2 * ((double)ph / 4294967296.0);
        ncob[2 * r + 0] = (float)cos(a);
        ncob[2 * r + 1] = (float)sin(a);
    }
    // decimate-by-4 inverse: twd[(i*4+mu2)*64 + lane] = W1024^((16*(lane%16) + 4*(lane/16) + i)*mu2)
    //                        twe[mu1*64 + lane]       = W256^((4*(lane/16) + (lane%16)/4)*mu1)
    for (int i = 0; i < 4; i++)
        for (int mu2 = 0; mu2 < 4; mu2++)
            for (int lane = 0; lane < 64; lane++)
            {
                const int e = ((16 * (lane % 16) + 4 * (lane / 16) + i) * mu2) % 1024;
                const double a = -PI2 * (double)e / 1024.0;
                twd[2 * ((i * 4 + mu2) * 64 + lane) + 0] = (float)cos(a);
                twd[2 * ((i * 4 + mu2) * 64 + lane) + 1] = (float)sin(a);
            }
    for (int mu1 = 0; mu1 < 16; mu1++)
        for (int lane = 0; lane < 64; lane++)
        {
            const int e = ((4 * (lane / 16) + (lane % 16) / 4) * mu1) % 256;
            const double a = -PI2 * (double)e / 256.0;
            twe[2 * (mu1 * 64 + lane) + 0] = (float)cos(a);
            twe[2 * (mu1 * 64 + lane) + 1] = (float)sin(a);
        }
    for (int rho = 0; rho < 4; rho++)
        for (int k0 = 0; k0 < 16; k0++)
            for (int lane = 0; lane < 64; lane++)
            {
                const int e = ((lane + 64 * rho) * k0) % 4096;
                const double a = -PI2 * (double)e / 4096.0;
                tw1[2 * ((rho * 16 + k0) * 64 + lane) + 0] = (float)cos(a);
                tw1[2 * ((rho * 16 + k0) * 64 + lane) + 1] = (float)sin(a);
            }
    for (int k1 = 0; k1 < 16; k1++)
        for (int n2 = 0; n2 < 16; n2++)
        {
            const double a = -PI2 * (double)((n2 * k1) % 256) / 256.0;
            tw2[2 * (k1 * 16 + n2) + 0] = (float)cos(a);
            tw2[2 * (k1 * 16 + n2) + 1] = (float)sin(a);
        }
    // DFT of the taps in float64 with an exact-argument table
    std::vector<double> ct(4096), st(4096), hd(2 * 4096); // not static: contexts may be created from several threads
    for (int e = 0; e < 4096; e++)
    {
        ct[e] = cos(-PI2 * (double)e / 4096.0);
        st[e] = sin(-PI2 * (double)e / 4096.0);
    }
    for (int i = 0; i < 4; i++)
        for (int k2 = 0; k2 < 16; k2++)
            for (int lane = 0; lane < 64; lane++)
            {
                const int k = (4 * (lane / 16) + i) + 16 * (lane % 16) + 256 * k2;
                double re = 0.0, im = 0.0;
                for (int n = 0; n < T; n++)
                {
                    const int e = (int)(((int64_t)k * n) & 4095);
                    const double hr = ctaps ? (double)taps[2 * n] : (double)taps[n];
                    const double hi = ctaps ? (double)taps[2 * n + 1] : 0.0;
                    re += hr * ct[e] - hi * st[e];
                    im += hr * st[e] + hi * ct[e];
                }
                hd[2 * ((i * 16 + k2) * 64 + lane) + 0] = re / 4096.0 * in_scale; // in_scale: 2^-15 for raw int16 samples
                hd[2 * ((i * 16 + k2) * 64 + lane) + 1] = im / 4096.0 * in_scale;
            }
    if (bank == 8)
    {
        // filter bank at decimation 8: G_q[a] = W16^(a q) sum_j H(k0 + 16 k1 + 256 (q + 2 j)) W8^(a j) at ((i*16 + 8 q + a)*64 + lane)
        // (second stage of pass 3, the multiplication by the slot's H and the 8-way alias fold merged; kernel, TAIL_BANK8_CHANNEL)
        for (int i = 0; i < 4; i++)
            for (int lane = 0; lane < 64; lane++)
                for (int q = 0; q < 2; q++)
                    for (int a8 = 0; a8 < 8; a8++)
                    {
                        double re = 0.0, im = 0.0;
                        for (int j = 0; j < 8; j++)
                        {
                            const double *h = &hd[2 * ((i * 16 + q + 2 * j) * 64 + lane)];
                            const int e = (256 * a8 * q + 512 * a8 * j) & 4095;
                            re += h[0] * ct[e] - h[1] * st[e];
                            im += h[0] * st[e] + h[1] * ct[e];
                        }
                        // Round 4: the bank's forward passes are the decimate-by-4 kernels' ((cos, tan) twiddles on the inputs of passes 2
                        // and 3), so the factor b^a, b = W4096^(k0 + 16 k1), that input a of pass 3 still carries is folded in here.
                        // This image serves the per-channel forms (TAIL_BANK8_CHANNEL) and the all-slots form's even slots (TAIL_BANK8_ALL);
                        // bank_parity = 1: the all-slots form's image for the ODD slots -- also the slot twiddle's common factor W16^a,
                        // and the halves exchanged (first half: the factor of w0 = G_1, second: G_0)
                        int half = q;
                        {
                            const int par = bank_parity ? 1 : 0;
                            const int eb = a8 * ((4 * (lane / 16) + i) + 16 * (lane % 16)); // b^a
                            const int e = (256 * a8 * par + eb) & 4095; // W16^(a par) b^a
                            const double gr = re * ct[e] - im * st[e], gi = re * st[e] + im * ct[e];
                            re = gr;
                            im = gi;
                            half = par ? 1 - q : q;
                        }
                        hp[2 * ((i * 16 + 8 * half + a8) * 64 + lane) + 0] = (float)re;
                        hp[2 * ((i * 16 + 8 * half + a8) * 64 + lane) + 1] = (float)im;
                    }
        bank_tan_forward(tw1, tw2); // (the 512-point inverse keeps twd above)
        bank_tan_inverse(twe);
        fft_phasor_tables(tables);
        return;
    }
    if (bank == 16)
    {
        // 16-slot filter bank at the channel rate: G0[n2] = sum_k2 H(k0 + 16 k1 + 256 k2) W16^(n2 k2) at ((i*16 + n2)*64 + lane)
        // (pass 3, the multiplication by the slot's H and the 16-way alias fold merged; see the kernel, TAIL_BANK16_ALL)
        for (int i = 0; i < 4; i++)
            for (int lane = 0; lane < 64; lane++)
                for (int n2 = 0; n2 < 16; n2++)
                {
                    double re = 0.0, im = 0.0;
                    for (int k2 = 0; k2 < 16; k2++)
                    {
                        const double *h = &hd[2 * ((i * 16 + k2) * 64 + lane)];
                        const int e = (256 * n2 * k2) & 4095;
                        re += h[0] * ct[e] - h[1] * st[e];
                        im += h[0] * st[e] + h[1] * ct[e];
                    }
                    {
                        // (round 4) the b^n2, b = W4096^(k0 + 16 k1), that input n2 of pass 3 still carries ((cos, tan) forward passes)
                        const int eb = (n2 * ((4 * (lane / 16) + i) + 16 * (lane % 16))) & 4095;
                        const double gr = re * ct[eb] - im * st[eb], gi = re * st[eb] + im * ct[eb];
                        re = gr;
                        im = gi;
                    }
                    hp[2 * ((i * 16 + n2) * 64 + lane) + 0] = (float)re;
                    hp[2 * ((i * 16 + n2) * 64 + lane) + 1] = (float)im;
                }
        bank_tan_forward(tw1, tw2);
        bank_tan_inverse(twe);
        fft_phasor_tables(tables);
        return;
    }
    if (D != 4)
    {
        for (int e = 0; e < 2 * 4096; e++)
            hp[e] = (float)hd[e];
        if (full_rate)
        {
            // the full-rate pipeline's twiddles in (cos, tan) form (LDS map at the top of the file): forward pass 2 and the first
            // stage of forward pass 3 as in the decimate-by-4 image; the shared table T; inverse pass 2
            for (int e = 0; e < 2 * 4096; e++)
                tw1[e] = 0.0f;
            for (int e = 0; e < 2 * 256; e++)
                tw2[e] = 0.0f;
            for (int e = 0; e < 2 * 1024; e++)
                twd[e] = 0.0f;
            for (int i = 0; i < 4; i++)
            {
                for (int lane = 0; lane < 64; lane++)
                {
                    float all[30];
                    tan_fft16_entries(-PI2 * (double)((4 * (lane / 16) + i) + 16 * (lane % 16)) / 4096.0, all, 1);
                    for (int e = 0; e < 3; e++)
                    {
                        tw1[2 * ((i * 3 + e) * 64 + lane) + 0] = all[2 * e];
                        tw1[2 * ((i * 3 + e) * 64 + lane) + 1] = all[2 * e + 1];
                    }
                }
                for (int g = 0; g < 4; g++)
                    tan_fft16_entries(-PI2 * (double)(4 * g + i) / 256.0, tw2 + 2 * (i * 60 + g), 4);
            }
            float *tt = tw1 + 2 * 1024; // (LDS_TT)
            for (int m = 0; m < 1024; m++)
            {
                const double th = -PI2 * (double)m / 4096.0;
                const unsigned pos = tsw((unsigned)m);
                tan_entry(th, 0.0, tt + 2 * pos);
                tan_entry(2.0 * th, 0.0, tt + 2 * (1024 + pos));
                tan_entry(3.0 * th, tan_cos(th), tt + 2 * (2048 + pos));
            }
            for (int n2 = 0; n2 < 16; n2++)
                tan_fft16_entries(-PI2 * (double)n2 / 256.0, twd + 2 * n2, 16);
            fft_phasor_tables(tables);
        }
        return;
    }
    // decimate-by-4 kernels: the table holds G[m0][q] = W16^(m0 q) * sum_p H(q + 4p) W4^(m0 p) at ((i*16 + 4*m0 + q)*64 + lane)
    // (second radix-4 stage of pass 3, multiplication by H and alias fold merged; see the kernel)
    for (int i = 0; i < 4; i++)
        for (int lane = 0; lane < 64; lane++)
            for (int m0 = 0; m0 < 4; m0++)
                for (int q = 0; q < 4; q++)
                {
                    double re = 0.0, im = 0.0;
                    for (int p = 0; p < 4; p++)
                    {
                        const double *h = &hd[2 * ((i * 16 + q + 4 * p) * 64 + lane)];
                        const int e = (256 * m0 * q + 1024 * m0 * p) & 4095; // W16^(m0 q) W4^(m0 p) as a power of W4096
                        re += h[0] * ct[e] - h[1] * st[e];
                        im += h[0] * st[e] + h[1] * ct[e];
                    }
                    {
                        // G' = b^m0 G, b = W4096^(k0 + 16 k1): the factor the first stage of pass 3 still owes (see the kernel)
                        const int eb = (m0 * ((4 * (lane / 16) + i) + 16 * (lane % 16))) & 4095;
                        const double gr = re * ct[eb] - im * st[eb], gi = re * st[eb] + im * ct[eb];
                        re = gr;
                        im = gi;
                    }
                    hp[2 * ((i * 16 + 4 * m0 + q) * 64 + lane) + 0] = (float)re;
                    hp[2 * ((i * 16 + 4 * m0 + q) * 64 + lane) + 1] = (float)im;
                }
    // the decimate-by-4 kernels' twiddles in (cos, tan) form, in the slots of the tables they replace (LDS map at the top)
    for (int e = 0; e < 2 * 4096; e++)
        tw1[e] = 0.0f;
    for (int e = 0; e < 2 * 256; e++)
        tw2[e] = 0.0f;
    for (int e = 0; e < 2 * 1024; e++)
        twd[e] = twe[e] = 0.0f;
    for (int i = 0; i < 4; i++)
    {
        for (int lane = 0; lane < 64; lane++)
        {
            // pass 3, first stage: b = W4096^(k0 + 16 k1); only entries 0..2 (b^4, b^8, b^12) are used
            float all[30];
            tan_fft16_entries(-PI2 * (double)((4 * (lane / 16) + i) + 16 * (lane % 16)) / 4096.0, all, 1);
            for (int e = 0; e < 3; e++)
            {
                tw1[2 * ((i * 3 + e) * 64 + lane) + 0] = all[2 * e];
                tw1[2 * ((i * 3 + e) * 64 + lane) + 1] = all[2 * e + 1];
            }
        }
        for (int g = 0; g < 4; g++) // pass 2: b = W256^k0, k0 = 4 g + i
            tan_fft16_entries(-PI2 * (double)(4 * g + i) / 256.0, tw2 + 2 * (i * 60 + g), 4);
    }
    for (int lane = 0; lane < 64; lane++) // inverse, last pass: b = W1024^lane
        tan_fft16_entries(-PI2 * (double)lane / 1024.0, twd + 2 * lane, 64);
    for (int mu2 = 0; mu2 < 4; mu2++) // inverse, middle pass: b = W64^mu2
        tan_fft16_entries(-PI2 * (double)mu2 / 64.0, twe + 2 * mu2, 4);
    fft_phasor_tables(tables);
}

// Table image of the odd-decimation kernel (fir_odd_kernel, F = 3 or 5), float64 math, rounded once:
//   G_p [(p*16 + slot)*64 + lane] = FFT1024(g_p)[k0 + 16 k1 + 256 k2'] / 1024 (slot = 4 i + k2', k0 = 4 (lane/16) + i, k1 = lane%16),
//        g_0[k] = h[F k], g_p[d] = h[F d - p] (p >= 1, d >= 1);  in_scale: 2^-15 for raw int16 samples
//   TB [e*16 + k0] (b = W256^k0) | TC [(i*3 + e)*64 + lane] (b = W1024^(k0 + 16 k1), entries 0..2 of the transform's 15)
//   TWD [e*64 + lane] (b = W1024^lane) | TWE [e*4 + mu2] (b = W64^mu2) | NCO row phasors (64 outputs per row)
void fft_build_tables_odd(const float *taps, int T, int ctaps, int F, uint32_t nco_delta, double in_scale, float *tables)
{
    const double PI2 = 6.283185307179586476925286766559;
    float *gt = tables, *tb = gt + 2 * F * 1024, *tc = tb + 2 * 256, *twd = tc + 2 * 768, *twe = twd + 2 * 1024, *ncob = twe + 2 * 64;
    for (int e = 0; e < 2 * (256 + 768 + 1024 + 64 + 64); e++)
        tb[e] = 0.0f;
    fft_phasor_tables(ncob + 2 * 64 - 6144 / 4); // (the phasor tables of lds_phasor, behind the NCO row phasors)
    for (int k0 = 0; k0 < 16; k0++)
        tan_fft16_entries(-PI2 * (double)k0 / 256.0, tb + 2 * k0, 16);
    for (int i = 0; i < 4; i++)
        for (int lane = 0; lane < 64; lane++)
        {
            float all[30];
            tan_fft16_entries(-PI2 * (double)((4 * (lane / 16) + i) + 16 * (lane % 16)) / 1024.0, all, 1);
            // (the last pass is a 4-point DFT over mu2: its inputs carry b, b^2, b^3 = entries 3, 4, 5 of the 16-point set, q = 0)
            for (int e = 0; e < 3; e++)
            {
                tc[2 * ((i * 3 + e) * 64 + lane) + 0] = all[2 * (3 + e)];
                tc[2 * ((i * 3 + e) * 64 + lane) + 1] = all[2 * (3 + e) + 1];
            }
        }
    for (int lane = 0; lane < 64; lane++)
        tan_fft16_entries(-PI2 * (double)lane / 1024.0, twd + 2 * lane, 64);
    for (int mu2 = 0; mu2 < 4; mu2++)
        tan_fft16_entries(-PI2 * (double)mu2 / 64.0, twe + 2 * mu2, 4);
    for (uint32_t r = 0; r < 64; r++)
    {
        const double a = PI2 * ((double)(uint32_t)(64u * r * nco_delta) / 4294967296.0);
        ncob[2 * r + 0] = (float)cos(a);
        ncob[2 * r + 1] = (float)sin(a);
    }
    std::vector<double> ct(1024), st(1024), gr(1024), gi(1024);
    for (int e = 0; e < 1024; e++)
    {
        ct[e] = cos(-PI2 * (double)e / 1024.0);
        st[e] = sin(-PI2 * (double)e / 1024.0);
    }
    for (int p = 0; p < F; p++)
    {
        // polyphase component p at the decimated rate, with the delay of its phase stream
        for (int e = 0; e < 1024; e++)
            gr[e] = gi[e] = 0.0;
        for (int k = 0; k < T; k++)
        {
            // x[F m - k] = x_p[m - d] with F d - p = k
            if ((k + p) % F)
                continue;
            const int d = (k + p) / F;
            gr[d] += ctaps ? (double)taps[2 * k] : (double)taps[k];
            gi[d] += ctaps ? (double)taps[2 * k + 1] : 0.0;
        }
        int dmax = 0;
        for (int e = 0; e < 1024; e++)
            if (gr[e] != 0.0 || gi[e] != 0.0)
                dmax = e;
        for (int slot = 0; slot < 16; slot++)
            for (int lane = 0; lane < 64; lane++)
            {
                const int k = (4 * (lane / 16) + slot / 4) + 16 * (lane % 16) + 256 * (slot % 4);
                double re = 0.0, im = 0.0;
                for (int d = 0; d <= dmax; d++)
                {
                    const int e = (int)(((int64_t)k * d) & 1023);
                    re += gr[d] * ct[e] - gi[d] * st[e];
                    im += gr[d] * st[e] + gi[d] * ct[e];
                }
                gt[2 * ((p * 16 + slot) * 64 + lane) + 0] = (float)(re / 1024.0 * in_scale);
                gt[2 * ((p * 16 + slot) * 64 + lane) + 1] = (float)(im / 1024.0 * in_scale);
            }
    }
}

