// if_fir_combiner_shim.cpp — the C ABI of the channel combiner (include/if_fir.h, if_fir_combiner_*; docs/SPEC.md §9).  Its own
// opaque context on the streaming contexts' shared base.  Same conventions as the interpolator: 1/0 status, a message per
// context, no CPU fallback; a failed call leaves the context and its stream position unchanged.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#include "if_fir.h"
#ifdef IF_FIR_DEVELOPMENT
#include "if_fir_debug.h"
#endif
#include "if_fir_combiner.h"
#include "if_fir_stream_ctx.h"

#define IF_FIR_API extern "C" __attribute__((visibility("default")))

// the streaming state: what a call advances (and a failed if_fir_combiner_process puts back)
struct combiner_state
{
    int hist_cur;
    uint64_t consumed;        // input samples per channel since init/reset (the next call's first output has index consumed * L)
};

// the centres as the kernels take them: phase words split into grid point and residual, one multiply table per distinct residual
struct combiner_plan
{
    uint32_t word[if_fir::COMBINER_MAX_CHANNELS];
    uint32_t rword[if_fir::COMBINER_MAX_CHANNELS];
    uint16_t G[if_fir::COMBINER_MAX_CHANNELS];
    uint16_t table[if_fir::COMBINER_MAX_CHANNELS];
    int tab_cur;              // which of the two device images of the residual tables the kernels read
};

struct if_fir_combiner : if_fir::StreamCtx
{
    int T, L, C;
    int ctaps;
    uint32_t backend_req, backend;
    std::vector<float> taps;  // host copy: if_fir_combiner_set_centres rebuilds the residual tables from it
    float *d_taps;            // generic kernel: T floats or T (re, im) pairs
    float2 *d_H[2], *d_tw;    // overlap-save: (C + 1) multiply tables of 4096 entries -- table 0 = the plain H, in both images --
                              // and the twiddles (nullptr outside the overlap-save range)
    if_fir::StreamHistory hist; // the last hist_len input samples of every channel (C x hist_len), float32
    int hist_len;
    combiner_state st;
    combiner_plan plan;
    void *d_stage_in, *d_stage_out; // if_fir_combiner_process: C x ullMaxSamples inputs, ullMaxSamples x L outputs
    int grid_limit;           // development hook
};

using if_fir::set_err;
static thread_local char g_combiner_init_err[256] = "";

static uint32_t resolve_backend(const if_fir_combiner *c, uint32_t req)
{
    if (req == IF_FIR_BACKEND_AUTO)
        return if_fir::combiner_fft_supported(c->T, c->L) ? IF_FIR_BACKEND_HIP_FFT : IF_FIR_BACKEND_HIP_GENERIC;
    return req;
}

// bytes between two channels in the host-pointer call's input staging buffer: ullMaxSamples float32 samples, rounded up to the
// generic backend's 16-byte alignment
static size_t stage_pitch(uint64_t max_samples)
{
    return ((size_t)max_samples * 8 + 15) & ~(size_t)15;
}

static void free_ctx(if_fir_combiner *c)
{
    if (!c)
        return;
    if_fir::stream_ctx_close(c, {c->d_taps, c->d_H[0], c->d_H[1], c->d_tw, c->hist.buf[0], c->hist.buf[1], c->d_stage_in, c->d_stage_out});
    delete c;
}

// centres -> plan (tab_cur untouched) and, for the overlap-save range, the residual tables 1 .. *ntables - 1 in `tables`
// (table 0, the plain H, is built once at init); false with the message set when a centre is out of range
static bool make_plan(char *err, const char *who, const if_fir_combiner *c, const double *pdCentre, combiner_plan *p,
                      std::vector<float2> *tables, int *ntables)
{
    if (!pdCentre)
    {
        set_err(err, "%s: pdCentre is NULL", who);
        return false;
    }
    int32_t residual[if_fir::COMBINER_MAX_CHANNELS + 1] = {0};
    int nt = 1;
    for (int ch = 0; ch < c->C; ch++)
    {
        const double f = pdCentre[ch];
        if (!std::isfinite(f) || std::fabs(f) > 0.5)
        {
            set_err(err, "%s: centre %d must be within +-0.5 cycles/sample (got %g)", who, ch, f);
            return false;
        }
        const uint32_t P = if_fir::nco_word_of(f);
        uint32_t G;
        int32_t r;
        if_fir::combiner_split_word(P, &G, &r);
        int t = 0;
        while (t < nt && residual[t] != r)
            t++;
        if (t == nt)
            residual[nt++] = r;
        p->word[ch] = P;
        p->rword[ch] = (uint32_t)r;
        p->G[ch] = (uint16_t)(G & 4095u);
        p->table[ch] = (uint16_t)t;
    }
    *ntables = nt;
    if (tables && if_fir::combiner_fft_supported(c->T, c->L))
    {
        tables->resize((size_t)nt * if_fir::INTERP_N);
        for (int t = 1; t < nt; t++)
            if_fir::combiner_build_table(c->taps.data(), c->T, c->ctaps, residual[t], tables->data() + (size_t)t * if_fir::INTERP_N);
    }
    return true;
}

static uint8_t combiner_init(if_fir_combiner_t **ppCtx, const float *pfTaps, uint32_t ulTaps, uint32_t ulL, uint32_t ulChannels,
                             const double *pdCentre, uint64_t ullMax, int32_t lDevice, int ctaps)
{
    if (!if_fir::stream_ctx_init_begin(g_combiner_init_err, "if_fir_combiner_init", ppCtx))
        return 0;
    if (!pfTaps || ulTaps == 0 || ulTaps > IF_FIR_MAX_TAPS)
    {
        set_err(g_combiner_init_err, "if_fir_combiner_init: taps must be 1..%u (got %u)%s", IF_FIR_MAX_TAPS, ulTaps, pfTaps ? "" : ", pfTaps is NULL");
        return 0;
    }
    if (ulL < 1 || ulL > IF_FIR_MAX_INTERPOLATION)
    {
        set_err(g_combiner_init_err, "if_fir_combiner_init: interpolation must be 1..%u (got %u)", IF_FIR_MAX_INTERPOLATION, ulL);
        return 0;
    }
    if (ulChannels < 1 || ulChannels > IF_FIR_COMBINER_MAX_CHANNELS)
    {
        set_err(g_combiner_init_err, "if_fir_combiner_init: channels must be 1..%u (got %u)", IF_FIR_COMBINER_MAX_CHANNELS, ulChannels);
        return 0;
    }
    if (ullMax == 0 || ullMax > ((uint64_t)1 << 40) / ulL)
    {
        set_err(g_combiner_init_err, "if_fir_combiner_init: ullMaxSamples must be 1..2^40/L (got %llu)", (unsigned long long)ullMax);
        return 0;
    }
    if_fir_combiner *c = new (std::nothrow) if_fir_combiner();
    if (!c)
    {
        set_err(g_combiner_init_err, "if_fir_combiner_init: out of host memory");
        return 0;
    }
    c->T = (int)ulTaps;
    c->L = (int)ulL;
    c->C = (int)ulChannels;
    c->ctaps = ctaps;
    const size_t tap_floats = (size_t)ulTaps * (ctaps ? 2 : 1);
    c->taps.assign(pfTaps, pfTaps + tap_floats);
    std::vector<float2> tables;
    int ntables = 0;
    if (!make_plan(g_combiner_init_err, "if_fir_combiner_init", c, pdCentre, &c->plan, &tables, &ntables) ||
        !if_fir::stream_ctx_device_ok(g_combiner_init_err, "if_fir_combiner_init", lDevice))
    {
        delete c;
        return 0;
    }
    c->backend_req = IF_FIR_BACKEND_AUTO;
    c->backend = resolve_backend(c, IF_FIR_BACKEND_AUTO);
    c->hist_len = if_fir::interp_hist_len(c->T, c->L);
    hipError_t e = if_fir::stream_ctx_open(c, lDevice, ullMax);
    if_fir::stream_ctx_alloc_upload(e, &c->d_taps, pfTaps, tap_floats * sizeof(float));
    if_fir::stream_history_alloc(e, &c->hist, (size_t)c->C * c->hist_len * sizeof(float2), 0);
    if (e == hipSuccess && if_fir::combiner_fft_supported(c->T, c->L))
    {
        std::vector<float2> tw(if_fir::INTERP_N);
        if_fir::interp_build_tables(pfTaps, c->T, ctaps, tables.data(), tw.data()); // table 0: the interpolator's H
        const size_t image = (size_t)(c->C + 1) * if_fir::INTERP_N * sizeof(float2);
        for (int i = 0; i < 2; i++)
            if_fir::stream_ctx_alloc_zeroed(e, &c->d_H[i], image);
        if (e == hipSuccess)
            e = hipMemcpy(c->d_H[0], tables.data(), tables.size() * sizeof(float2), hipMemcpyHostToDevice);
        if (e == hipSuccess)
            e = hipMemcpy(c->d_H[1], tables.data(), if_fir::INTERP_N * sizeof(float2), hipMemcpyHostToDevice);
        if_fir::stream_ctx_alloc_upload(e, &c->d_tw, tw.data(), tw.size() * sizeof(float2));
    }
    if (e == hipSuccess)
        e = hipMalloc(&c->d_stage_in, stage_pitch(ullMax) * c->C);
    if (e == hipSuccess)
        e = hipMalloc(&c->d_stage_out, (size_t)ullMax * ulL * 8);
    return if_fir::stream_ctx_init_end(g_combiner_init_err, "if_fir_combiner_init", e, c, ppCtx, free_ctx);
}

IF_FIR_API uint8_t if_fir_combiner_init(if_fir_combiner_t **ppCtx, const float *pfTaps, uint32_t ulTaps, uint32_t ulInterpolation,
                                        uint32_t ulChannels, const double *pdCentre, uint64_t ullMaxSamples, int32_t lDevice)
{
    return combiner_init(ppCtx, pfTaps, ulTaps, ulInterpolation, ulChannels, pdCentre, ullMaxSamples, lDevice, 0);
}

IF_FIR_API uint8_t if_fir_combiner_init_complex(if_fir_combiner_t **ppCtx, const float *pfTapsIQ, uint32_t ulTaps, uint32_t ulInterpolation,
                                                uint32_t ulChannels, const double *pdCentre, uint64_t ullMaxSamples, int32_t lDevice)
{
    return combiner_init(ppCtx, pfTapsIQ, ulTaps, ulInterpolation, ulChannels, pdCentre, ullMaxSamples, lDevice, 1);
}

IF_FIR_API void if_fir_combiner_destroy(if_fir_combiner_t *pCtx)
{
    free_ctx(pCtx);
}

IF_FIR_API const char *if_fir_combiner_last_error(const if_fir_combiner_t *pCtx)
{
    return pCtx ? pCtx->err : g_combiner_init_err;
}

IF_FIR_API uint8_t if_fir_combiner_reset(if_fir_combiner_t *pCtx)
{
    if (!pCtx || !if_fir::stream_history_zero(pCtx, pCtx->hist))
        return 0;
    pCtx->st.consumed = 0;
    return 1;
}

IF_FIR_API uint8_t if_fir_combiner_set_backend(if_fir_combiner_t *pCtx, uint32_t ulBackend)
{
    if (!pCtx)
        return 0;
    if (ulBackend != IF_FIR_BACKEND_AUTO && ulBackend != IF_FIR_BACKEND_HIP_FFT && ulBackend != IF_FIR_BACKEND_HIP_GENERIC)
    {
        set_err(pCtx->err, "if_fir_combiner_set_backend: backend %u does not combine (AUTO, HIP_FFT or HIP_GENERIC)", ulBackend);
        return 0;
    }
    if (ulBackend == IF_FIR_BACKEND_HIP_FFT && !if_fir::combiner_fft_supported(pCtx->T, pCtx->L))
    {
        set_err(pCtx->err, "if_fir_combiner_set_backend: the overlap-save backend takes L in {4, 8, 16, 32, 64} and <= %d taps "
                      "(L = %d, %d taps)", if_fir::INTERP_FFT_MAX_TAPS, pCtx->L, pCtx->T);
        return 0;
    }
    pCtx->backend_req = ulBackend;
    pCtx->backend = resolve_backend(pCtx, ulBackend);
    return 1;
}

IF_FIR_API uint32_t if_fir_combiner_get_backend(const if_fir_combiner_t *pCtx)
{
    return pCtx ? pCtx->backend : 0u;
}

IF_FIR_API uint8_t if_fir_combiner_set_input_format(if_fir_combiner_t *pCtx, uint32_t ulFormat)
{
    return if_fir::stream_ctx_set_input_format(pCtx, "if_fir_combiner_set_input_format", ulFormat);
}

IF_FIR_API uint8_t if_fir_combiner_set_centres(if_fir_combiner_t *pCtx, const double *pdCentre)
{
    if (!pCtx)
        return 0;
    combiner_plan p = pCtx->plan;
    std::vector<float2> tables;
    int ntables = 0;
    if (!make_plan(pCtx->err, "if_fir_combiner_set_centres", pCtx, pdCentre, &p, &tables, &ntables))
        return 0;
    if (pCtx->d_H[0] && ntables > 1)
    {
        // into the image the kernels in flight do not read; the plan changes hands only once the tables are on the device
        p.tab_cur = pCtx->plan.tab_cur ^ 1;
        HIP_TRY(pCtx, hipSetDevice(pCtx->device));
        HIP_TRY(pCtx, hipMemcpyAsync(pCtx->d_H[p.tab_cur] + if_fir::INTERP_N, tables.data() + if_fir::INTERP_N,
                                     (size_t)(ntables - 1) * if_fir::INTERP_N * sizeof(float2), hipMemcpyHostToDevice, pCtx->stream));
        HIP_TRY(pCtx, hipStreamSynchronize(pCtx->stream));
    }
    pCtx->plan = p;
    return 1;
}

IF_FIR_API uint8_t if_fir_combiner_get_centres(const if_fir_combiner_t *pCtx, double *pdCentre)
{
    if (!pCtx || !pdCentre)
        return 0;
    for (int ch = 0; ch < pCtx->C; ch++)
        pdCentre[ch] = if_fir::nco_freq_of(pCtx->plan.word[ch]);
    return 1;
}

IF_FIR_API uint8_t if_fir_combiner_set_stream(if_fir_combiner_t *pCtx, void *pStream)
{
    return if_fir::stream_ctx_set_stream(pCtx, pStream);
}

IF_FIR_API uint8_t if_fir_combiner_synchronize(if_fir_combiner_t *pCtx)
{
    return if_fir::stream_ctx_synchronize(pCtx);
}

IF_FIR_API uint64_t if_fir_combiner_out_count(const if_fir_combiner_t *pCtx, uint64_t ullSamples)
{
    return pCtx ? ullSamples * (uint64_t)pCtx->L : 0;
}

static uint8_t run_device(if_fir_combiner *c, const void *const *in, void *out, uint64_t n, uint64_t *pout, const char *who)
{
    if (n > ((uint64_t)1 << 40) / (uint64_t)c->L)
    {
        set_err(c->err, "%s: sample count too large", who);
        return 0;
    }
    if (!in)
    {
        set_err(c->err, "%s: the array of input pointers is NULL", who);
        return 0;
    }
    const bool fft = c->backend == IF_FIR_BACKEND_HIP_FFT;
    const uintptr_t in_mask = fft ? (c->in_i16 ? 3 : 7) : 15, out_mask = fft ? 7 : 15;
    uintptr_t in_bits = 0;
    bool in_null = false;
    for (int ch = 0; ch < c->C; ch++)
    {
        in_bits |= (uintptr_t)in[ch];
        in_null = in_null || !in[ch];
    }
    if ((in_bits & in_mask) || ((uintptr_t)out & out_mask))
    {
        set_err(c->err, "%s: device pointers must be %u-byte (input) and %u-byte (output) aligned for this backend", who,
                (unsigned)in_mask + 1, (unsigned)out_mask + 1);
        return 0;
    }
    if (n && (in_null || !out))
    {
        set_err(c->err, "%s: NULL device pointer", who);
        return 0;
    }
    const uint64_t m = n * (uint64_t)c->L;
    if (pout)
        *pout = m;
    if (n == 0)
        return 1;
    if (if_fir::stream_ctx_capturing(c, who))
        return 0;
    HIP_TRY(c, hipSetDevice(c->device));
    if_fir::CombinerArgs a{};
    for (int ch = 0; ch < c->C; ch++)
    {
        a.ch.in[ch] = in[ch];
        a.ch.rword[ch] = c->plan.rword[ch];
        a.ch.G[ch] = c->plan.G[ch];
        a.ch.table[ch] = c->plan.table[ch];
    }
    a.C = c->C;
    a.out = out;
    a.hist = c->hist.at<float2>(c->st.hist_cur);
    a.hist_out = c->hist.at<float2>(c->st.hist_cur ^ 1);
    a.hist_len = c->hist_len;
    a.H = c->d_H[c->plan.tab_cur];
    a.tw = c->d_tw;
    a.taps = c->d_taps;
    a.T = c->T;
    a.L = c->L;
    a.ctaps = c->ctaps;
    a.in_i16 = c->in_i16;
    a.N = (int64_t)n;
    a.M = (int64_t)m;
    a.first_out = (uint32_t)(c->st.consumed * (uint64_t)c->L);
    a.grid_limit = c->grid_limit;
    a.device = c->device;
    a.stream = c->stream;
    HIP_TRY(c, fft ? if_fir::launch_combiner_fft(a) : if_fir::launch_combiner_generic(a));
    c->st.consumed += n;
    c->st.hist_cur ^= 1;
    return 1;
}

IF_FIR_API uint8_t if_fir_combiner_process_device(if_fir_combiner_t *pCtx, const void *const *ppDevIn, void *pDevOut, uint64_t ullSamples,
                                                  uint64_t *pullOutSamples)
{
    if (!pCtx)
        return 0;
    return run_device(pCtx, ppDevIn, pDevOut, ullSamples, pullOutSamples, "if_fir_combiner_process_device");
}

IF_FIR_API uint8_t if_fir_combiner_process(if_fir_combiner_t *pCtx, const void *const *ppIQIn, float *pfIQOut, uint64_t ullSamples,
                                           uint64_t *pullOutSamples)
{
    if (!pCtx)
        return 0;
    if (!if_fir::stream_ctx_fits(pCtx, "if_fir_combiner_process", ullSamples))
        return 0;
    bool in_null = !ppIQIn;
    for (int ch = 0; ppIQIn && ch < pCtx->C; ch++)
        in_null = in_null || !ppIQIn[ch];
    if (!ppIQIn || (ullSamples && (in_null || !pfIQOut)))
    {
        set_err(pCtx->err, "if_fir_combiner_process: NULL buffer");
        return 0;
    }
    if (pullOutSamples)
        *pullOutSamples = 0;
    if (ullSamples == 0)
        return 1;
    // channel ch is staged at ch x stage_pitch bytes; channels 1 .. C-1 are copied here, channel 0 by the shared staged call, on
    // the same stream
    const size_t elem = pCtx->in_i16 ? 4 : 8, pitch = stage_pitch(pCtx->max_samples);
    const void *dev_in[if_fir::COMBINER_MAX_CHANNELS];
    HIP_TRY(pCtx, hipSetDevice(pCtx->device));
    for (int ch = 0; ch < pCtx->C; ch++)
    {
        dev_in[ch] = static_cast<char *>(pCtx->d_stage_in) + ch * pitch;
        if (ch)
            HIP_TRY(pCtx, hipMemcpyAsync(const_cast<void *>(dev_in[ch]), ppIQIn[ch], (size_t)ullSamples * elem, hipMemcpyHostToDevice,
                                         pCtx->stream));
    }
    uint64_t m = 0;
    if (!if_fir::stream_ctx_staged(
            pCtx, "if_fir_combiner_process", "outputs", pCtx->d_stage_in, ppIQIn[0], ullSamples, &pCtx->st,
            [&] { return run_device(pCtx, dev_in, pCtx->d_stage_out, ullSamples, &m, "if_fir_combiner_process"); },
            [&] { return hipMemcpyAsync(pfIQOut, pCtx->d_stage_out, (size_t)m * 8, hipMemcpyDeviceToHost, pCtx->stream); }))
        return 0;
    if (pullOutSamples)
        *pullOutSamples = m;
    return 1;
}

#ifdef IF_FIR_DEVELOPMENT
IF_FIR_API uint8_t if_fir_debug_combiner_config(if_fir_combiner_t *pCtx, uint32_t ulGridLimit)
{
    if (!pCtx)
        return 0;
    pCtx->grid_limit = if_fir::stream_ctx_grid_limit(ulGridLimit);
    return 1;
}

IF_FIR_API uint8_t if_fir_debug_combiner_seek(if_fir_combiner_t *pCtx, uint64_t ullSamples)
{
    if (!pCtx)
        return 0;
    pCtx->st.consumed = ullSamples;
    return 1;
}

IF_FIR_API uint32_t if_fir_debug_combiner_tables(const float *pfTaps, uint32_t ulTaps, uint32_t bComplexTaps, double dCentre,
                                                 uint32_t *pulGrid, int32_t *plResidual, float *pfOut, uint32_t ulOutFloats)
{
    if (!pfTaps || !pulGrid || !plResidual || !pfOut || ulOutFloats < 2u * if_fir::INTERP_N ||
        !if_fir::interp_fft_supported((int)ulTaps, 4) || !std::isfinite(dCentre) || std::fabs(dCentre) > 0.5)
        return 0;
    if_fir::combiner_split_word(if_fir::nco_word_of(dCentre), pulGrid, plResidual);
    std::vector<float2> H(if_fir::INTERP_N);
    if_fir::combiner_build_table(pfTaps, (int)ulTaps, bComplexTaps ? 1 : 0, *plResidual, H.data());
    memcpy(pfOut, H.data(), H.size() * sizeof(float2));
    return 2u * if_fir::INTERP_N;
}
#endif
